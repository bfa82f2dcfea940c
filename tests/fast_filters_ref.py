"""Host references and input domains of the dither kernel's filter tests (test_fast_filters_cpu.py, test_gpu_fast_filters.py)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "nquant.android_amd", "csrc", "nq_dither_fast.hip")


def bits_to_f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


# ---- tanh: the floats with 0.5 <= |x| < 9.2 (the comparison is made in f64: the float nearest to 9.2 lies below it)
TANH_FIRST = int(np.float32(0.5).view(np.uint32))
TANH_COUNT = int(np.float32(9.2).view(np.uint32)) - TANH_FIRST + (1 if float(np.float32(9.2)) < 9.2 else 0)
# half-width of the disputed window.  Where numpy's f64 tanh is further than this from a rounding boundary, every evaluation within
# 1e-15 of tanh (the kernel's stated error, numpy's last place, a device library) narrows to the same float
TANH_WINDOW = 1.2e-14


def tanh_reference(x32):
    """(float32 reference, disputed mask) for positive or negative float32 inputs."""
    v = np.tanh(x32.astype(np.float64))
    lo, hi = (v - TANH_WINDOW).astype(np.float32), (v + TANH_WINDOW).astype(np.float32)
    return v.astype(np.float32), lo != hi


_disputed = None


def tanh_disputed_bits(chunk=1 << 22):
    """Bit patterns (positive sign) of the disputed inputs of the whole domain."""
    global _disputed
    if _disputed is None:
        found = []
        for s in range(0, TANH_COUNT, chunk):
            bits = np.arange(TANH_FIRST + s, TANH_FIRST + min(s + chunk, TANH_COUNT), dtype=np.uint32)
            found.append(bits[tanh_reference(bits.view(np.float32))[1]])
        _disputed = np.concatenate(found)
    return _disputed


# ---- closestColorIndex err, NQ/PnnLABQuantizer.java:421-445 without semi-transparency, statement by statement
COEFFS = np.array([[0.299, 0.587, 0.114], [-0.14713, -0.28886, 0.436], [0.615, -0.51499, -0.10001]], np.float32)


def closest_err_numpy(PR, PG, PB, ratio, pairs):
    c, c2 = pairs[:, 0].view(np.uint32), pairs[:, 1].view(np.uint32)
    d = [((c2 >> s) & 0xFF).astype(np.int32) - ((c >> s) & 0xFF).astype(np.int32) for s in (16, 8, 0)]
    err = PR * (1 - ratio) * np.square(d[0].astype(np.float64))
    err = err + PG * (1 - ratio) * np.square(d[1].astype(np.float64))
    err = err + PB * (1 - ratio) * np.square(d[2].astype(np.float64))
    for i in range(3):
        for j in range(3):
            err = err + ratio * np.square((COEFFS[i, j] * d[j].astype(np.float32)).astype(np.float64))
    return err


def unpack_triples(packed, mask):
    """{colour, palette entry} of packed |dr| << 16 | |dg| << 8 | |db| under a sign mask, as the CLOSEST_ERR mode of nq_selftest_fast
    builds them: a negative difference puts the magnitude into the colour, a positive one into the palette entry."""
    packed = np.asarray(packed, np.uint32)
    neg = np.uint32(sum(0xFF << (8 * j) for j in range(3) if (mask >> j) & 1))
    c = (packed & neg) | np.uint32(0xFF000000)
    c2 = (packed & ~neg & np.uint32(0xFFFFFF)) | np.uint32(0xFF000000)
    return np.stack([c, c2], axis=1).view(np.int32)


# ---- random.nextInt(32767): one draw uu = next(31) -> (uu % bound, accepted), java.util.Random.nextInt(int) in 64-bit integers
def nextint_ref(uu):
    uu = np.asarray(uu, np.int64)
    r = uu % 32767
    return r, ~(uu - r + 32766 >= 2 ** 31)


def rem_ref(r, dsum):
    """r % (closest[3] + closest[2]) as Java computes it for 0 <= r < 32767 and an int32 divisor (never 0 where it is evaluated)."""
    r, dsum = np.asarray(r, np.int64), np.asarray(dsum, np.int64)
    return np.where(dsum != 0, np.fmod(r, np.where(dsum == 0, 1, dsum)), r)


# ---- constants of the kernel source
def near_eps():
    """NQ_FAST_NEAR_EPS as the kernel source defines it."""
    m = re.findall(r"^#define NQ_FAST_NEAR_EPS ([0-9.e+-]+)f$", open(KERNEL_SOURCE).read(), re.M)
    assert len(m) == 1, m
    return float(m[0])


def kernel_constants():
    src = open(KERNEL_SOURCE).read()

    def one(pattern):
        m = re.findall(pattern, src, re.M)
        assert len(m) == 1, (pattern, m)
        return m[0]
    k = {}
    k["near_eps"] = near_eps()
    k["safe_factor"] = float(one(r"^    safe = d2 - d1 > ([0-9.e+-]+)f \* NQ_FAST_NEAR_EPS;$"))
    rel, ab = one(r"^    const float delta = __builtin_fmaf\(e, ([0-9.e+-]+)f, ([0-9.e+-]+)f\);$")
    k["delta_rel"], k["delta_abs"] = float(rel), float(ab)
    sw = set(re.findall(r"fabsf\(yd - thr32\) > ([0-9.e+-]+)f", src))
    assert len(sw) == 1, sw
    k["ydiff_switch"] = float(sw.pop())
    lo, hi = one(r"^        const float lo = \(float\) \(v - ([0-9.e+-]+)\), hi = \(float\) \(v \+ ([0-9.e+-]+)\);$")
    assert lo == hi
    k["tanh_window"] = float(lo)
    return k
