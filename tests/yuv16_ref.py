"""Numpy restatement of the 10-bit YUV input (include/nquant_abi.h "10-bit YUV input"), independent of the library and
written from the header's text: the coefficients as floor(16384 e + 1/2) of the exact rationals (fractions), the sample taken from the
high or the low ten bits of its word, the per-pixel integer matrix with the arithmetic shift and the clamp to 12 bits, sample replication
of the chroma, then either the scaling to 8 bits (SDR) or E[] -> the gamut rows -> the logarithmic index -> O[] (PQ, HLG) with the tables
READ from include/nq_hdr_luts.inc (never recomputed), and the fused call as the conversion followed by resample_ref.resample.  convert()
and resample() are what the GPU tests compare against, word for word.  exact() states the same pipeline in float64 with no table and
no fixed point."""
import os
import re
from fractions import Fraction

import numpy as np

import resample_ref

BT709, FULL_RANGE, BT2020, MSB, PQ, HLG = 1, 2, 4, 8, 16, 32
LINEAR = resample_ref.LINEAR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the header's table: (matrix bits, full range) -> (cy, crv, cgu, cgv, cbu)
HEADER_TABLE = {(0, False): (76590, 104982, 25769, 53475, 132687), (0, True): (65584, 91949, 22570, 46836, 116215),
                (BT709, False): (76590, 117921, 14027, 35053, 138947), (BT709, True): (65584, 103282, 12285, 30701, 121698),
                (BT2020, False): (76590, 110418, 12322, 42783, 140879), (BT2020, True): (65584, 96710, 10792, 37472, 123390)}
GAMUT = ((6801, -2407, -298), (-510, 4640, -34), (-75, -412, 4583))


def load_tables(path=None):
    """{name: int64 array} of the four tables of include/nq_hdr_luts.inc."""
    src = open(path or os.path.join(ROOT, "include", "nq_hdr_luts.inc")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"NQ_HDR_LUT\(\s*([\w ]+?)\s*,\s*(\w+)\s*,\s*(\d+)\s*\)\s*=\s*\{(.*?)\};", src, re.S):
        vals = np.array([int(v) for v in m.group(4).replace("\n", "").split(",") if v.strip()], np.int64)
        assert vals.size == int(m.group(3)), m.group(2)
        assert vals.min() >= 0 and vals.max() < (65536 if m.group(1) == "unsigned short" else 256), m.group(2)
        out[m.group(2)] = vals
    assert sorted(out) == ["NQ_HDR_E_HLG", "NQ_HDR_E_PQ", "NQ_HDR_O_HLG", "NQ_HDR_O_PQ"]
    return out


TABLES = load_tables()


def tables(flags):
    """(E, O) of the flag word's transfer."""
    name = "PQ" if flags & PQ else "HLG"
    return TABLES["NQ_HDR_E_" + name], TABLES["NQ_HDR_O_" + name]


def rationals(flags):
    """(cy, crv, cgu, cgv, cbu) as exact fractions on the 12-bit scale, and the luma offset yo."""
    if flags & BT2020:
        kr, kb = Fraction(2627, 10000), Fraction(593, 10000)
    elif flags & BT709:
        kr, kb = Fraction(2126, 10000), Fraction(722, 10000)
    else:
        kr, kb = Fraction(299, 1000), Fraction(114, 1000)
    kg = 1 - kr - kb
    sy, sc = (Fraction(4095, 1023), Fraction(4095, 1023)) if flags & FULL_RANGE else (Fraction(4095, 876), Fraction(4095, 896))
    return (sy, sc * 2 * (1 - kr), sc * 2 * (1 - kb) * kb / kg, sc * 2 * (1 - kr) * kr / kg, sc * 2 * (1 - kb)), (0 if flags & FULL_RANGE else 64)


def coefficients(flags):
    """floor(16384 e + 1/2) of the rationals, as Python ints, and yo."""
    es, yo = rationals(flags)
    return tuple(int((16384 * e + Fraction(1, 2)).__floor__()) for e in es), yo


def samples(words, flags):
    """The 10-bit samples of 16-bit words: the high ten bits with MSB, else the low ten; the other six are ignored."""
    w = np.asarray(words).astype(np.int64)
    return (w >> 6) & 1023 if flags & MSB else w & 1023


def signal12(Y, U, V, flags):
    """Step 1: (R', G', B') on the 12-bit scale, int64 arrays in 0..4095, of 10-bit samples Y, U, V."""
    (cy, crv, cgu, cgv, cbu), yo = coefficients(flags)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    l = cy * (Y - yo) + 8192
    u, v = U - 512, V - 512
    terms = (l + crv * v, l - cgu * u - cgv * v, l + cbu * u)
    assert max(int(np.abs(t).max()) for t in terms + (l,)) < 160_000_000
    return tuple(np.clip(t >> 14, 0, 4095) for t in terms)           # numpy's >> on signed integers is the arithmetic shift


def index(l):
    """The index of O for linear light l (int64 array, 0..65535)."""
    l = np.asarray(l).astype(np.int64)
    e = 8 + sum((l >= (1 << k)).astype(np.int64) for k in range(9, 16))             # 31 - clz(l) for 256 <= l < 2^16
    return np.where(l < 256, l, 256 + 128 * (e - 8) + ((l >> (e - 7)) & 127))


def pixel(Y, U, V, flags):
    """The three 8-bit channels of 10-bit samples Y, U, V by the header's integer pipeline: (R, G, B) int64 arrays in 0..255."""
    c = signal12(Y, U, V, flags)
    if not flags & (PQ | HLG):
        return tuple((v * 255 + 2047) // 4095 for v in c)
    E, O = tables(flags)
    e = [E[v] for v in c]
    out = []
    for row in GAMUT:
        terms = [k * v for k, v in zip(row, e)]
        assert max(int(np.abs(t).max()) for t in terms) < 450_000_000
        out.append(O[index(np.clip((terms[0] + terms[1] + terms[2] + 2048) >> 12, 0, 65535))])
    return tuple(out)


# ---- the same pipeline in float64: no tables, no fixed point ----
_M1, _M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
_C1, _C2, _C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
_HA, _HB, _HC = 0.17883277, 0.28466892, 0.55991073


def pq_eotf(x):
    p = np.power(np.asarray(x, np.float64), 1.0 / _M2)
    return np.power(np.maximum(p - _C1, 0.0) / (_C2 - _C3 * p), 1.0 / _M1)


def hlg_inverse_oetf(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.5, x * x / 3.0, (np.exp((x - _HC) / _HA) + _HB) / 12.0)


def srgb_encode(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 1e-300), 1.0 / 2.4) - 0.055)


def tone(x, p):
    return np.minimum(1.0, x * (1.0 + x / (p * p)) / (1.0 + x))


def linear_light(signal, flags):
    """Signal 0..1 -> linear light with 1 = reference white, saturating where E does (65535 / 8192)."""
    if flags & PQ:
        return np.minimum(65535.0 / 8192.0, 10000.0 * pq_eotf(signal) / 203.0)
    return hlg_inverse_oetf(signal) / float(hlg_inverse_oetf(0.75))


def peak(flags):
    return 65535.0 / 8192.0 if flags & PQ else float(hlg_inverse_oetf(1.0) / hlg_inverse_oetf(0.75))


def exact(Y, U, V, flags, rounded=True):
    """The real-valued pipeline in float64: the matrix from the rationals, the clamp to the signal range, then SDR: 255 c, or PQ / HLG:
    the EOTF, the BT.2020 -> BT.709 matrix of the GAMUT rows / 4096, the clamp to the table's range, the tone curve and the sRGB
    encoding.  rounded: round-half-up to int64 levels, else the real levels."""
    es, yo = rationals(flags)
    cy, crv, cgu, cgv, cbu = (float(e) / 4095.0 for e in es)
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    l, u, v = cy * (Y - yo), U - 512.0, V - 512.0
    c = [np.clip(t, 0.0, 1.0) for t in (l + crv * v, l - cgu * u - cgv * v, l + cbu * u)]
    if not flags & (PQ | HLG):
        levels = [255.0 * t for t in c]
    else:
        e = [linear_light(t, flags) for t in c]
        p = peak(flags)
        levels = []
        for row in GAMUT:
            x = np.clip((row[0] * e[0] + row[1] * e[1] + row[2] * e[2]) / 4096.0, 0.0, 65535.0 / 8192.0)
            levels.append(255.0 * srgb_encode(tone(x, p)))
    if not rounded:
        return tuple(levels)
    return tuple(np.clip(np.floor(t + 0.5), 0, 255).astype(np.int64) for t in levels)


def convert_one(y, u, v, flags):
    """One frame: y (h, w), u and v ((h + 1) // 2, (w + 1) // 2) uint16 arrays of WORDS (any strides) -> int32 ARGB array (h, w)."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    h, w = y.shape
    assert u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    rows, cols = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    r, g, b = pixel(samples(y, flags), samples(u, flags)[rows, cols], samples(v, flags)[rows, cols], flags)
    word = np.int64(0xFF) << 24 | r << 16 | g << 8 | b
    return word.astype(np.uint32).view(np.int32)


def convert(frames, flags=0):
    """n frames (y, u, v) -> list of int32 ARGB arrays."""
    return [convert_one(y, u, v, flags) for y, u, v in frames]


def resample(frames, size=None, crop=None, flags=0, resample_flags=LINEAR):
    """The fused call: the conversion followed by the frame reduction with the same crop, target and flags."""
    return resample_ref.resample(convert(frames, flags), size, crop, resample_flags)


def random_planes(w, h, seed, flags=MSB):
    """(y, u, v) of random 10-bit samples in 16-bit words, tight, with junk in the six bits the flag word ignores."""
    rng = np.random.default_rng(seed)
    ch2, cw2 = (h + 1) // 2, (w + 1) // 2

    def plane(shape):
        s = rng.integers(0, 1024, shape, dtype=np.uint16)
        junk = rng.integers(0, 64, shape, dtype=np.uint16)
        return (s << 6 | junk) if flags & MSB else (junk << 10 | s)
    return plane((h, w)), plane((ch2, cw2)), plane((ch2, cw2))


def grid_chroma():
    """The 64 chroma pairs of the grid frame: the 9 combinations of {0, 512, 1023}, then 55 seeded ones."""
    rng = np.random.default_rng(2020)
    pairs = [(a, b) for a in (0, 512, 1023) for b in (0, 512, 1023)]
    pairs += [tuple(int(v) for v in rng.integers(0, 1024, 2)) for _ in range(55)]
    return pairs


def grid_frame(flags=MSB):
    """The grid frame, 1024 x 128: column x has Y = x, row pair r the chroma pair grid_chroma()[r].  Samples sit where the flag word
    reads them; the other six bits are 0."""
    pairs = grid_chroma()
    y = np.broadcast_to(np.arange(1024, dtype=np.uint16)[None, :], (128, 1024)).copy()
    u = np.broadcast_to(np.array([p[0] for p in pairs], np.uint16)[:, None], (64, 512)).copy()
    v = np.broadcast_to(np.array([p[1] for p in pairs], np.uint16)[:, None], (64, 512)).copy()
    if flags & MSB:
        y, u, v = y << 6, u << 6, v << 6
    return y, u, v
