"""The quality measurement's definition (include/nquant_abi.h "quality measurement") as restated in compare_ref.py, without a GPU:
known answers, the properties the GPU tests rely on, the claim the measurement exists for (dither raises the per-pixel error and lowers
the error of the block means), the library's argument checks as far as they go without a device, and the constants of the kernel that
tests/test_gpu_compare.py counts with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import compare_ref
import conftest
import ordered_ref
import resample_ref
from nquant.android_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
BLACK, WHITE = 0xFF000000, 0xFFFFFFFF


def _full(w, h, word):
    return np.full((h, w), word, np.uint32)


def _checker(w, h, first=BLACK, second=WHITE):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + yy) & 1, second, first).astype(np.uint32)


def sample():
    rgb = np.load(os.path.join(HERE, "golden", "sample_495x438.npz"))["rgb"]
    return synth.tile_photo(rgb, rgb.shape[1], rgb.shape[0])


# ---- known answers (slots 0..12, linear) ----
def test_black_against_white_16x16():
    """Means 0 and 65535: 65535^2 = 4294836225 per block and channel; l = floor(32768 * 26634 / 266369034) = 3 per block (N = 64,
    C1 = 26634, Sy = 16320), cs = 32768 (no variance on either side)."""
    got = compare_ref.compare(_full(16, 16, BLACK), _full(16, 16, WHITE))
    assert got[:13].tolist() == [256, 4, 0, 16646400, 16646400, 16646400, 255, 0, 17179344900, 17179344900, 17179344900, 12, 32765]
    assert got[13:].tolist() == [0, 0, 0]


def test_black_against_white_1x1():
    got = compare_ref.compare(_full(1, 1, BLACK), _full(1, 1, WHITE))
    assert got[:13].tolist() == [1, 1, 0, 65025, 65025, 65025, 255, 0, 4294836225, 4294836225, 4294836225, 3, 32765]


def test_checkerboard_against_its_inverse():
    """Equal block means, opposite structure: lf is 0 and the SSIM negative."""
    got = compare_ref.compare(_checker(16, 16), _checker(16, 16, WHITE, BLACK))
    assert got[:13].tolist() == [256, 4, 0, 16646400, 16646400, 16646400, 255, 0, 0, 0, 0, -130604, 65419]


def test_sample_picture_against_itself():
    img = sample()
    got = compare_ref.compare(img, img)
    want = np.zeros(16, np.int64)
    want[0], want[1], want[11] = 216810, 3410, 111738880
    assert got.tolist() == want.tolist() and want[11] == 32768 * 3410


def test_partial_blocks_against_black():
    """Rows 0..8 and columns 0..8 of the checkerboard: four blocks of 64, 8, 8 and 1 pixels."""
    got = compare_ref.compare(_checker(16, 16)[:9, :9], _full(9, 9, BLACK))
    assert got[0] == 81 and got[1] == 4 and got[12] == 32768


# ---- properties ----
PAIRS = [(1, 1), (7, 5), (8, 8), (9, 9), (45, 37), (64, 64)]


@pytest.mark.parametrize("flags", [0, 1])
def test_identical_inputs(flags):
    for i, (w, h) in enumerate(PAIRS):
        a = resample_ref.random_argb(w, h, 100 + i)
        got = compare_ref.compare(a, a.copy(), flags)
        blocks = ((w + 7) // 8) * ((h + 7) // 8)
        want = np.zeros(16, np.int64)
        want[0], want[1], want[11] = w * h, blocks, 32768 * blocks
        assert got.tolist() == want.tolist()


@pytest.mark.parametrize("flags", [0, 1])
def test_every_slot_is_symmetric_and_within_its_bound(flags):
    for i, (w, h) in enumerate(PAIRS):
        a, b = resample_ref.random_argb(w, h, 200 + i), resample_ref.random_argb(w, h, 300 + i)
        ab, ba = compare_ref.compare(a, b, flags), compare_ref.compare(b, a, flags)
        assert ab.tolist() == ba.tolist()
        px, blocks = w * h, ((w + 7) // 8) * ((h + 7) // 8)
        assert ab[0] == px and ab[1] == blocks
        assert all(0 <= v <= 65025 * px for v in ab[2:6]) and 0 <= ab[6] <= 255
        assert all(0 <= v <= 65535 ** 2 * blocks for v in ab[7:11])
        assert -32768 * blocks <= ab[11] <= 32768 * blocks and 0 <= ab[12] <= 65536
        assert ab[13:].tolist() == [0, 0, 0]


def test_clear_pixels_on_both_sides_contribute_nothing():
    """a = 0 on both sides: whatever the colour bits are, the pair measures like the pair with those pixels zeroed."""
    a, b = resample_ref.random_argb(45, 37, 1), resample_ref.random_argb(45, 37, 2)
    clear = np.random.default_rng(3).random((37, 45)) < 0.4
    a2 = np.where(clear, a.view(np.uint32) & np.uint32(0x00FFFFFF), a.view(np.uint32))
    b2 = np.where(clear, b.view(np.uint32) & np.uint32(0x00FFFFFF), b.view(np.uint32))
    a3, b3 = np.where(clear, np.uint32(0), a2), np.where(clear, np.uint32(0), b2)
    assert (a2 != a3).any()
    for flags in (0, 1):
        assert compare_ref.compare(a2, b2, flags).tolist() == compare_ref.compare(a3, b3, flags).tolist()
    only = np.where(clear, np.uint32(0x00123456), np.uint32(0))          # nothing but clear pixels, with colour bits
    got = compare_ref.compare(only, np.zeros_like(only))
    assert got[2:11].tolist() == [0] * 9 and got[11] == 32768 * got[1] and got[12] == 0


def test_the_indexed_form_is_the_argb_form_of_palette_index():
    rng = np.random.default_rng(4)
    src = [resample_ref.random_argb(w, h, 400 + w) for w, h in PAIRS]
    for K in (1, 2, 256):
        pal = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
        pal[0] &= np.uint32(0x00FFFFFF)                                 # a fully transparent entry
        idx = [rng.integers(0, K, f.shape).astype(np.uint16) for f in src]
        got = compare_ref.compare_indexed(src, idx, pal)
        want = compare_ref.compare_frames(src, [pal[m] for m in idx])
        assert got.tolist() == want.tolist()
    idx[-1][0, 0] = 300                                                 # an index past the palette reads as the word 0
    zero = pal[idx[-1].clip(0, 255)]
    zero[0, 0] = 0
    assert compare_ref.compare_indexed(src[-1:], idx[-1:], pal).tolist() == compare_ref.compare_frames(src[-1:], [zero]).tolist()


# ---- the claim: dither raises the per-pixel error and lowers the error of the block means ----
@pytest.mark.parametrize("name", ["sample_lab16_dither", "sample_lab256_dither"])
def test_dither_raises_sse_and_lowers_the_block_mean_error(name):
    img = sample()
    palette = np.load(os.path.join(HERE, "golden", name + ".npz"))["palette"]
    nearest = ordered_ref.dither([img], palette, 0)[1][0]
    dithered = ordered_ref.dither([img], palette, 255)[1][0]
    for flags in (1, 0):
        plain, dith = compare_ref.compare(img, nearest, flags), compare_ref.compare(img, dithered, flags)
        print(name, flags, plain.tolist(), dith.tolist())
        assert (dith[3:6] > plain[3:6]).all()
        assert (dith[8:11] < plain[8:11]).all()
    if name == "sample_lab16_dither":                                   # the figures of the table in DESIGN.md 5k
        plain, dith = compare_ref.compare(img, nearest), compare_ref.compare(img, dithered)
        assert (plain[3], plain[8], plain[11]) == (48821977, 44057189345, 97747650)
        assert (dith[3], dith[8], dith[11]) == (68505645, 38322942955, 80711457)


# ---- the library without a device ----
SYMBOLS = ["nq_compare_frames_device", "nq_compare_indexed_device", "nq_compare_frames", "nq_compare_indexed"]


def test_the_four_exports_exist(nq):
    L = nq.load_library()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in nq.abi_symbols()
    assert "nq_handle" not in re.search(r"int nq_compare_frames_device\(([^)]*)\)", open(os.path.join(HERE, "..", "include", "nquant_abi.h")).read()).group(1)


class _Call:
    """One valid call of every entry point on host memory (a device form only ever gets as far as the argument checks here, or to a
    device that is not there), with fields to spoil."""

    def __init__(self, n=2, w=12, h=10):
        self.n, self.device, self.flags, self.K = n, 0, 1, 4
        self.src = [np.zeros((h, w), np.uint32) for _ in range(n)]
        self.out = [np.zeros((h, w), np.uint32) for _ in range(n)]
        self.idx = [np.zeros((h, w), np.uint16) for _ in range(n)]
        self.pal = np.arange(256, dtype=np.uint32)
        self.w, self.h = np.full(n, w, np.int32), np.full(n, h, np.int32)
        self.res = np.full(16 * n + 2, -7, np.int64)
        self.p_src = [a.ctypes.data for a in self.src]
        self.p_out = [a.ctypes.data for a in self.out]
        self.p_idx = [a.ctypes.data for a in self.idx]
        self.p_pal, self.p_w, self.p_h, self.p_res = self.pal.ctypes.data, self.w.ctypes.data, self.h.ctypes.data, self.res.ctypes.data + 8
        self.t_src = self.t_out = self.t_idx = True      # False: a NULL table

    def run(self, L, symbol):
        tab = lambda ptrs, on: (C.c_void_p * len(ptrs))(*ptrs) if on else None
        src = tab(self.p_src, self.t_src)
        indexed = "indexed" in symbol
        out = tab(self.p_idx, self.t_idx) if indexed else tab(self.p_out, self.t_out)
        args = [self.device] + ([None] if symbol.endswith("_device") else []) + [self.n, src, out]
        if indexed:
            args += [self.p_pal, self.K]
        args += [self.p_w, self.p_h, self.flags, self.p_res]
        return getattr(L, symbol)(*args)


def _spoilers():
    def setter(**kw):
        def f(c):
            for k, v in kw.items():
                setattr(c, k, v)
        return f

    def side(i, w, h):
        def f(c):
            c.w[i], c.h[i] = w, h
        return f

    def entry(name, i, v):
        def f(c):
            getattr(c, name)[i] = v
        return f

    def bump(name, i, by):
        def f(c):
            getattr(c, name)[i] += by
        return f

    both = [("n = 0", setter(n=0)), ("n = 65536", setter(n=65536)), ("n < 0", setter(n=-1)), ("width 0", side(1, 0, 10)),
            ("height 65536", side(0, 12, 65536)), ("negative width", side(0, -12, 10)), ("65535 x 65535 pixels", side(1, 65535, 65535)),
            ("unknown flag bits", setter(flags=2)), ("unknown flag bits (high)", setter(flags=1 | 1 << 30)), ("negative device", setter(device=-1)),
            ("NULL source table", setter(t_src=False)), ("NULL source entry", entry("p_src", 1, None)),
            ("NULL widths", setter(p_w=None)), ("NULL heights", setter(p_h=None)), ("NULL result", setter(p_res=None)),
            ("source not 4-byte aligned", bump("p_src", 0, 2)), ("result not 8-byte aligned", lambda c: setattr(c, "p_res", c.p_res + 4)),
            ("result inside a source frame", lambda c: setattr(c, "p_res", c.p_src[1] + 8))]
    argb = [("NULL output table", setter(t_out=False)), ("NULL output entry", entry("p_out", 0, None)),
            ("output not 4-byte aligned", bump("p_out", 1, 2)), ("result inside an output", lambda c: setattr(c, "p_res", c.p_out[0] + 16))]
    indexed = [("K = 0", setter(K=0)), ("K = 257", setter(K=257)), ("NULL palette", setter(p_pal=None)), ("NULL index table", setter(t_idx=False)),
               ("NULL index entry", entry("p_idx", 1, None)), ("index map not 2-byte aligned", bump("p_idx", 0, 1)),
               ("result inside an index map", lambda c: setattr(c, "p_res", c.p_idx[1] + 8))]
    return both, argb, indexed


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_invalid_arguments_are_refused_before_any_device(nq, symbol):
    L = nq.load_library()
    both, argb, indexed = _spoilers()
    for what, spoil in both + (indexed if "indexed" in symbol else argb):
        c = _Call()
        spoil(c)
        keep = [a.copy() for a in c.src + c.out + c.idx]
        assert c.run(L, symbol) == -1, what
        assert (c.res == -7).all(), what
        assert all((a == b).all() for a, b in zip(keep, c.src + c.out + c.idx)), what
        assert L.nq_last_error(None), what


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_valid_arguments_need_a_device(nq, symbol):
    if conftest.HAS_GPU:
        return              # a device is present: tests/test_gpu_compare.py runs the valid calls (a device form must not see host memory)
    L = nq.load_library()
    c = _Call()
    assert c.run(L, symbol) == -5
    assert (c.res == -7).all() and b"no HIP device" in L.nq_last_error(None)


def test_the_python_module_is_exported(nq):
    for name in ("Quality", "choose_colors", "compare_frames", "compare_frames_device", "compare_indexed", "compare_indexed_device"):
        assert hasattr(nq, name) and name in nq.__all__
    total = nq.Quality.total([nq.Quality(compare_ref.compare(_full(16, 16, BLACK), _full(16, 16, WHITE))),
                              nq.Quality(compare_ref.compare(_checker(16, 16), _checker(16, 16, WHITE, BLACK)))])
    assert total.slots[:13].tolist() == [512, 8, 0, 33292800, 33292800, 33292800, 255, 0, 17179344900, 17179344900, 17179344900, -130592, 65419]
    assert total.max_diff == 255 and abs(total.ssim - (-130592 / (32768.0 * 8))) < 1e-12 and abs(total.worst_block - (1 - 65419 / 32768.0)) < 1e-12
    same = nq.Quality(compare_ref.compare(_full(8, 8, WHITE), _full(8, 8, WHITE)))
    assert same.psnr == float("inf") and same.lf_psnr == float("inf") and same.ssim == 1.0 and same.worst_block == 1.0
    assert abs(total.psnr - 10 * np.log10(65025 * 3 * 512 / (3 * 33292800))) < 1e-9


# ---- the constants tests/test_gpu_compare.py counts with ----
def constants():
    """(frames per launch, grid cap in workgroups, strip width in columns, waves per workgroup) as the sources spell them."""
    csrc = os.path.join(HERE, "..", "nquant.android_amd", "csrc")
    hip = open(os.path.join(csrc, "nq_compare.hip")).read()
    hdr = open(os.path.join(csrc, "nq_kernels.h")).read()
    get = lambda text, pat: int(re.search(pat, text, re.M).group(1))
    threads = get(hip, r"^constexpr int CMP_THREADS = (\d+);$")
    assert re.search(r"^constexpr int CMP_WAVES = CMP_THREADS / 64;$", hip, re.M)
    return (get(hdr, r"^constexpr int COMPARE_FRAMES_PER_LAUNCH = (\d+);$"), get(hip, r"^constexpr int CMP_GRID_CAP = (\d+);"),
            get(hip, r"^constexpr int CMP_STRIP_WIDTH = (\d+);"), threads // 64)


def test_the_constants_the_gpu_test_counts_with():
    """tests/test_gpu_compare.py picks its frame counts around the frames of a launch, its widths around a wave's strip, and sizes the
    frame that reaches the strip loop from the grid cap.  Changing one of them must fail here, not silently move those paths out of the
    test's reach."""
    assert constants() == (16, 512, 256, 4)
