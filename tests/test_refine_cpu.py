"""The palette refinement's definition (include/nquant_abi.h "palette refinement") as restated in refine_ref.py, without a GPU:
hand-computed answers, the properties the GPU tests rely on, and the gain on the sample picture with the stored fixture palettes.  The
last test holds the library to the header as far as that goes without a device: the entry points exist and refuse a NULL handle."""
import ctypes as C
import os

import numpy as np
import pytest

import refine_ref
from nquant.android_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _u32(*v):
    return np.array(v, np.uint32)


def test_two_pixels_one_entry():
    """Pixels (10, 20, 30) and (20, 40, 61), entry (0, 0, 0): d = 1400 + 5721; the mean is (15, 30, 45.5 -> 46); then the pixels
    are (5, 10, 16) and (5, 10, 15) away from it."""
    frame = _u32(0xFF0A141E, 0xFF14283D).reshape(1, 2)
    pal, sse, cnt, passes = refine_ref.refine([frame], _u32(0xFF000000), 2)
    assert sse[0] == (100 + 400 + 900) + (400 + 1600 + 3721)
    assert pal.tolist() == [0xFF0F1E2E]
    assert sse[1] == (25 + 100 + 256) + (25 + 100 + 225) and sse[2] == sse[1]
    assert cnt.tolist() == [2] and passes == 2


def test_a_pixel_between_two_entries_takes_the_lower_index():
    frame = _u32(0xFF000064).reshape(1, 1)                      # b = 100, entries at b = 90 and b = 110, both ways round
    for palette in (_u32(0xFF00005A, 0xFF00006E), _u32(0xFF00006E, 0xFF00005A)):
        pal, sse, cnt, passes = refine_ref.refine([frame], palette, 1)
        assert cnt.tolist() == [1, 0] and sse.tolist() == [100, 0]
        assert pal.tolist() == [0xFF000064, int(palette[1])]


def test_half_rounds_up():
    frame = _u32(0xFF010101, 0xFF020202).reshape(2, 1)          # 1 + 2 over 2 pixels is 2
    pal, sse, cnt, passes = refine_ref.refine([frame], _u32(0xFF808080), 1)
    assert pal.tolist() == [0xFF020202] and sse[1] == 3 and cnt.tolist() == [2]


@pytest.mark.parametrize("K", [1, 2, 16, 256])
def test_sse_never_rises(K):
    img = synth.gradient_noise(96, 80, 3)
    rng = np.random.default_rng(K)
    palette = (rng.integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000))
    pal, sse, cnt, passes = refine_ref.refine([img], palette, 6)
    assert (np.diff(sse) <= 0).all() and sse[6] < sse[0], sse.tolist()
    assert cnt.sum() == img.size and 1 <= passes <= 7


def test_alpha_of_the_palette_never_changes():
    img = synth.with_alpha(synth.gradient_noise(96, 80, 4), 4)
    rng = np.random.default_rng(5)
    palette = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32) | np.uint32(0x01000000)
    pal, sse, cnt, passes = refine_ref.refine([img], palette, 4)
    assert ((pal >> 24) == (palette >> 24)).all() and (pal != palette).any()
    assert cnt.sum() == int(((img.view(np.uint32) >> 24) != 0).sum())


def test_a_pinned_entry_is_untouched_and_empty():
    img = synth.gradient_noise(96, 80, 6)
    palette = _u32(0xFF202020, 0x00808080, 0xFFC0C0C0)          # the pinned entry is nearer to most pixels than its neighbours
    pal, sse, cnt, passes = refine_ref.refine([img], palette, 3)
    assert pal[1] == 0x00808080 and cnt[1] == 0 and cnt.sum() == img.size
    assert pal[0] != palette[0] and pal[2] != palette[2]


def test_a_fixed_point_stops_after_one_pass():
    img = synth.few_colors(40, 30, 7, 5)
    palette = np.unique(img.view(np.uint32))
    pal, sse, cnt, passes = refine_ref.refine([img], palette, 9)
    assert passes == 1 and (pal == palette).all() and (sse == 0).all() and sse.size == 10


def test_no_live_entry_and_no_counted_pixel():
    img = synth.gradient_noise(16, 8, 8)
    pal, sse, cnt, passes = refine_ref.refine([img], _u32(0x00123456, 0x00FFFFFF), 3)
    assert pal.tolist() == [0x00123456, 0x00FFFFFF] and (sse == 0).all() and (cnt == 0).all() and passes == 1
    clear = (img.view(np.uint32) & np.uint32(0x00FFFFFF))
    pal, sse, cnt, passes = refine_ref.refine([clear], _u32(0xFF123456), 3)
    assert pal.tolist() == [0xFF123456] and (sse == 0).all() and (cnt == 0).all() and passes == 1


@pytest.mark.parametrize("iterations", [0, 1, 4])
def test_weighted_frames_equal_the_expanded_sequence(iterations):
    """refine_weighted(pool, weights) is refine() of the sequence that repeats every frame of the pool that often, in all four outputs:
    what lets test_gpu_refine.py state the result of a call with 140 000 frames from five assignment passes."""
    pool = [synth.gradient_noise(33, 31, 21), synth.with_alpha(synth.gradient_noise(9, 7, 22), 22), np.full((4, 4), 0xFF3060C0, np.uint32)]
    weights = (5, 3, 1)
    rng = np.random.default_rng(23)
    order = rng.permutation(np.repeat(np.arange(3), weights))
    for K in (2, 16):
        palette = rng.integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000)
        want = refine_ref.refine([pool[i] for i in order], palette, iterations)
        got = refine_ref.refine_weighted(pool, weights, palette, iterations)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
        assert got[3] == want[3]
        assert iterations == 0 or got[3] > 1


def test_the_constants_the_flush_test_counts_with():
    """tests/test_gpu_refine.py reaches the flush inside the round loop of the shipped kernel by the number of frames alone, and works
    that number out from these two values.  Changing either must fail here, not silently move the flush out of the test's reach."""
    import re
    src = open(os.path.join(HERE, "..", "nquant.android_amd", "csrc", "nq_refine.hip")).read()
    assert re.search(r"^#define NQ_REFINE_FLUSH_PIXELS \(1 << 24\)$", src, re.M)
    assert re.search(r"^constexpr unsigned REF_FLUSH_PIXELS = NQ_REFINE_FLUSH_PIXELS;", src, re.M)
    assert re.search(r"^constexpr int REF_THREADS = 256;$", src, re.M)


# sse[0] and the ratios sse[j] / sse[0], j = 1, 4, 8, of the stored palettes on the sample picture, computed with this restatement.
# The 256-entry palettes hold alpha-254 entries (23 and 89 of them) and the picture is opaque: their pixels keep a distance of 1 in
# alpha through every pass, because the alpha of an entry never changes.  (Moving alpha to the mean as well would give 0.923 / 0.889 /
# 0.876 and 0.863 / 0.762 / 0.722 -- and turn an opaque palette's 254 into 255, which is what the definition rules out.)
SAMPLE = {"sample_rgb256_dither": (4522087, 0.931, 0.894, 0.881),
          "sample_lab256_dither": (6495541, 0.877, 0.775, 0.733),
          "sample_lab16_dither": (84105248, 0.869, 0.815, 0.810)}


@pytest.mark.parametrize("name", sorted(SAMPLE))
def test_passes_lower_the_error_of_the_stored_palettes_on_the_sample_picture(name):
    rgb = np.load(os.path.join(HERE, "golden", "sample_495x438.npz"))["rgb"]
    img = synth.tile_photo(rgb, rgb.shape[1], rgb.shape[0])
    palette = np.load(os.path.join(HERE, "golden", name + ".npz"))["palette"]
    pal, sse, cnt, passes = refine_ref.refine([img], palette, 8)
    sse0, r1, r4, r8 = SAMPLE[name]
    assert sse[8] < sse[0] and (np.diff(sse) <= 0).all()
    assert sse[0] == sse0
    assert [round(float(sse[j]) / float(sse[0]), 3) for j in (1, 4, 8)] == [r1, r4, r8]
    assert ((pal >> 24) == (palette.view(np.uint32) >> 24)).all()


def test_the_library_exports_the_calls_and_refuses_a_null_handle(nq):
    """No device is needed to be refused: a NULL handle is NQ_ERR_INVALID and leaves every output alone."""
    L = nq.load_library()
    frame = np.zeros(8, np.uint32)
    src = (C.c_void_p * 1)(frame.ctypes.data)
    w, hgt = np.array([2], np.int32), np.array([3], np.int32)
    for entry in ("nq_refine_palette", "nq_refine_palette_device"):
        pal, sse, cnt, passes = np.full(4, 0xFF112233, np.uint32), np.full(4, -7, np.int64), np.full(4, -7, np.int64), C.c_int32(-7)
        assert getattr(L, entry)(None, 1, src, w.ctypes.data, hgt.ctypes.data, pal.ctypes.data, 2, 1, sse.ctypes.data, cnt.ctypes.data,
                                 C.byref(passes)) == -1
        assert (pal == 0xFF112233).all() and (sse == -7).all() and (cnt == -7).all() and passes.value == -7
    for entry in ("nq_convert_frames_refined", "nq_convert_frames_refined_device"):
        out, K = np.full(8, -7, np.int32), C.c_int32(-7)
        dst = (C.c_void_p * 1)(out.ctypes.data)
        seeds = np.zeros(1, np.int64)
        assert getattr(L, entry)(None, 1, src, w.ctypes.data, hgt.ctypes.data, 16, 2, 1, seeds.ctypes.data, 1, dst, None, pal.ctypes.data,
                                 C.byref(K)) == -1
        assert (out == -7).all() and K.value == -7
    assert callable(nq.refine_palette) and callable(nq.palette_error) and callable(nq.convert_frames_refined) and callable(nq.refine_palette_device)
