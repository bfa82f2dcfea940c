"""The ordered dither's definition (include/nquant_abi.h "ordered dither") as restated in ordered_ref.py, without a GPU: hand-computed
answers, the mask property they rest on, the properties the GPU tests rely on, and the error on the sample picture with the stored
fixture palettes against the stored error-diffusion output.  The last test holds the library to the header as far as that goes
without a device: the entry points exist and refuse a NULL handle."""
import ctypes as C
import os

import numpy as np
import pytest

import ordered_ref as R
import refine_ref
from nquant.android_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _u32(*v):
    return np.array(v, np.uint32)


def test_the_mask_holds_every_value_16_times():
    """The share of positions at which a pixel takes i2 is exact only because of this; the 1232 below rests on it."""
    assert R.MASK.shape == (64, 64)
    assert np.bincount((R.MASK + 128).reshape(-1), minlength=256).tolist() == [16] * 256


def test_a_flat_frame_between_two_entries():
    """Entries b = 0 and b = 100, every pixel b = 30: den = 10 000, d1 = 900, d2 = 4900, D = 4000.  (255 - 2 m) * 10 000 > 1 024 000 is
    255 - 2 m > 102.4, m <= 76: 77 mask values, 16 positions each, 1232 of the 4096 pixels (t = 0.3: 1228.8)."""
    frame = np.full((64, 64), 0xFF00001E, np.uint32)
    low = (R.MASK + 128) <= 76
    assert int(low.sum()) == 1232
    for limit in (100, 255):
        idx, out, stats = R.dither([frame], _u32(0xFF000000, 0xFF000064), limit)
        assert ((idx[0] == 1) == low).all()
        assert (out[0] == np.where(low, 0xFF000064, 0xFF000000)).all()
        assert stats.tolist() == [[1232, 1232 * 4900 + 2864 * 900]]
    idx, out, stats = R.dither([frame], _u32(0xFF000000, 0xFF000064), 99)       # the entries are 100 apart
    assert (idx[0] == 0).all() and stats.tolist() == [[0, 4096 * 900]]
    idx, out, stats = R.dither([frame], _u32(0xFF000064, 0xFF000000), 100)      # the entries swapped: the mirrored indices
    assert ((idx[0] == 0) == low).all() and stats.tolist() == [[1232, 1232 * 4900 + 2864 * 900]]


def _pinned_palette(K, seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000)
    pal[K // 2] &= np.uint32(0x00FFFFFF)                        # a pinned entry
    return pal


@pytest.mark.parametrize("alpha", [False, True])
def test_limit_0_is_the_assignment_of_the_refinement(alpha):
    img = synth.gradient_noise(96, 80, 3)
    if alpha:
        img = synth.with_alpha(img, 4)
    for K in (2, 16, 256):
        pal = _pinned_palette(K, K)
        idx, out, stats = R.dither([img], pal, 0)
        _, sse, cnt, _ = refine_ref.refine([img], pal, 0)
        counted = (img.view(np.uint32) >> 24) != 0
        assert np.bincount(idx[0][counted], minlength=K).tolist() == cnt.tolist()
        assert stats.tolist() == [[0, int(sse[0])]]
        assert (idx[0][~counted] == K // 2).all()               # T: the pinned entry
        assert alpha == bool((~counted).any())


@pytest.mark.parametrize("limit", [1, 40, 255])
def test_every_pixel_shows_i1_or_an_entry_within_the_limit_of_it(limit):
    img = synth.with_alpha(synth.gradient_noise(96, 80, 5), 6)
    for K in (3, 64):
        pal = _pinned_palette(K, 10 + K)
        i1 = R.dither([img], pal, 0)[0][0].astype(np.int64)
        idx, out, stats = R.dither([img], pal, limit)
        got = idx[0].astype(np.int64)
        ch = R._channels(pal)
        far = np.abs(ch[got.reshape(-1)] - ch[i1.reshape(-1)]).max(axis=1)
        assert (far <= limit).all()
        assert ((got != i1).sum() == stats[0, 0]) and (out[0] == pal[got]).all()
        if limit == 255:
            assert stats[0, 0] > 0


def test_an_equidistant_pixel_has_i1_the_lower_index():
    frame = np.full((64, 64), 0xFF000064, np.uint32)            # b = 100, entries at b = 90 and b = 110, both ways round
    for palette in (_u32(0xFF00005A, 0xFF00006E), _u32(0xFF00006E, 0xFF00005A)):
        idx, _, stats = R.dither([frame], palette, 0)
        assert (idx[0] == 0).all() and stats.tolist() == [[0, 4096 * 100]]
        idx, _, stats = R.dither([frame], palette, 255)         # D = 0: i2 wherever 255 - 2 m > 0, half of the positions
        assert ((idx[0] == 1) == ((R.MASK + 128) <= 127)).all() and stats.tolist() == [[2048, 4096 * 100]]


def test_duplicates_are_never_mixed():
    img = synth.gradient_noise(96, 80, 7)
    pal = _u32(0xFF202020, 0xFF202020, 0xFFC0C0C0, 0xFFC0C0C0, 0xFF808080)
    idx, _, stats = R.dither([img], pal, 255)
    assert not np.isin(idx[0], (1, 3)).any()                   # i2 of a pixel nearest to entry 0 is its duplicate, den = 0
    near = R.dither([img], pal, 0)[0][0]
    assert ((idx[0] != near) <= (near == 4)).all()             # only the single entry mixes, with whichever duplicate pair is second


def test_transparent_pixels_take_T_and_are_not_counted():
    img = synth.with_alpha(synth.gradient_noise(40, 30, 8), 9, p_transparent=0.2)
    clear = (img.view(np.uint32) >> 24) == 0
    assert clear.any() and not clear.all()
    pal = _u32(0xFF102030, 0xFFE0D0C0, 0x00FFFFFF, 0xFF808080, 0x00000000)
    idx, out, stats = R.dither([img], pal, 255)
    assert (idx[0][clear] == 2).all() and (out[0][clear] == 0x00FFFFFF).all() and not np.isin(idx[0][~clear], (2, 4)).any()
    kept = img.view(np.uint32).copy()
    kept[clear] = 0x00FFFFFF                                    # at distance 0 from entry 2 in r, g, b: it would add nothing either way
    kept[clear] ^= 0x00123456
    assert R.dither([kept], pal, 255)[2].tolist() == stats.tolist()
    # without an a = 0 entry the same pixels are counted and take a live entry
    idx2, _, stats2 = R.dither([img], pal[[0, 1, 3]], 255)
    assert stats2[0, 1] > stats[0, 1] and (idx2[0] < 3).all()


def test_no_live_entry_gives_index_0_everywhere():
    img = synth.with_alpha(synth.gradient_noise(16, 8, 8), 3, p_transparent=0.3)
    idx, out, stats = R.dither([img], _u32(0x00123456, 0x00FFFFFF), 255)
    assert (idx[0] == 0).all() and (out[0] == 0x00123456).all() and stats[0, 0] == 0
    ch = R._channels(img)
    counted = ch[:, 0] != 0
    assert stats[0, 1] == int(((ch[counted] - np.array([0, 0x12, 0x34, 0x56])) ** 2).sum())


def test_frames_that_differ_in_a_rectangle_give_maps_that_differ_only_there():
    a = synth.gradient_noise(96, 80, 11)
    b = a.copy()
    b[17:40, 50:83] = synth.gradient_noise(33, 23, 12)
    pal = _pinned_palette(32, 13) | np.uint32(0xFF000000)
    idx, _, _ = R.dither([a, b], pal, 64)
    diff = idx[0] != idx[1]
    assert diff.any() and not diff[:17].any() and not diff[40:].any() and not diff[:, :50].any() and not diff[:, 83:].any()


def test_a_frame_shifted_by_the_mask_period_gives_the_shifted_map():
    small = synth.gradient_noise(70, 50, 14)
    big = synth.gradient_noise(70 + 64 + 9, 50 + 64 + 5, 15)
    big[64:64 + 50, 64:64 + 70] = small
    pal = _pinned_palette(24, 16) | np.uint32(0xFF000000)
    idx, _, _ = R.dither([small, big], pal, 255)
    assert (idx[1][64:64 + 50, 64:64 + 70] == idx[0]).all()
    big2 = synth.gradient_noise(70 + 64 + 9, 50 + 64 + 5, 15)
    big2[63:63 + 50, 64:64 + 70] = small                       # one row off the period: another part of the mask
    assert (R.dither([big2], pal, 255)[0][0][63:63 + 50, 64:64 + 70] != idx[0]).any()


# {pixels that took i2, squared error} of the stored palettes on the top-left 256 x 256 of the sample picture at limit 255, computed
# with this restatement: 8.0 % and 23.0 % of the pixels are mixed.
SAMPLE = {"sample_lab16_dither": (5244, 28569980), "sample_lab256_dither": (15074, 2386199)}


@pytest.mark.parametrize("name", sorted(SAMPLE))
def test_the_error_on_the_sample_picture_is_below_the_stored_diffusion_output(name):
    rgb = np.load(os.path.join(HERE, "golden", "sample_495x438.npz"))["rgb"]
    img = np.ascontiguousarray(synth.tile_photo(rgb, rgb.shape[1], rgb.shape[0])[:256, :256])
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    palette = z["palette"]
    idx, out, stats = R.dither([img], palette, 255)
    stored = z["tiled_index"][:256, :256].astype(np.int64)
    stored_err = int(((R._channels(img) - R._channels(palette)[stored.reshape(-1)]) ** 2).sum())
    print("%s: %d pixels mixed, error %d against %d of the stored tiled_index output" % (name, stats[0, 0], stats[0, 1], stored_err))
    assert stats[0, 1] < stored_err
    assert tuple(stats[0].tolist()) == SAMPLE[name]


def test_the_library_exports_the_calls_and_refuses_a_null_handle(nq):
    """No device is needed to be refused: a NULL handle is NQ_ERR_INVALID and leaves every output alone."""
    L = nq.load_library()
    frame = np.zeros(8, np.uint32)
    src = (C.c_void_p * 1)(frame.ctypes.data)
    w, hgt = np.array([2], np.int32), np.array([3], np.int32)
    header = open(os.path.join(HERE, "..", "include", "nquant_abi.h")).read()
    for entry in ("nq_dither_ordered", "nq_dither_ordered_device", "nq_convert_frames_ordered", "nq_convert_frames_ordered_device"):
        assert entry in nq.abi_symbols() and hasattr(L, entry) and ("int %s(" % entry) in header, entry
    pal = np.full(4, 0xFF112233, np.uint32)
    for entry in ("nq_dither_ordered", "nq_dither_ordered_device"):
        out, index, stats = np.full(8, -7, np.int32), np.full(8, 77, np.uint16), np.full(2, -7, np.int64)
        dst, idx = (C.c_void_p * 1)(out.ctypes.data), (C.c_void_p * 1)(index.ctypes.data)
        assert getattr(L, entry)(None, 1, src, w.ctypes.data, hgt.ctypes.data, pal.ctypes.data, 2, 16, dst, idx, stats.ctypes.data) == -1
        assert (out == -7).all() and (index == 77).all() and (stats == -7).all() and (pal == 0xFF112233).all()
    for entry in ("nq_convert_frames_ordered", "nq_convert_frames_ordered_device"):
        out, index, K = np.full(8, -7, np.int32), np.full(8, 77, np.uint16), C.c_int32(-7)
        dst, idx = (C.c_void_p * 1)(out.ctypes.data), (C.c_void_p * 1)(index.ctypes.data)
        assert getattr(L, entry)(None, 1, src, w.ctypes.data, hgt.ctypes.data, 16, 2, 16, dst, idx, pal.ctypes.data, C.byref(K)) == -1
        assert (out == -7).all() and (index == 77).all() and K.value == -7 and (pal == 0xFF112233).all()
    assert callable(nq.dither_ordered) and callable(nq.dither_ordered_device) and callable(nq.convert_frames_ordered)
    import inspect
    for fn in (nq.convert_frames_to_gif, nq.convert_shots_to_gif, nq.convert_clip_to_gif, nq.convert_frames_to_apng):
        assert inspect.signature(fn).parameters["ordered"].default is None
    frames = [np.zeros((4, 4), np.int32)] * 2
    with pytest.raises(TypeError):
        nq.convert_frames_to_gif(1, frames, 16, True, ordered=True)
    with pytest.raises(ValueError):
        nq.convert_frames_to_gif(1, frames, 16, True, ordered=32, seeds=[0, 0])
    with pytest.raises(ValueError):
        nq.convert_frames_to_apng(1, frames, 16, True, ordered=256)
