"""CPU-side checks of the frame reduction (include/nquant_abi.h "frame reduction"): the committed linear-light table, properties of the
restatement in resample_ref.py that the GPU tests compare against (exact copy at equal size, no overflow at 2048 x 2048 -> 1 x 1, within
one level of Pillow's box filter in stored values and of the float64 formula in linear light, no colour from transparent pixels),
fit_size, and the interface: both symbols in the built library and the Python entry points."""
import inspect

import numpy as np
import pytest

import resample_ref as R


def _srgb_decode(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def _srgb_encode(l):
    l = np.asarray(l, np.float64)
    return np.where(l <= 0.0031308, l * 12.92, 1.055 * np.maximum(l, 0.0) ** (1 / 2.4) - 0.055)


def _opaque(rgb):
    rgb = np.asarray(rgb).astype(np.uint32)
    return (np.uint32(0xFF000000) | rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]).astype(np.uint32).view(np.int32)


def _channels(argb):
    u = np.asarray(argb).view(np.uint32)
    return np.stack([(u >> 16) & 255, (u >> 8) & 255, u & 255], -1).astype(np.int64)


def _images(w, h, seed):
    """Noise, four colours in blocks, and a gradient: opaque (h, w, 3) uint8 arrays."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)
    four = colours[(np.arange(h)[:, None] * 2 // h) * 2 + (np.arange(w)[None, :] * 2 // w)]
    ramp = np.stack([np.broadcast_to(np.arange(w)[None, :] * 255 // max(w - 1, 1), (h, w)),
                     np.broadcast_to(np.arange(h)[:, None] * 255 // max(h - 1, 1), (h, w)),
                     np.full((h, w), 128)], -1).astype(np.uint8)
    return {"noise": noise, "four": four, "gradient": ramp}


def test_table_file_is_the_rounded_srgb_decoding():
    T = R.linear_table()
    assert T.shape == (256,) and (np.diff(T.astype(np.int64)) > 0).all()
    assert T[:4].tolist() == [0, 20, 40, 60] and int(T[254]) == 64952 and int(T[255]) == 65535
    exact = 65535.0 * _srgb_decode(np.arange(256) / 255.0)
    assert np.abs(T.astype(np.float64) - exact).max() <= 1.0
    assert R.table(0).tolist() == [257 * v for v in range(256)]


@pytest.mark.parametrize("flags", [0, R.LINEAR])
def test_equal_size_copies_the_crop_and_clears_transparent_pixels(flags):
    f = R.random_argb(13, 9, 4)
    u = f.view(np.uint32)
    assert (u >> 24 == 0).any() and (u >> 24 == 255).any() and ((u >> 24 > 0) & (u >> 24 < 255)).any()
    want = np.where(u >> 24 == 0, np.uint32(0), u).view(np.int32)
    assert (R.resample([f], flags=flags)[0] == want).all()
    got = R.resample([f], crop=(3, 2, 7, 5), flags=flags)[0]
    assert got.shape == (5, 7) and (got == want[2:7, 3:10]).all()


@pytest.mark.parametrize("flags", [0, R.LINEAR])
def test_white_2048_square_does_not_overflow(flags):
    """S_c = 2048^2 * 65535 * 255 is just below 2^46 and the numerator 2 S_c + S_a of the division passes it: far beyond float64's
    53 bits of exact products, and beyond any 32-bit intermediate."""
    f = np.full((2048, 2048), -1, np.int32)
    assert 2 * 2048 * 2048 * 65535 * 255 > 2**46
    assert R.resample([f], size=(1, 1), flags=flags)[0].view(np.uint32).tolist() == [[0xFFFFFFFF]]
    assert R.resample([f], size=(2, 1), flags=flags)[0].view(np.uint32).tolist() == [[0xFFFFFFFF, 0xFFFFFFFF]]


INTEGER_RATIOS = [((8, 8), (4, 4)), ((12, 6), (4, 2)), ((30, 20), (10, 5)), ((64, 64), (8, 8)), ((21, 14), (3, 2)), ((40, 24), (8, 8))]
FRACTIONAL = [((13, 9), (5, 4)), ((64, 48), (17, 11)), ((100, 60), (33, 7))]


@pytest.mark.parametrize("src,dst", INTEGER_RATIOS, ids=lambda s: "%dx%d" % s)
def test_stored_value_mode_is_within_one_level_of_pillow_box(src, dst):
    """Integer ratios only: Pillow's BOX samples whole pixels at fractional ratios.  The margin is the two roundings involved."""
    from PIL import Image
    (w, h), (dw, dh) = src, dst
    worst = 0
    for name, rgb in _images(w, h, 7 * w + h).items():
        got = _channels(R.resample([_opaque(rgb)], size=dst, flags=0)[0])
        assert (R.resample([_opaque(rgb)], size=dst, flags=0)[0].view(np.uint32) >> 24 == 255).all()
        im = Image.fromarray(rgb, "RGB")
        box = np.asarray(im.resize((dw, dh), Image.BOX)).astype(np.int64)
        worst = max(worst, int(np.abs(got - box).max()))
        red = np.asarray(im.reduce((w // dw, h // dh))).astype(np.int64)
        assert red.shape == (dh, dw, 3)
        worst = max(worst, int(np.abs(got - red).max()))
    print("max |restatement - Pillow| at %s -> %s: %d" % (src, dst, worst))
    assert worst <= 1


@pytest.mark.parametrize("src,dst", INTEGER_RATIOS + FRACTIONAL, ids=lambda s: "%dx%d" % s)
def test_linear_mode_is_within_one_level_of_the_float_formula(src, dst):
    """decode, weighted mean, encode, round -- in float64.  The margin is the two roundings involved (the table's and the result's)."""
    (w, h), (dw, dh) = src, dst
    Wy = R.weights(h, dh).astype(np.float64) / h
    Wx = R.weights(w, dw).astype(np.float64) / w
    worst = 0
    for name, rgb in _images(w, h, 11 * w + h).items():
        got = _channels(R.resample([_opaque(rgb)], size=dst, flags=R.LINEAR)[0])
        lin = _srgb_decode(rgb / 255.0)
        mean = np.einsum("yi,ijc,xj->yxc", Wy, lin, Wx)
        want = np.floor(255.0 * _srgb_encode(mean) + 0.5).astype(np.int64)
        worst = max(worst, int(np.abs(got - want).max()))
    print("max |restatement - float64 formula| at %s -> %s: %d" % (src, dst, worst))
    assert worst <= 1


@pytest.mark.parametrize("flags", [0, R.LINEAR])
def test_transparent_pixels_do_not_bleed_colour(flags):
    """A semi-transparent red pixel next to a fully transparent green one: red at half the alpha, no green."""
    f = np.array([[0x80FF0000, 0x0000FF00]], np.uint32).view(np.int32)
    got = int(R.resample([f], size=(1, 1), flags=flags)[0].view(np.uint32)[0, 0])
    assert got == 0x40FF0000
    f = np.array([[0x00123456, 0x00FFFFFF]], np.uint32).view(np.int32)
    assert int(R.resample([f], size=(1, 1), flags=flags)[0][0, 0]) == 0


def test_weights_of_one_output_sum_to_the_source_side_and_match_the_footprint():
    for src, dst in ((13, 5), (9, 4), (8, 4), (7, 7), (4099, 1), (67, 3)):
        Wm = R.weights(src, dst)
        assert (Wm.sum(1) == src).all() and (Wm.sum(0) == dst).all()
        for x in range(dst):
            j0, j1 = R.footprint(x, src, dst)
            nzj = np.nonzero(Wm[x])[0]
            assert nzj[0] == j0 and nzj[-1] == j1 and len(nzj) == j1 - j0 + 1


def test_fit_size(nq):
    cases = [((3840, 2160, 960, 960), (960, 540)), ((3840, 2160, 960, 100), (178, 100)), ((100, 50, 200, 200), (100, 50)),
             ((100, 50, 200, 25), (50, 25)), ((4096, 4096, 1024, 2048), (1024, 1024)), ((1000, 1, 10, 10), (10, 1)),
             ((1, 1000, 10, 10), (1, 10)), ((3, 2, 2, 2), (2, 1)), ((1920, 1080, 1920, 1080), (1920, 1080)), ((7, 5, 5, 5), (5, 4)),
             ((5, 7, 5, 5), (4, 5)), ((1, 1, 1, 1), (1, 1))]
    for args, want in cases:
        got = nq.fit_size(*args)
        assert got == want, (args, got, want)
        assert 1 <= got[0] <= min(args[0], args[2]) and 1 <= got[1] <= min(args[1], args[3])
    for bad in ((0, 5, 5, 5), (5, 5, 0, 5), (5, -1, 5, 5)):
        with pytest.raises(ValueError):
            nq.fit_size(*bad)


def test_resample_symbols_and_wrappers_are_exported(nq):
    import os
    import re
    from conftest import ROOT
    L = nq.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nquant_abi.h")).read(), flags=re.S)
    for name in ("nq_resample_frames_device", "nq_resample_frames"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"#define\s+NQ_RESAMPLE_LINEAR\s+1\b", header)
    for name in ("resample_frames", "resample_frames_device", "fit_size"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    for fn in (nq.convert_frames_to_gif, nq.convert_shots_to_gif, nq.convert_clip_to_gif, nq.convert_frames_to_apng, nq.convert_frames_refined):
        p = inspect.signature(fn).parameters
        assert p["size"].default is None and p["crop"].default is None and p["linear_resample"].default is True, fn.__name__


def test_null_handle_and_python_argument_checks_need_no_device(nq):
    L = nq.load_library()
    assert L.nq_resample_frames(None, 1, None, 4, 4, 0, 0, 4, 4, None, 2, 2, 1) == -1
    assert L.nq_resample_frames_device(None, 1, None, 4, 4, 0, 0, 4, 4, None, 2, 2, 1) == -1
    with pytest.raises(ValueError):
        nq.resample_frames_device(None, [], 4, 4, [], (2, 2))
