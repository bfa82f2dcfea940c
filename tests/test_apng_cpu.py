"""CPU-side checks of the APNG encoder (include/nquant_abi.h "APNG encoding"): the restatement in apng_ref.py gives files that compose
back to the RGBA frames, through its own composer and through Pillow (so the bytes the GPU tests compare against are right), in mark
mode and in crop mode; the mode rule; one frame gives png_ref's bytes; nq_apng_max_bytes bounds a sequence that changes everywhere;
the size claim of the delta encoding on the restatement; the symbols and wrappers exist; without a HIP device the calls refuse to
compute (no CPU fallback)."""
import numpy as np
import pytest

import apng_ref
import png_ref
from conftest import HAS_GPU
from gif_delta_cases import KS, palette_of, sequence
from gif_delta_ref import rectangles

PIL = pytest.importorskip("PIL")


def alpha_palette(K, rng):
    """An opaque palette with one alpha-0 and (K >= 2) one alpha-0x80 entry."""
    pal = palette_of(K, rng)
    pal[K // 2] &= 0x00FFFFFF
    if K >= 2:
        pal[(K // 2 + 1) % K] = (pal[(K // 2 + 1) % K] & 0x00FFFFFF) | 0x80000000
    return pal


def composes_back(data, frames, pal, why):
    own, got = apng_ref.compose(data), apng_ref.pillow_canvases(data)
    assert len(own) == len(got) == len(frames), why
    for i, (c, g, f) in enumerate(zip(own, got, frames)):
        want = apng_ref.rgba_of(f, pal)
        assert (c == want).all(), (why, i, "own composer")
        assert (g == want).all(), (why, i, "Pillow")


@pytest.mark.parametrize("kind", ["opaque", "alpha"])
@pytest.mark.parametrize("K", KS)
def test_restatement_composes_back_to_the_frames(K, kind):
    rng = np.random.default_rng(300 + K)
    pal = palette_of(K, rng) if kind == "opaque" else alpha_palette(K, rng)
    mark = kind == "opaque" and K <= 255
    for h, w in ((1, 1), (1, 77), (37, 91)):
        frames = sequence(h, w, K, rng)
        delays = list(range(len(frames)))
        for S in (0, 7):
            data = apng_ref.encode(frames, pal, delays_cs=delays, loop=3, segment_bytes=S)
            head, parsed = apng_ref.parse(data)
            Kt = K + mark
            assert (head["width"], head["height"], head["num_frames"], head["num_plays"]) == (w, h, len(frames), 3)
            assert head["depth"] == png_ref.bit_depth(Kt) and len(head["palette"]) == Kt
            assert [(p["x"], p["y"], p["w"], p["h"]) for p in parsed] == rectangles(frames)
            assert [p["blend"] for p in parsed] == [0] + [int(mark)] * (len(frames) - 1)
            assert all(p["dispose"] == 0 and p["delay_num"] == i and p["delay_den"] == 100 for i, p in enumerate(parsed))
            if mark:
                assert head["palette"][K] == 0 and all(c >> 24 == 255 for c in head["palette"][:K])
            # a frame's payload is the IDAT payload of the still image that is its body
            chunks = [c for c in png_ref.parse(data) if c[0] in (b"IDAT", b"fdAT")]
            for (kind_, payload), body in zip(chunks, apng_ref.bodies(frames, pal)):
                still = dict(png_ref.parse(png_ref.encode(body, apng_ref.palette_t(pal), S)))[b"IDAT"]
                assert (payload if kind_ == b"IDAT" else payload[4:]) == still
            composes_back(data, frames, pal, (K, kind, h, w, S))
            assert len(data) <= apng_ref.max_bytes(len(frames), w, h, S)


def test_mode_rule():
    opaque = lambda K: 0xFF000000 | np.arange(K, dtype=np.int64)
    assert apng_ref.unchanged_index(opaque(255)) == 255 and apng_ref.unchanged_index(opaque(1)) == 1
    assert apng_ref.unchanged_index(opaque(256)) is None
    for a in (0, 0x80, 0xFE):
        pal = opaque(17)
        pal[5] = (pal[5] & 0x00FFFFFF) | a << 24
        assert apng_ref.unchanged_index(pal) is None, a
    a = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    b = a.copy()
    b[0, 0], b[1, 1] = 8, 8
    assert (apng_ref.bodies([a, b], opaque(9))[1] == [[8, 9], [9, 8]]).all()                 # mark: unchanged pixels are u = 9
    clear = opaque(9)
    clear[0] &= 0x00FFFFFF
    assert (apng_ref.bodies([a, b], clear)[1] == [[8, 1], [3, 8]]).all()                     # crop
    # the mark-mode depth grows at K = 2, 4, 16
    for K, depth in ((2, 2), (4, 4), (16, 8), (3, 2), (15, 4), (17, 8)):
        data = apng_ref.encode([np.zeros((2, 2), int), np.ones((2, 2), int)], opaque(K))
        assert apng_ref.parse(data)[0]["depth"] == depth, K


@pytest.mark.parametrize("K", KS)
def test_one_frame_is_the_still_image_file(K):
    rng = np.random.default_rng(K)
    idx = rng.integers(0, K, (13, 29))
    for pal in (palette_of(K, rng), alpha_palette(K, rng)):
        for S in (0, 5):
            data = apng_ref.encode([idx], pal, segment_bytes=S)
            assert data == png_ref.encode(idx, pal, S) and b"acTL" not in data and b"fcTL" not in data


def test_max_bytes_bounds_a_sequence_that_changes_everywhere(nq):
    assert "nq_apng_max_bytes" in nq.abi_symbols()
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (40, 50)) for _ in range(3)]
    pal = 0xFF000000 | np.arange(256, dtype=np.int64)
    for S in (1, 7, 4096, 0, 65535):
        data = apng_ref.encode(frames, pal, segment_bytes=S)
        assert rectangles(frames)[1:] == [(0, 0, 50, 40)] * 2
        bound = nq.apng_max_bytes(3, 50, 40, S)
        assert len(data) <= bound == apng_ref.max_bytes(3, 50, 40, S), (S, len(data), bound)
        assert bound == nq.png_max_bytes([50] * 3, [40] * 3, None, S) + 58
    for bad in ((0, 4, 4, 0), (1, 0, 4, 0), (1, 4, 65536, 0), (1, 4, 4, -1), (1, 4, 4, 65536), (1, 65535, 65535, 0)):
        with pytest.raises(nq.NqError):
            nq.apng_max_bytes(*bad)


# the sprite animation of test_gpu_gif_delta.py, already in index space: a 16 x 16 sprite over a static 128 x 96 noise background
W, H, SPRITE = 128, 96, 16


def sprite_frames(K=255):
    rng = np.random.default_rng(8)
    back = rng.integers(0, K, (H, W))
    sprite = rng.integers(0, K, (SPRITE, SPRITE))
    frames = []
    for i in range(4):
        f = back.copy()
        x, y = 9 + 23 * i, 13 + 17 * i
        f[y:y + SPRITE, x:x + SPRITE] = sprite
        frames.append(f)
    return frames


def test_delta_file_is_smaller_than_the_separate_stills():
    """Computed on the restatement (deterministic; the GPU bytes equal it), on the 4-frame sprite animation with K = 255 indices; the
    figures are this test's own print.  Mark mode (the 255 opaque entries): 15 742 bytes against 52 989 for four separate PNG files,
    0.297x.  Crop mode (the same frames over the same entries plus a 256th, unused one, which leaves no room for u): 17 570
    against 53 001 bytes, 0.332x.  One bound per mode, each the computed ratio plus 0.01: 0.31 and 0.34.  Crop mode's figure is the geometry -- frame 0 is a
    quarter of the stills and each of the three rectangles covers the sprite's old and new place, 39 x 33 of 128 x 96 pixels: 0.25 +
    3 x 0.105 / 4 = 0.329, noise gains nothing -- and mark mode's is below it because its unchanged pixels are one repeated index;
    a restatement that stopped marking them would land on crop mode's figure and fail the first bound.  The mark-mode file must
    also be smaller than the crop-mode file of the same frames."""
    frames = sprite_frames(255)
    assert rectangles(frames)[1:] == [(9 + 23 * (i - 1), 13 + 17 * (i - 1), 23 + SPRITE, 17 + SPRITE) for i in (1, 2, 3)]
    size = {}
    for mode, K, bound in (("mark", 255, 0.31), ("crop", 256, 0.34)):
        pal = 0xFF000000 | np.arange(K, dtype=np.int64)
        assert (apng_ref.unchanged_index(pal) is not None) == (mode == "mark")
        data = apng_ref.encode(frames, pal)
        stills = sum(len(png_ref.encode(f, pal)) for f in frames)
        print("%s mode: delta %d bytes, stills %d bytes, ratio %.3f" % (mode, len(data), stills, len(data) / stills))
        assert len(data) < bound * stills, (mode, len(data), stills)
        composes_back(data, frames, pal, mode)
        size[mode] = len(data)
    assert size["mark"] < size["crop"], size


def test_symbols_and_wrappers_are_exported(nq):
    L = nq.load_library()
    for name in ("nq_apng_max_bytes", "nq_encode_apng_device", "nq_encode_apng"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
    for name in ("apng_max_bytes", "encode_apng", "encode_apng_device", "write_apng", "convert_frames_to_apng"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    import inspect
    p = inspect.signature(nq.encode_apng).parameters
    assert list(p) == ["frames", "palette", "delays_cs", "loop", "segment_bytes", "device", "return_rects"]
    p = inspect.signature(nq.convert_frames_to_apng).parameters
    assert list(p)[:8] == ["kind", "frames", "nMaxColors", "dither", "delays_cs", "loop", "seeds", "tile"]


def test_null_handle_and_bad_shapes_are_refused_without_a_device(nq):
    """What can be refused without a handle (a handle needs a device): a NULL handle and bad shape arguments answer -1
    (NQ_ERR_INVALID) and leave the outputs alone."""
    import ctypes as C
    L = nq.load_library()
    size = C.c_int64(-7)
    a = np.zeros((4, 4), np.uint16)
    src = (C.c_void_p * 1)(a.ctypes.data)
    pal = np.array([0xFF000000, 0xFFFFFFFF], np.uint32)
    buf = np.zeros(4096, np.uint8)
    for entry in ("nq_encode_apng", "nq_encode_apng_device"):
        assert getattr(L, entry)(None, 1, src, 4, 4, pal.ctypes.data, 2, None, 0, 0, buf.ctypes.data, 4096, C.byref(size), None) == -1
        assert size.value == -7
    out = C.c_int64(-7)
    assert L.nq_apng_max_bytes(1, 4, 4, 0, None) == -1 and L.nq_apng_max_bytes(0, 4, 4, 0, C.byref(out)) == -1 and out.value == -7


def test_python_argument_checks(nq):
    pal = [0xFF000000, 0xFFFFFFFF]
    with pytest.raises(ValueError):
        nq.encode_apng([], pal)
    with pytest.raises(ValueError):
        nq.encode_apng([np.zeros((4, 4), np.uint16), np.zeros((4, 5), np.uint16)], pal)
    with pytest.raises(TypeError):
        nq.encode_apng([np.zeros((4, 4), np.float32)], pal)
    with pytest.raises(ValueError):
        nq.encode_apng([np.full((4, 4), 70000)], pal)
    with pytest.raises(ValueError):
        nq.convert_frames_to_apng(0, [np.zeros((4, 4), np.int32), np.zeros((5, 4), np.int32)], 16, True)
    with pytest.raises(ValueError):
        nq.convert_frames_to_apng(0, [np.zeros((4, 4), np.int32)] * 2, 257, True)
    with pytest.raises(ValueError):
        nq.convert_frames_to_apng(0, [], 16, True)
    with pytest.raises(ValueError):
        nq.encode_apng_device(None, [], 4, 4, pal)


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_encode_apng_has_no_cpu_fallback(nq, tmp_path):
    maps = [np.zeros((8, 8), np.uint16), np.ones((8, 8), np.uint16)]
    for m in (maps, maps[:1]):
        with pytest.raises(nq.NqError) as e:
            nq.encode_apng(m, [0xFF000000, 0xFFFFFFFF])
        assert e.value.status == -5
    with pytest.raises(nq.NqError) as e:
        nq.write_apng(str(tmp_path / "a.png"), maps, [0xFF000000, 0xFFFFFFFF])
    assert e.value.status == -5 and not (tmp_path / "a.png").exists()
    with pytest.raises(nq.NqError) as e:
        nq.convert_frames_to_apng(0, [np.full((8, 8), -1, np.int32)] * 2, 16, False)
    assert e.value.status == -5
