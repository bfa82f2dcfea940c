"""CPU-side checks of the delta-mode GIF encoder (include/nquant_abi.h "GIF encoding, delta mode"): the restatement in
gif_delta_ref.py gives files that compose back to the frames, through its own parser and through Pillow (so the bytes the GPU tests
compare against are right); one frame gives gif_ref's bytes; gif_ref.max_bytes bounds every file; the symbols and wrappers exist;
without a HIP device the host form refuses to compute (no CPU fallback)."""
import numpy as np
import pytest

import gif_delta_ref
import gif_ref
from conftest import HAS_GPU
from gif_delta_cases import KS, palette_of, pillow_canvases, rgb_of, sequence

PIL = pytest.importorskip("PIL")

@pytest.mark.parametrize("K", KS)
def test_restatement_composes_back_to_the_frames(K):
    rng = np.random.default_rng(100 + K)
    pal = palette_of(K, rng)
    for h, w in ((1, 1), (1, 40), (23, 1), (19, 31)):
        frames = sequence(h, w, K, rng)
        for S in (0, 7, h * w):
            gif = gif_delta_ref.encode(frames, pal, delays_cs=list(range(len(frames))), loop=0, segment_pixels=S)
            screen, gct, parsed = gif_delta_ref.parse(gif)
            assert (screen["width"], screen["height"], screen["background"]) == (w, h, 0)
            u = gif_delta_ref.unchanged_index(K)
            assert len(gct) == 3 << (gif_ref.color_bits(K + (u is not None)) + 1)
            assert [(p["x"], p["y"], p["w"], p["h"]) for p in parsed] == gif_delta_ref.rectangles(frames)
            assert all(p["disposal"] == 1 and p["transparency"] == u and p["delay"] == i for i, p in enumerate(parsed))
            for i, (canvas, f) in enumerate(zip(gif_delta_ref.compose(gif), frames)):
                assert (canvas == f).all(), (K, h, w, S, i)
            assert len(gif) <= gif_ref.max_bytes([f.shape for f in frames], S), (K, h, w, S)
            got = pillow_canvases(gif)
            assert len(got) == len(frames)
            for i, (g, f) in enumerate(zip(got, frames)):
                assert (g == rgb_of(f, pal)).all(), (K, h, w, S, i)


def test_rectangles_of_the_sequence():
    rng = np.random.default_rng(1)
    h, w = 19, 31
    r = gif_delta_ref.rectangles(sequence(h, w, 16, rng))
    assert r[:9] == [(0, 0, w, h), (0, 0, 1, 1), (0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1),
                     (0, h - 1, w, 1), (w - 1, 0, 1, h)]
    assert r[9] == (w // 2, h // 3, w // 5, h // 4)
    assert r[10] == (w // 4, h // 4, w // 2 - w // 4 + 1, h // 2 - h // 4 + 1)


def test_bodies_mark_unchanged_pixels():
    a = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    b = a.copy()
    b[0, 0], b[1, 1] = 9, 9
    assert (gif_delta_ref.bodies([a, b], 10)[1] == [[9, 10], [10, 9]]).all()
    big = [a + 200, b + 200]
    assert (gif_delta_ref.bodies(big, 256)[1] == [[209, 201], [203, 209]]).all()        # K = 256: cropped only


@pytest.mark.parametrize("K", KS)
def test_one_frame_is_the_full_frame_file(K):
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng)
    pal[K // 2] &= 0x00FFFFFF                       # alpha 0 is allowed for one frame
    idx = rng.integers(0, K, (13, 29))
    for S in (0, 5):
        assert gif_delta_ref.encode([idx], pal, segment_pixels=S) == gif_ref.encode(idx, pal, segment_pixels=S)


def test_max_bytes_bounds_a_frame_that_changes_everywhere(nq):
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 255, (64, 64)) for _ in range(3)]
    for K in (255, 256):
        for S in (1, 0):
            gif = gif_delta_ref.encode(frames, 0xFF000000 | np.arange(K), segment_pixels=S)
            assert len(gif) <= gif_ref.max_bytes([(64, 64)] * 3, S)
            assert len(gif) <= nq.gif_max_bytes([64] * 3, [64] * 3, 256, S)


def test_delta_symbols_and_wrappers_are_exported(nq):
    L = nq.load_library()
    for name in ("nq_encode_gif_delta_device", "nq_encode_gif_delta"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
    for name in ("encode_gif_delta", "encode_gif_delta_device"):
        assert callable(getattr(nq, name)), name
    import inspect
    for fn in (nq.write_gif, nq.convert_frames_to_gif):
        p = list(inspect.signature(fn).parameters.values())[-1]
        assert p.name == "delta" and p.default is False, fn.__name__


def test_delta_python_argument_checks(nq):
    pal = [0xFF000000, 0xFFFFFFFF]
    with pytest.raises(ValueError):
        nq.encode_gif_delta([], pal)
    with pytest.raises(ValueError):
        nq.encode_gif_delta([np.zeros((4, 4), np.uint16), np.zeros((4, 5), np.uint16)], pal)
    with pytest.raises(TypeError):
        nq.encode_gif_delta([np.zeros((4, 4), np.float32)], pal)
    with pytest.raises(ValueError):
        nq.convert_frames_to_gif(0, [np.zeros((4, 4), np.int32), np.zeros((5, 4), np.int32)], 16, True, delta=True)
    with pytest.raises(ValueError):
        nq.convert_frames_to_gif(0, [np.zeros((4, 4), np.int32)] * 2, 257, True, delta=True)
    with pytest.raises(ValueError):
        nq.encode_gif_delta_device(None, [], 4, 4, pal)


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_encode_gif_delta_has_no_cpu_fallback(nq):
    maps = [np.zeros((8, 8), np.uint16), np.ones((8, 8), np.uint16)]
    for m in (maps, maps[:1]):
        with pytest.raises(nq.NqError) as e:
            nq.encode_gif_delta(m, [0xFF000000, 0xFFFFFFFF])
        assert e.value.status == -5
    with pytest.raises(nq.NqError) as e:
        nq.convert_frames_to_gif(0, [np.full((8, 8), -1, np.int32)] * 2, 16, False, delta=True)
    assert e.value.status == -5
