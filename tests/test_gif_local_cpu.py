"""GIF files with one colour table per frame, without a GPU: the restatement in gif_local_ref.py writes files that its own parser and
Pillow compose back to the colours every frame shows (full frames and delta mode, every K of the definition in one file), within the
threshold under lossy; with equal palettes it is the delta restatement's canvas; the named edge cases of "changed by colour"; the size
bound; and the library declares, exports and guards the five calls."""
import ctypes as C
import os

import numpy as np
import pytest

import gif_delta_ref
import gif_local_cases as cases
import gif_local_ref as R
import gif_ref
from conftest import HAS_GPU
from gif_delta_cases import palette_of, pillow_canvases, sequence

SHAPES = ((1, 1), (1, 40), (23, 1), (19, 31))


def _segments(h, w):
    return (0, 7, h * w)


def _composes(gif, want, why, lossy=0):
    """The restatement's own parser and Pillow compose the file to `want` (RGB per frame), within `lossy` per channel."""
    own = R.compose(gif)
    assert len(own) == len(want), why
    for i, (c, f) in enumerate(zip(own, want)):
        assert c.shape == f.shape and np.abs(c.astype(int) - f.astype(int)).max() <= lossy, (why, i)
    pytest.importorskip("PIL")
    got = pillow_canvases(gif)
    assert len(got) == len(want), why
    for i, (g, f) in enumerate(zip(got, want)):
        assert np.abs(g.astype(int) - f.astype(int)).max() <= lossy, (why, i, "Pillow")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("delta", [False, True])
def test_files_compose_back_to_the_colours_shown(shape, delta):
    h, w = shape
    rng = np.random.default_rng(7 * h + w)
    frames, pals = cases.mixed(h, w, rng)
    delays = [(3 * i) % 7 for i in range(len(frames))]
    want = cases.shown(frames, pals)
    for S in _segments(h, w):
        data, subs = (R.encode_delta if delta else R.encode)(frames, pals, delays, 0, S)
        assert subs == 0
        _composes(data, want, (shape, delta, S))
        screen, parsed = R.parse(data)
        assert screen["packed"] == 0x70 and screen["loop"] == 0 and all(p["local"] for p in parsed)
        assert [p["m"] for p in parsed] == [gif_ref.min_code_size(len(p_) + (delta and len(p_) < 256)) for p_ in pals]
        assert [p["delay"] for p in parsed] == delays
        if delta:
            assert [(p["x"], p["y"], p["w"], p["h"]) for p in parsed] == R.rectangles(frames, pals)
            assert parsed[1]["w"] * parsed[1]["h"] == 1 and all(p["disposal"] == 1 for p in parsed)
        assert len(data) <= R.max_bytes([f.shape for f in frames], S)


@pytest.mark.parametrize("delta", [False, True])
def test_lossy_16_stays_within_16_per_channel(delta):
    substituted = 0
    for h, w in SHAPES:
        rng = np.random.default_rng(h + 3 * w)
        frames, pals = cases.mixed(h, w, rng, near=True)
        want = cases.shown(frames, pals)
        for S in _segments(h, w):
            data, subs = (R.encode_delta if delta else R.encode)(frames, pals, None, 0, S, 16)
            substituted += subs
            _composes(data, want, (h, w, delta, S), 16)
            if delta:                                # rectangles do not depend on lossy
                assert [(p["x"], p["y"], p["w"], p["h"]) for p in R.parse(data)[1]] == R.rectangles(frames, pals)
    assert substituted > 0


def test_one_frame_is_the_local_form_not_the_global_one():
    rng = np.random.default_rng(3)
    a, pal = rng.integers(0, 17, (19, 31)), palette_of(17, rng)
    data, _ = R.encode([a], [pal], segment_pixels=7)
    assert R.encode_delta([a], [pal], segment_pixels=7)[0] == data
    assert data != gif_ref.encode(a, pal, segment_pixels=7)
    screen, parsed = R.parse(data)
    assert screen["packed"] == 0x70 and parsed[0]["local"] and "delay" not in parsed[0]
    assert (parsed[0]["index"] == a).all()
    # a transparent entry brings the extension back, without a disposal
    pal[5] &= 0x00FFFFFF
    _, parsed = R.parse(R.encode([a], [pal])[0])
    assert parsed[0]["transparency"] == 5 and parsed[0]["disposal"] == 0


@pytest.mark.parametrize("K", [2, 17, 255, 256])
def test_equal_palettes_give_the_delta_restatements_canvases(K):
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng)
    assert len(set((pal & 0xFFFFFF).tolist())) == K          # no duplicate colours: "by colour" is "by index"
    frames = sequence(19, 31, K, rng)
    for S in (0, 7):
        data, _ = R.encode_delta(frames, [pal] * len(frames), None, 0, S)
        old = gif_delta_ref.encode(frames, pal, None, 0, S)
        assert R.rectangles(frames, [pal] * len(frames)) == gif_delta_ref.rectangles(frames)
        for c, o in zip(R.compose(data), gif_delta_ref.compose(old)):
            assert (c == cases.rgb_of(o, pal)).all()
        # the bodies are the same index maps, so the frames' data are the same bytes: only the tables moved
        assert [p["index"].tolist() for p in R.parse(data)[1]] == [p["index"].tolist() for p in gif_delta_ref.parse(old)[2]]


def test_named_edge_cases():
    rng = np.random.default_rng(21)
    for name, (frames, pals, rects) in cases.edge_cases(rng).items():
        if rects is not None:
            assert R.rectangles(frames, pals) == rects, name
        for S in (0, 7):
            data, _ = R.encode_delta(frames, pals, [2, 3], -1, S)
            _composes(data, cases.shown(frames, pals), (name, S))
            _, parsed = R.parse(data)
            assert [p["transparency"] for p in parsed] == [len(p) if len(p) < 256 else None for p in pals], name
    # the body of "equal rgb" marks the pixel that moved between the two equal entries as unchanged
    frames, pals, _ = cases.edge_cases(np.random.default_rng(21))["equal rgb"]
    assert R.bodies(frames, pals)[1].tolist() == [[1]]
    assert R.changed(frames, pals, 1).sum() == 1 and (frames[0] != frames[1]).sum() == 2


def test_every_file_is_within_the_bound(nq):
    rng = np.random.default_rng(4)
    for (h, w), S in (((40, 40), 1), ((40, 40), 0), ((1, 1), 1), ((19, 31), 7)):
        frames = [rng.integers(0, 256, (h, w)) for _ in range(3)]
        pals = [palette_of(256, rng) for _ in range(3)]
        bound = nq.gif_local_max_bytes([w] * 3, [h] * 3, S)
        assert bound == R.max_bytes([(h, w)] * 3, S) == nq.gif_max_bytes([w] * 3, [h] * 3, 256, S) + 768 * 3
        for enc in (R.encode, R.encode_delta):
            assert len(enc(frames, pals, None, 0, S)[0]) <= bound, (h, w, S)
        assert len(R.encode(frames[:1], pals[:1], None, 0, S)[0]) <= nq.gif_local_max_bytes([w], [h], S)
    with pytest.raises(nq.NqError):
        nq.gif_local_max_bytes([0], [4])
    with pytest.raises(ValueError):
        nq.gif_local_max_bytes([4, 4], [4])


NAMES = ("nq_gif_local_max_bytes", "nq_encode_gif_local_device", "nq_encode_gif_local", "nq_encode_gif_local_delta_device",
         "nq_encode_gif_local_delta")


def test_the_library_declares_and_exports_the_five_calls(nq):
    L = nq.load_library()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nquant_abi.h")).read()
    for name in NAMES:
        assert name in nq.abi_symbols() and hasattr(L, name) and ("int %s(" % name) in header, name
    import inspect
    for fn in (nq.encode_gif_local, nq.encode_gif_local_device, nq.encode_gif_local_delta, nq.encode_gif_local_delta_device):
        p = inspect.signature(fn).parameters
        assert p["lossy"].default == 0 and "palettes" in p, fn.__name__
    for fn in (nq.encode_gif_local_delta, nq.encode_gif_local_delta_device):
        assert inspect.signature(fn).parameters["return_rects"].default is False
    p = inspect.signature(nq.convert_shots_to_gif).parameters
    assert list(p)[:5] == ["kind", "frames", "shot_starts", "nMaxColors", "dither"] and list(p)[-1] == "delta" and p["delta"].default is True
    # the older entry points keep their last parameter
    assert list(inspect.signature(nq.write_gif).parameters)[-1] == "delta"
    assert list(inspect.signature(nq.convert_frames_to_gif).parameters)[-1] == "delta"


def test_python_argument_errors(nq):
    a = np.zeros((4, 6), np.uint16)
    pal = [0xFF000000, 0xFFFFFFFF]
    with pytest.raises(ValueError):
        nq.encode_gif_local([a, a], [pal])                      # one palette per frame
    with pytest.raises(ValueError):
        nq.encode_gif_local_delta([a, np.zeros((4, 5), np.uint16)], [pal, pal])
    with pytest.raises(ValueError):
        nq.encode_gif_local([], [])
    with pytest.raises(TypeError):
        nq.encode_gif_local([a.astype(np.float32)], [pal])
    frames = [np.zeros((4, 6), np.int32)] * 3
    for starts in ([], [1], [0, 0], [0, 2, 1], [0, 3]):
        with pytest.raises(ValueError):
            nq.convert_shots_to_gif(0, frames, starts, 16, True)
    with pytest.raises(ValueError):
        nq.convert_shots_to_gif(0, frames, [0], 257, True)
    with pytest.raises(ValueError):
        nq.convert_shots_to_gif(0, frames, [0], 16, True, hold=4, delta=False)
    with pytest.raises(TypeError):
        nq.convert_shots_to_gif(0, frames, [0], 16, True, lossy=True)
    with pytest.raises(ValueError):
        nq.convert_shots_to_gif(0, frames, [0], 16, True, seeds=[1])


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_without_a_device_every_call_raises_status_minus_5(nq):
    a = np.zeros((4, 6), np.uint16)
    pal = [0xFF000000, 0xFFFFFFFF]
    calls = (lambda: nq.encode_gif_local([a], [pal]), lambda: nq.encode_gif_local_delta([a, a], [pal, pal]),
             lambda: nq.convert_shots_to_gif(0, [np.zeros((4, 6), np.int32)] * 2, [0, 1], 16, True))
    for call in calls:
        with pytest.raises(nq.NqError) as e:
            call()
        assert e.value.status == -5
    # the two device forms, on a bare handle that needs no device to exist
    L = nq.load_library()
    h = C.c_void_p()
    if L.nq_create(0, 0, C.byref(h)) == 0:
        src = (C.c_void_p * 1)(a.ctypes.data)
        p = np.array(pal, np.uint32)
        K, one, size, buf = np.array([2], np.int32), np.array([4], np.int32), C.c_int64(0), np.zeros(4096, np.uint8)
        assert L.nq_encode_gif_local_device(h, 1, src, one.ctypes.data, one.ctypes.data, p.ctypes.data, 2, K.ctypes.data, None, 0, 0, 0,
                                            buf.ctypes.data, 4096, C.byref(size)) == -5
        assert L.nq_encode_gif_local_delta_device(h, 1, src, 4, 4, p.ctypes.data, 2, K.ctypes.data, None, 0, 0, 0, buf.ctypes.data, 4096,
                                                  C.byref(size), None) == -5
        L.nq_destroy(h)
