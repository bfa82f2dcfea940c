"""CPU-side checks of the YUV input (include/nquant_abi.h "YUV input"): the restatement in yuv_ref.py that the GPU tests compare
against (its coefficients from the exact rationals and the header's table, within one level of the exact formula over all 2^24
triples and differing from it in at most 1e-3 of them, grey and the limited range's end points), yuv_planes, the Python argument
errors, the no-device error and the interface: the four symbols in the built library and the Python entry points."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import yuv_ref as Y
from conftest import HAS_GPU, ROOT

FLAG_WORDS = (0, Y.BT709, Y.FULL_RANGE, Y.BT709 | Y.FULL_RANGE)


def test_coefficients_are_the_rounded_rationals_and_the_headers_table():
    for flags in FLAG_WORDS:
        es, yo = Y.rationals(flags)
        got, yo2 = Y.coefficients(flags)
        assert yo == yo2 == (0 if flags & Y.FULL_RANGE else 16)
        for e, c in zip(es, got):
            assert isinstance(e, Fraction) and isinstance(c, int)
            assert Fraction(c) <= 65536 * e + Fraction(1, 2) < Fraction(c + 1)             # c = floor(65536 e + 1/2)
        assert got == Y.HEADER_TABLE[flags], flags
    # the header's text carries the same rows
    header = open(os.path.join(ROOT, "include", "nquant_abi.h")).read()
    for name, flags in (("601 limited", 0), ("601 full", Y.FULL_RANGE), ("709 limited", Y.BT709), ("709 full", Y.BT709 | Y.FULL_RANGE)):
        m = re.search(r"%s\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)" % name, header)
        assert m and tuple(int(v) for v in m.groups()) == Y.HEADER_TABLE[flags], name
    assert re.search(r"#define\s+NQ_YUV_BT709\s+1\b", header) and re.search(r"#define\s+NQ_YUV_FULL_RANGE\s+2\b", header)


@pytest.mark.parametrize("flags", FLAG_WORDS)
def test_every_triple_is_within_one_level_of_the_exact_formula(flags):
    """All 2^24 (Y, U, V), one luma value at a time.  The share of triples that differ at all is capped at 1e-3 per channel so that
    "within 1" cannot hide a wrong coefficient (the restatement stays below 5.2e-4: B of BT.601 full range)."""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    differ = np.zeros(3, np.int64)
    worst = 0
    for luma in range(256):
        got = Y.pixel(np.full(U.shape, luma), U, V, flags)
        want = Y.exact(np.full(U.shape, luma), U, V, flags)
        for c in range(3):
            d = np.abs(got[c] - want[c])
            worst = max(worst, int(d.max()))
            differ[c] += int((d != 0).sum())
    share = differ / float(2**24)
    print("flags %d: worst %d, share of differing triples R %.2e G %.2e B %.2e" % ((flags, worst) + tuple(share)))
    assert worst <= 1
    assert (share <= 1e-3).all(), share


def test_grey_and_the_ends_of_the_limited_range():
    v = np.arange(256)
    mid = np.full(256, 128)
    for flags in (Y.FULL_RANGE, Y.FULL_RANGE | Y.BT709):
        for c in Y.pixel(v, mid, mid, flags):
            assert (c == v).all()                                                           # full-range grey is the identity
    for flags in (0, Y.BT709):
        assert [int(c[0]) for c in Y.pixel([16], [128], [128], flags)] == [0, 0, 0]
        assert [int(c[0]) for c in Y.pixel([235], [128], [128], flags)] == [255, 255, 255]
        assert all((c[:17] == 0).all() and (c[235:] == 255).all() for c in Y.pixel(v, mid, mid, flags))
    # the word: alpha 255, channels at shifts 16, 8, 0; the chroma sample of pixel (x, y) is (x >> 1, y >> 1)
    y = np.full((3, 5), 128, np.uint8)
    u = np.array([[128, 128, 128], [255, 128, 128]], np.uint8)
    v = np.full((2, 3), 128, np.uint8)
    got = Y.convert_one(y, u, v, Y.FULL_RANGE).view(np.uint32)
    assert (got >> 24 == 255).all()
    blue = got & 255
    assert (blue[:2] == 128).all() and (blue[2, :2] == 255).all() and (blue[2, 2:] == 128).all()


@pytest.mark.parametrize("layout", ["nv12", "nv21", "i420", "yv12"])
@pytest.mark.parametrize("size", [(7, 5), (8, 4), (1, 1), (5, 2)], ids=lambda s: "%dx%d" % s)
def test_yuv_planes_returns_views_with_the_layouts_strides(nq, layout, size):
    w, h = size
    cw2, ch2 = (w + 1) // 2, (h + 1) // 2
    buf = np.arange(w * h + 2 * cw2 * ch2, dtype=np.int64).astype(np.uint8)
    y, u, v = nq.yuv_planes(buf, w, h, layout)
    base = buf.ctypes.data
    assert y.shape == (h, w) and u.shape == v.shape == (ch2, cw2)
    assert all(np.shares_memory(p, buf) and p.dtype == np.uint8 for p in (y, u, v))
    assert y.ctypes.data == base and y.strides == (w, 1)
    off = {"nv12": (0, 1), "nv21": (1, 0), "i420": (0, cw2 * ch2), "yv12": (cw2 * ch2, 0)}[layout]
    assert (u.ctypes.data - base - w * h, v.ctypes.data - base - w * h) == off
    want = (2 * cw2, 2) if layout in ("nv12", "nv21") else (cw2, 1)
    assert u.strides == want and v.strides == want
    buf[w * h + off[0]] ^= 0xFF                                                             # a view: a write to the buffer shows
    assert u[0, 0] == buf[w * h + off[0]]
    # the synthetic generator writes the same layout
    from nquant.android_amd import synth
    planes = {lay: nq.yuv_planes(synth.yuv420(w, h, 5, lay), w, h, lay) for lay in ("nv12", layout)}
    assert all((a == b).all() for a, b in zip(planes["nv12"], planes[layout]))
    assert synth.yuv420(w, h, 5, layout).dtype == np.uint8 and (synth.yuv420(w, h, 5, layout) == synth.yuv420(w, h, 5, layout)).all()


def test_yuv_planes_argument_errors(nq):
    buf = np.zeros(7 * 5 + 2 * 4 * 3, np.uint8)
    with pytest.raises(ValueError):
        nq.yuv_planes(buf, 7, 5, "nv16")
    with pytest.raises(ValueError):
        nq.yuv_planes(buf[:-1], 7, 5, "nv12")
    with pytest.raises(ValueError):
        nq.yuv_planes(buf, 0, 5, "nv12")
    with pytest.raises(TypeError):
        nq.yuv_planes(buf.astype(np.int32), 7, 5, "nv12")
    with pytest.raises(TypeError):
        nq.yuv_planes(np.zeros(2 * buf.size, np.uint8)[::2], 7, 5, "nv12")


def test_python_argument_errors_need_no_device(nq):
    from nquant.android_amd import yuv as M
    y, u, v = Y.random_planes(7, 5, 1)
    for bad in ([], [(y, u)], [y], [(y.astype(np.int32), u, v)], [(y, u[:, :2], v)], [(y, u, v), (y[:4], u, v)], [(y.reshape(-1), u, v)]):
        with pytest.raises((ValueError, TypeError)):
            M._host_frames(bad)
    # views that one set of strides describes are passed as they are; anything else is copied tight
    buf = np.zeros(7 * 5 + 2 * 4 * 3, np.uint8)
    planes, w, h, ys, cs, step = M._host_frames([nq.yuv_planes(buf, 7, 5, "nv12")])
    assert (w, h, ys, cs, step) == (7, 5, 7, 8, 2) and all(np.shares_memory(p, buf) for p in planes[0])
    planes, w, h, ys, cs, step = M._host_frames([(y, u, v)])
    assert (ys, cs, step) == (7, 4, 1) and planes[0][0] is y
    wide = np.zeros((5, 16), np.uint8)
    planes, w, h, ys, cs, step = M._host_frames([(wide[:, :7], u, v)])
    assert (ys, cs, step) == (16, 4, 1) and np.shares_memory(planes[0][0], wide)
    planes, w, h, ys, cs, step = M._host_frames([(y, u, v), nq.yuv_planes(buf, 7, 5, "nv12")])       # two layouts in one call
    assert (ys, cs, step) == (7, 4, 1) and not np.shares_memory(planes[1][1], buf)
    planes, w, h, ys, cs, step = M._host_frames([(y[::-1], u, v)])                                    # a negative stride
    assert (ys, cs, step) == (7, 4, 1) and (planes[0][0] == y[::-1]).all() and planes[0][0].strides == (7, 1)
    planes, w, h, ys, cs, step = M._host_frames([(y, np.zeros((3, 12), np.uint8)[:, ::3], v)])        # an element stride of 3
    assert (ys, cs, step) == (7, 4, 1)
    for bad in ("bt709", {"bt2020": True}, 1):
        with pytest.raises(TypeError):
            M._yuv_keyword(bad)
    assert M._yuv_keyword({}) == 0 and M._yuv_keyword({"bt709": True}) == 1 and M._yuv_keyword({"full_range": True, "bt709": True}) == 3
    with pytest.raises(ValueError):
        nq.frames_from_yuv_device(None, [], [], [], 4, 4, 4, 2, 1, [])
    with pytest.raises(ValueError):
        nq.resample_frames_yuv_device(None, [], [], [], 4, 4, 4, 2, 1, [], (2, 2))


def test_yuv_symbols_and_wrappers_are_exported(nq):
    L = nq.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nquant_abi.h")).read(), flags=re.S)
    for name in ("nq_frames_from_yuv_device", "nq_frames_from_yuv", "nq_resample_frames_yuv_device", "nq_resample_frames_yuv"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("frames_from_yuv", "frames_from_yuv_device", "resample_frames_yuv", "resample_frames_yuv_device", "yuv_planes"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    for fn in (nq.convert_frames_to_gif, nq.convert_shots_to_gif, nq.convert_clip_to_gif, nq.convert_frames_to_apng, nq.convert_frames_refined,
               nq.convert_frames_ordered):
        assert inspect.signature(fn).parameters["yuv"].default is None, fn.__name__
    p = inspect.signature(nq.resample_frames_yuv).parameters
    assert [p[k].default for k in ("crop", "linear", "bt709", "full_range", "device")] == [None, True, False, False, 0]
    # a null handle is refused by all four
    assert L.nq_frames_from_yuv(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, None) == -1
    assert L.nq_frames_from_yuv_device(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, None) == -1
    assert L.nq_resample_frames_yuv(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, 0, 0, 4, 4, None, 2, 2, 1) == -1
    assert L.nq_resample_frames_yuv_device(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, 0, 0, 4, 4, None, 2, 2, 1) == -1


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_without_a_device_every_call_raises_no_device(nq):
    frames = [Y.random_planes(8, 4, 2)]
    calls = [lambda: nq.frames_from_yuv(frames), lambda: nq.resample_frames_yuv(frames, (4, 2)),
             lambda: nq.convert_frames_to_gif(1, frames, 16, True, yuv={}),
             lambda: nq.convert_frames_to_gif(1, frames, 16, True, size=(4, 2), yuv={"bt709": True}),
             lambda: nq.convert_shots_to_gif(1, frames, [0], 16, True, yuv={}),
             lambda: nq.convert_clip_to_gif(1, frames, 16, True, yuv={}),
             lambda: nq.convert_frames_to_apng(1, frames, 16, True, yuv={}),
             lambda: nq.convert_frames_refined(1, frames, 16, True, 1, yuv={}),
             lambda: nq.convert_frames_ordered(1, frames, 16, 8, yuv={})]
    for call in calls:
        with pytest.raises(nq.NqError) as e:
            call()
        assert e.value.status == -5
