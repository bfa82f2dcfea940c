"""Orientation on the GPU (nq_orient_frames* and the *_oriented entry points): every result equals the restatement in orient_ref.py
word for word -- all 8 codes at one-dimensional sizes and at sides of ORIENT_TILE - 1, ORIENT_TILE and ORIENT_TILE + 1 in each dimension
independently, widths and heights that are and are not multiples of 4, sources and outputs on a 16-byte boundary and one word behind
it (both paths), three frames per buffer with guard words between the outputs, more tiles than the grid holds; the YUV forms in four
layouts and two flag words at odd sides, equal to the library's own two steps as well; the two reducing calls for ARGB and NV12
sources; host forms; rejected arguments; and the converters' orient= keyword."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orient_ref as O
import resample_ref as R
import yuv_ref as Y
from conftest import ROOT
from nquant.android_amd import gif as G
from test_gpu_yuv import _Planes, _Stream

pytestmark = pytest.mark.gpu


def _constant(name):
    src = open(os.path.join(ROOT, "nquant.android_amd", "csrc", "nq_orient.hip")).read()
    return int(re.search(r"constexpr (?:int|long long) %s = (\d+);" % name, src).group(1))


TILE, MAX_BLOCKS = _constant("ORIENT_TILE"), _constant("ORIENT_MAX_BLOCKS")
SHIFTS = ((0, 0), (1, 0), (0, 1))                              # (sources, outputs) in words behind a 16-byte boundary


def _kw(flags):
    return {"bt709": bool(flags & Y.BT709), "full_range": bool(flags & Y.FULL_RANGE)}


def _words(w, h, n, seed=0):
    """n frames whose words name their frame and place: no two words of a case are equal."""
    base = np.arange(w * h, dtype=np.int64).reshape(h, w)
    return [((base + (i + 1 + seed) * 0x01000000) & 0x7FFFFFFF).astype(np.int32) for i in range(n)]


@pytest.fixture(scope="module")
def q(nq):
    quantizer = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    yield quantizer
    quantizer.close()


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _argb_case(nq, q, frames, code, sshift, oshift):
    import torch
    h, w = frames[0].shape
    want = O.orient_all(frames, code)
    src = _Stream(frames, sshift, -7)
    dst = _Stream([np.full(r.shape, -9, np.int32) for r in want], oshift, -9)
    why = (w, h, len(frames), code, sshift, oshift)
    assert all(p % 16 == 4 * sshift for p in src.ptrs) and all(p % 16 == 4 * oshift for p in dst.ptrs), why
    torch.cuda.synchronize()
    nq.orient_frames_device(q, src.ptrs, w, h, dst.ptrs, code)
    torch.cuda.synchronize()
    got = dst.read()
    assert (got == dst.expect(want)).all(), (why, int((got != dst.expect(want)).sum()))      # the whole buffer: guards included
    assert (src.read() == src.host).all(), why


LINES = [(1, 1), (1, 5), (5, 1), (1, TILE - 1), (1, TILE), (1, TILE + 1), (TILE - 1, 1), (TILE, 1), (TILE + 1, 1), (4, 1), (1, 4)]
PLANES = [(w, h) for w in (TILE - 1, TILE, TILE + 1) for h in (TILE - 1, TILE, TILE + 1)] + \
         [(TILE + 4, 12), (12, TILE + 4), (8, 6), (6, 8), (2 * TILE + 8, TILE + 8)]


@pytest.mark.parametrize("size", LINES + PLANES, ids=lambda s: "%dx%d" % s)
def test_every_code_equals_the_restatement(nq, q, size):
    """Widths (and, for the turning codes, heights) that are multiples of 4 take the 16-byte path when every pointer is aligned, and
    the word path when sources or outputs lie one word on; every other size takes the word path."""
    w, h = size
    frames = _words(w, h, 3)
    for code in O.CODES:
        for sshift, oshift in SHIFTS:
            _argb_case(nq, q, frames, code, sshift, oshift)


def test_more_tiles_than_the_grid_holds(nq, q):
    """An item is (frame, tile) and the grid is capped at ORIENT_MAX_BLOCKS workgroups, which then stride over the rest: three thin
    frames of 1024 tiles each, in both directions and on both paths."""
    assert MAX_BLOCKS == 2048 and TILE == 64
    for (w, h), shift in (((1, 65535), 0), ((65535, 1), 0), ((4, 65532), 0), ((65532, 4), 0), ((4, 65532), 1)):
        tiles = 3 * -(-w // TILE) * -(-h // TILE)
        assert MAX_BLOCKS < tiles < 2 * MAX_BLOCKS
        frames = _words(w, h, 3)
        for code in (3, 5, 6):
            _argb_case(nq, q, frames, code, shift, shift)


_REF = {}


def _planes(w, h, n):
    key = (w, h, n)
    if key not in _REF:
        _REF[key] = [Y.random_planes(w, h, 1000 * w + 10 * h + i) for i in range(n)]
    return _REF[key]


def _converted(w, h, n, flags):
    key = (w, h, n, flags)
    if key not in _REF:
        _REF[key] = Y.convert(_planes(w, h, n), flags)
    return _REF[key]


YUV_SIZES = [(1, 1), (7, 3), (13, 9), (TILE + 1, 5), (5, TILE + 1), (8, 4), (12, 5), (TILE, 8), (TILE + 4, TILE + 4)]
YUV_LAYOUTS = ("i420", "i420pad5", "nv12", "nv21")


@pytest.mark.parametrize("size", YUV_SIZES, ids=lambda s: "%dx%d" % s)
def test_yuv_oriented_equals_convert_then_orient(nq, q, size):
    """Odd sides end in a column and a row whose chroma sample they do not share.  Widths 8, 12, 64 and 68 take the wide paths (the
    turning codes only where the height is a multiple of 4 too: 12 x 5 turns on the byte path) when planes and outputs are aligned and
    the strides allow it (not i420pad5); everything else takes the byte path.  One layout per size is also held against the library's
    own two steps."""
    import torch
    w, h = size
    n = 2
    frames = _planes(w, h, n)
    for flags in (0, Y.BT709 | Y.FULL_RANGE):
        full = _converted(w, h, n, flags)
        for code in O.CODES:
            want = O.orient_all(full, code)
            assert want[0].shape == O.oriented_size(w, h, code)[::-1]
            for layout in YUV_LAYOUTS:
                for pshift, oshift in ((0, 0), (1, 1)):
                    src = _Planes(frames, layout, pshift)
                    dst = _Stream([np.full(r.shape, -9, np.int32) for r in want], oshift, -9)
                    why = (w, h, flags, code, layout, pshift, oshift)
                    torch.cuda.synchronize()
                    nq.frames_from_yuv_device(q, src.y, src.u, src.v, *src.geometry(), dst.ptrs, orient=code, **_kw(flags))
                    torch.cuda.synchronize()
                    got = dst.read()
                    assert (got == dst.expect(want)).all(), (why, int((got != dst.expect(want)).sum()))
                    assert (src.read() == src.host).all(), why
            # the library's own two steps
            src = _Planes(frames, "nv12", 0)
            mid = _Stream([np.zeros((h, w), np.int32)] * n, 0, -7)
            two = _Stream([np.zeros_like(r) for r in want], 0, -9)
            nq.frames_from_yuv_device(q, src.y, src.u, src.v, *src.geometry(), mid.ptrs, **_kw(flags))
            nq.orient_frames_device(q, mid.ptrs, w, h, two.ptrs, code)
            torch.cuda.synchronize()
            assert (two.read() == two.expect(want)).all(), (w, h, flags, code)


# (source size, crop in oriented coordinates for codes 1..4 (x and y change places for 5..8), target likewise)
REDUCTIONS = [((24, 16), (3, 1, 17, 12), (5, 4)),               # an odd origin, a non-integer ratio
              ((24, 16), (1, 3, 16, 8), (16, 8)),               # 1:1
              ((24, 16), None, (7, 5)),
              ((TILE + 8, TILE + 4), (5, 3, TILE, TILE - 1), (TILE - 3, 9))]


def _for_code(code, crop, size):
    if code < 5:
        return crop, size
    return (None if crop is None else (crop[1], crop[0], crop[3], crop[2])), size[::-1]


@pytest.mark.parametrize("case", REDUCTIONS, ids=lambda c: "%dx%d-%s" % (c[0][0], c[0][1], "full" if c[1] is None else "crop%d-%d" % c[1][:2]))
def test_reducing_calls_equal_their_definitions(nq, q, case):
    """nq_resample_frames_oriented = orient, then reduce; nq_resample_frames_yuv_oriented = convert, orient, reduce: against the
    restatement and against the library's own steps, for an ARGB source (with transparent pixels) and an NV12 source."""
    import torch
    (w, h), crop0, size0 = case
    n = 2
    argb = [R.random_argb(w, h, 60 + i) for i in range(n)]
    planes = _planes(w, h, n)
    full = _converted(w, h, n, Y.BT709)
    for code in O.CODES:
        crop, size = _for_code(code, crop0, size0)
        ow, oh = O.oriented_size(w, h, code)
        for linear in (True, False):
            flags = R.LINEAR if linear else 0
            why = (w, h, code, crop, size, linear)
            # ARGB
            want = O.resample_oriented(argb, code, size, crop, flags)
            src = _Stream(argb, 0, -7)
            one = _Stream([np.full(r.shape, -9, np.int32) for r in want], 1, -9)
            mid = _Stream([np.zeros((oh, ow), np.int32)] * n, 0, -7)
            two = _Stream([np.full(r.shape, -9, np.int32) for r in want], 1, -9)
            nq.resample_frames_device(q, src.ptrs, w, h, one.ptrs, size, crop, linear, orient=code)
            nq.orient_frames_device(q, src.ptrs, w, h, mid.ptrs, code)
            nq.resample_frames_device(q, mid.ptrs, ow, oh, two.ptrs, size, crop, linear)
            torch.cuda.synchronize()
            assert (one.read() == one.expect(want)).all(), why
            assert (two.read() == two.expect(want)).all(), why
            assert (src.read() == src.host).all(), why
            # NV12
            want = R.resample(O.orient_all(full, code), size, crop, flags)
            ysrc = _Planes(planes, "nv12", 0)
            one = _Stream([np.full(r.shape, -9, np.int32) for r in want], 0, -9)
            conv = _Stream([np.zeros((h, w), np.int32)] * n, 0, -7)
            two = _Stream([np.full(r.shape, -9, np.int32) for r in want], 0, -9)
            nq.resample_frames_yuv_device(q, ysrc.y, ysrc.u, ysrc.v, *ysrc.geometry(), one.ptrs, size, crop, linear, bt709=True, orient=code)
            nq.frames_from_yuv_device(q, ysrc.y, ysrc.u, ysrc.v, *ysrc.geometry(), conv.ptrs, bt709=True)
            nq.orient_frames_device(q, conv.ptrs, w, h, mid.ptrs, code)
            nq.resample_frames_device(q, mid.ptrs, ow, oh, two.ptrs, size, crop, linear)
            torch.cuda.synchronize()
            assert (one.read() == one.expect(want)).all(), why
            assert (two.read() == two.expect(want)).all(), why
            assert (ysrc.read() == ysrc.host).all(), why


def test_host_forms_equal_the_device_forms(nq):
    """... which gave the restatement above: the host forms are held against it."""
    for (w, h), crop0, size0 in (((13, 9), (3, 1, 8, 6), (3, 4)), ((TILE + 4, 8), None, (9, 5))):
        argb = [R.random_argb(w, h, 80 + i) for i in range(3)]
        planes = _planes(w, h, 3)
        keep = [a.copy() for a in argb]
        for code in O.CODES:
            crop, size = _for_code(code, crop0, size0)
            got = nq.orient_frames(argb, code)
            assert len(got) == 3 and all(g.dtype == np.int32 and g.shape == r.shape and (g == r).all() for g, r in zip(got, O.orient_all(argb, code)))
            got = nq.frames_from_yuv(planes, full_range=True, orient=code)
            assert all(g.shape == r.shape and (g == r).all() for g, r in zip(got, O.yuv_oriented(planes, code, Y.FULL_RANGE))), code
            for linear in (True, False):
                flags = R.LINEAR if linear else 0
                got = nq.resample_frames(argb, size, crop=crop, linear=linear, orient=code)
                assert all(g.shape == r.shape and (g == r).all() for g, r in zip(got, O.resample_oriented(argb, code, size, crop, flags))), code
                got = nq.resample_frames_yuv(planes, size, crop=crop, linear=linear, full_range=True, orient=code)
                want = O.resample_yuv_oriented(planes, code, size, crop, Y.FULL_RANGE, flags)
                assert all(g.shape == r.shape and (g == r).all() for g, r in zip(got, want)), code
            # size and crop both None: the whole oriented frame at its own size
            got = nq.resample_frames(argb, None, orient=code)
            assert all((g == r).all() for g, r in zip(got, O.resample_oriented(argb, code)))
            got = nq.resample_frames_yuv(planes, None, orient=code)
            assert all((g == r).all() for g, r in zip(got, O.yuv_oriented(planes, code)))
        assert all((a == b).all() for a, b in zip(argb, keep))


def test_invalid_arguments_then_a_valid_call(nq, hd):
    """Every rejected call returns NQ_ERR_INVALID with an error text and leaves the pre-filled outputs and the sources alone, in
    host and device memory; the next valid call on the same handle is right."""
    import torch
    L = hd._L
    w, h, n = 12, 6, 2
    argb = _words(w, h, n, 5)
    planes = [tuple(np.ascontiguousarray(p) for p in f) for f in _planes(w, h, n)]
    full = Y.convert(planes, 0)
    hsrc = [a.reshape(-1).copy() for a in argb]
    hyuv = [np.concatenate([p.reshape(-1) for p in f]) for f in planes]               # I420, tight
    hdst = [np.full(w * h + 2, -9, np.int32) for _ in range(n)]
    dsrc = [torch.from_numpy(a).cuda() for a in hsrc]
    dyuv = [torch.from_numpy(a).cuda() for a in hyuv]
    ddst = [torch.from_numpy(a).cuda() for a in hdst]
    cw2, ch2 = w // 2, h // 2
    arr = lambda v: (C.c_void_p * len(v))(*v)

    def ptrs(host):
        src = [a.ctypes.data if host else t.data_ptr() for a, t in zip(hsrc, dsrc)]
        yb = [a.ctypes.data if host else t.data_ptr() for a, t in zip(hyuv, dyuv)]
        dst = [a.ctypes.data if host else t.data_ptr() for a, t in zip(hdst, ddst)]
        return src, yb, dst

    def call(host, kind, code, crop=(0, 0, 6, 6), size=(3, 3), edit=None):
        src, yb, dst = ptrs(host)
        if edit:
            edit(src, dst)
        tail = "" if host else "_device"
        yuv = (arr(yb), arr([b + w * h for b in yb]), arr([b + w * h + cw2 * ch2 for b in yb]), w, h, w, cw2, 1, 0)
        if kind == "orient":
            rc = getattr(L, "nq_orient_frames" + tail)(hd._h, n, arr(src), w, h, code, arr(dst))
        elif kind == "yuv":
            rc = getattr(L, "nq_frames_from_yuv_oriented" + tail)(hd._h, n, *yuv, code, arr(dst))
        elif kind == "reduce":
            rc = getattr(L, "nq_resample_frames_oriented" + tail)(hd._h, n, arr(src), w, h, code, *crop, arr(dst), *size, 1)
        else:
            rc = getattr(L, "nq_resample_frames_yuv_oriented" + tail)(hd._h, n, *yuv, code, *crop, arr(dst), *size, 1)
        torch.cuda.synchronize()
        return rc

    def state(host):
        if host:
            return [a.copy() for a in hsrc + hyuv + hdst]
        return [x.cpu().numpy().copy() for x in dsrc + dyuv + ddst]

    def reset(host):
        for a in hdst: a[:] = -9
        if not host:
            for d, a in zip(ddst, hdst): d.copy_(torch.from_numpy(a))

    def valid(host, kind, code, crop, size):
        want = {"orient": lambda: O.orient_all(argb, code), "yuv": lambda: O.orient_all(full, code),
                "reduce": lambda: O.resample_oriented(argb, code, size, crop), "yuv_reduce": lambda: R.resample(O.orient_all(full, code), size, crop)}[kind]()
        assert call(host, kind, code, crop, size) == 0, (host, kind, code)
        got = state(host)[-n:]
        px = want[0].size
        for k in range(n):
            assert (got[k][:px] == want[k].reshape(-1)).all() and (got[k][px:] == -9).all(), (host, kind, code)
        reset(host)

    def in_place(src, dst): dst[0] = src[0]
    def into_source(src, dst): dst[1] = src[0] + 4 * 5
    def same_output(src, dst): dst[1] = dst[0] + 4 * 7

    wide, tall = (6, 0, 6, 6), (0, 6, 6, 6)                       # each fits one of 12 x 6 and 6 x 12 only
    for host in (True, False):
        reset(host)
        for kind in ("orient", "yuv", "reduce", "yuv_reduce"):
            reducing = kind in ("reduce", "yuv_reduce")
            for code in (6, 2):
                fits, leaves = (tall, wide) if code >= 5 else (wide, tall)
                valid(host, kind, code, fits, (3, 3))
                bad = [dict(code=0), dict(code=9), dict(code=-1), dict(code=code, edit=same_output)]
                if kind in ("orient", "reduce"):
                    bad += [dict(code=code, edit=in_place), dict(code=code, edit=into_source)]
                if reducing:
                    bad += [dict(code=code, crop=leaves), dict(code=code, crop=fits, size=(7, 3)), dict(code=code, crop=fits, size=(3, 7)),
                            dict(code=code, crop=(-1, 0, 3, 3)), dict(code=code, crop=fits, size=(0, 3))]
                for kw in bad:
                    before = state(host)
                    assert call(host, kind, **kw) == -1, (host, kind, kw)
                    assert (L.nq_last_error(hd._h) or b"") != b""
                    assert all((a == b).all() for a, b in zip(before, state(host))), (host, kind, kw)
                valid(host, kind, code, fits, (6, 3) if reducing else (3, 3))


# ---- the converters ----
W, H, N, K = 24, 16, 3, 16


@pytest.fixture(scope="module")
def clip(nq):
    from nquant.android_amd import synth
    frames = [nq.yuv_planes(synth.yuv420(W, H, 90 + i, "nv12"), W, H, "nv12") for i in range(N)]
    return frames, nq.frames_from_yuv(frames, bt709=True)


def test_convert_frames_to_gif_with_orient(nq, clip):
    frames, full = clip
    yuv = {"bt709": True}
    turned = nq.orient_frames(full, 6)
    assert all(t.shape == (W, H) and (t == r).all() for t, r in zip(turned, O.orient_all(full, 6)))
    # YUV frames, reduced: the same converter on frames converted and oriented beforehand
    want, wpal = nq.convert_frames_to_gif(1, turned, K, True, size=(8, 12))
    got, gpal = nq.convert_frames_to_gif(1, frames, K, True, size=(8, 12), yuv=yuv, orient=6)
    assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all()
    # ... at full size, and from ARGB frames
    want, wpal = nq.convert_frames_to_gif(1, turned, K, True)
    for src, kw in ((frames, {"yuv": yuv}), (full, {})):
        got, gpal = nq.convert_frames_to_gif(1, src, K, True, orient=6, **kw)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all()
    assert got[6:10] == bytes([H, 0, W, 0])                       # the logical screen is H wide and W tall
    # orient=1 is the call without the keyword
    for src, kw in ((frames, {"yuv": yuv}), (frames, {"yuv": yuv, "size": (12, 8)}), (full, {}), (full, {"crop": (2, 2, 20, 12)})):
        a, apal = nq.convert_frames_to_gif(1, src, K, True, **kw)
        b, bpal = nq.convert_frames_to_gif(1, src, K, True, orient=1, **kw)
        assert a == b and (np.asarray(apal) == np.asarray(bpal)).all(), kw


def test_the_other_converters_with_orient(nq, clip):
    frames, full = clip
    yuv = {"bt709": True}
    turned = nq.orient_frames(full, 8)
    small = nq.resample_frames(turned, (8, 12))
    want = nq.convert_frames_to_apng(1, small, K, True)
    got = nq.convert_frames_to_apng(1, frames, K, True, size=(8, 12), yuv=yuv, orient=8)
    assert got[0] == want[0] and (np.asarray(got[1]) == np.asarray(want[1])).all()
    want = nq.convert_shots_to_gif(1, small, [0, 2], K, True)
    got = nq.convert_shots_to_gif(1, full, [0, 2], K, True, size=(8, 12), orient=8)
    assert got[0] == want[0] and all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got[1], want[1]))
    want = nq.convert_clip_to_gif(1, turned, K, True, min_shot=2)
    got = nq.convert_clip_to_gif(1, frames, K, True, min_shot=2, yuv=yuv, orient=8)
    assert got[0] == want[0] and got[2] == want[2]
    for convert, args in ((nq.convert_frames_refined, (K, True, 2)), (nq.convert_frames_ordered, (K, 8))):
        wpal, wouts = convert(1, small, *args)
        gpal, gouts = convert(1, frames, *args, size=(8, 12), yuv=yuv, orient=8)
        assert (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
        assert all((a.index == b.index).all() and (a.argb == b.argb).all() for a, b in zip(gouts, wouts)), convert.__name__
