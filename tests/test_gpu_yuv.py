"""YUV input on the GPU (nq_frames_from_yuv* / nq_resample_frames_yuv*): the 1:1 conversion and the fused conversion + reduction equal the
restatement in yuv_ref.py word for word -- for the four flag words, I420 (tight and with padded strides), NV12, NV21 and two unrelated
planes of element step 2, with plane pointers on a 16-byte boundary and one byte behind it, outputs on a 16-byte boundary and one word
behind it, at the smallest shapes that reach each path (one pixel, odd sides, an odd last row, widths that are and are not multiples
of 4, more items than the grid holds, footprints longer than a chunk), with crops of every parity; the fused call equals the two
calls it is defined by; the sources and the guard words around every output stay untouched; the host forms equal the device forms;
every rejected argument leaves the buffers alone and the handle usable; and the converters' yuv= equals the converter on the
converted frames."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_ref as Y
from conftest import ROOT
from nquant.android_amd import gif as G

pytestmark = pytest.mark.gpu

GUARD = 24                                                     # elements between two outputs of a buffer (a multiple of 8)
FLAG_WORDS = (0, Y.BT709, Y.FULL_RANGE, Y.BT709 | Y.FULL_RANGE)
LAYOUTS = ("i420", "i420pad4", "i420pad5", "nv12", "nv21", "split2")
FILL = 0xA5                                                    # the bytes between and around the planes


def _constant(name):
    src = open(os.path.join(ROOT, "nquant.android_amd", "csrc", "nq_yuv.hip")).read()
    return int(re.search(r"constexpr (?:int|long long) %s = (\d+);" % name, src).group(1))


YUV_THREADS, YUV_MAX_BLOCKS, YR_MAX_BLOCKS = _constant("YUV_THREADS"), _constant("YUV_MAX_BLOCKS"), _constant("YR_MAX_BLOCKS")


def _kw(flags):
    return {"bt709": bool(flags & Y.BT709), "full_range": bool(flags & Y.FULL_RANGE)}


class _Planes:
    """The planes of n frames (tight (y, u, v) arrays of one size) in ONE device byte buffer in `layout`, every plane `shift` bytes
    behind a 16-byte boundary, FILL bytes everywhere else:
      i420      tight planes                 i420pad4  y_stride = w + 4, c_stride = cw2 + 2 (the wide path keeps its alignment)
      i420pad5  y_stride = w + 5, c_stride = cw2 + 3 (odd strides: the byte path)
      nv12      u, v interleaved, u first    nv21      v first
      split2    element step 2, u and v in buffers of their own (the bytes in between belong to neither)"""

    def __init__(self, frames, layout, shift):
        import torch
        h, w = frames[0][0].shape
        ch2, cw2 = (h + 1) // 2, (w + 1) // 2
        self.w, self.h = w, h
        self.y_stride = {"i420pad4": w + 4, "i420pad5": w + 5}.get(layout, w)
        self.c_step = 1 if layout.startswith("i420") else 2
        self.c_stride = {"i420": cw2, "i420pad4": cw2 + 2, "i420pad5": cw2 + 3}.get(layout, 2 * cw2)
        yspan = (h - 1) * self.y_stride + w
        cspan = (ch2 - 1) * self.c_stride + (cw2 - 1) * self.c_step + 1
        room = lambda nbytes: (nbytes + 15) // 16 * 16 + 32
        pos, places = 32, []
        for _ in frames:
            py = pos + shift
            pos += room(yspan)
            if layout in ("nv12", "nv21"):
                lo = pos + shift
                pos += room(cspan + 1)
                pu, pv = (lo, lo + 1) if layout == "nv12" else (lo + 1, lo)
            else:
                pu = pos + shift
                pos += room(cspan)
                pv = pos + shift
                pos += room(cspan)
            places.append((py, pu, pv))
        self.host = np.full(pos + 32, FILL, np.uint8)
        for (py, pu, pv), (y, u, v) in zip(places, frames):
            for off, plane, stride, step in ((py, y, self.y_stride, 1), (pu, u, self.c_stride, self.c_step), (pv, v, self.c_stride, self.c_step)):
                np.lib.stride_tricks.as_strided(self.host[off:], plane.shape, (stride, step))[...] = plane
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        base = self.dev.data_ptr()
        self.y, self.u, self.v = ([base + p[k] for p in places] for k in range(3))
        self.places = places

    def views(self, buf):
        """The (y, u, v) strided views of every frame in a host copy of the buffer."""
        ch2, cw2 = (self.h + 1) // 2, (self.w + 1) // 2
        view = lambda off, shape, stride, step: np.lib.stride_tricks.as_strided(buf[off:], shape, (stride, step))
        return [(view(py, (self.h, self.w), self.y_stride, 1), view(pu, (ch2, cw2), self.c_stride, self.c_step),
                 view(pv, (ch2, cw2), self.c_stride, self.c_step)) for py, pu, pv in self.places]

    def geometry(self):
        return self.w, self.h, self.y_stride, self.c_stride, self.c_step

    def read(self):
        return self.dev.cpu().numpy()


class _Stream:
    """n int32 arrays of one size in ONE device buffer, guard elements before, between and after them; array i starts `shift`
    elements behind a 16-byte boundary."""

    def __init__(self, arrays, shift, sentinel):
        import torch
        px = arrays[0].size
        pitch = (px + 7) // 8 * 8 + GUARD
        self.offs = [GUARD + i * pitch + shift for i in range(len(arrays))]
        self.px = px
        self.host = np.full(GUARD + len(arrays) * pitch + 8, sentinel, np.int32)
        self.fill(self.host, arrays)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = [self.dev.data_ptr() + 4 * o for o in self.offs]

    def fill(self, buf, arrays):
        for a, o in zip(arrays, self.offs):
            buf[o:o + self.px] = np.asarray(a).reshape(-1)

    def expect(self, arrays):
        want = self.host.copy()
        self.fill(want, arrays)
        return want

    def read(self):
        return self.dev.cpu().numpy()


_REF = {}


def _frames(w, h, n):
    key = ("frames", w, h, n)
    if key not in _REF:
        _REF[key] = [Y.random_planes(w, h, 1000 * w + 10 * h + i) for i in range(n)]
    return _REF[key]


def _converted(w, h, n, flags):
    """(frames, their conversion by the restatement), computed once."""
    key = ("1:1", w, h, n, flags)
    if key not in _REF:
        _REF[key] = Y.convert(_frames(w, h, n), flags)
    return _frames(w, h, n), _REF[key]


def _reduced(w, h, n, flags, size, crop, linear):
    key = ("fused", w, h, n, flags, size, crop, linear)
    if key not in _REF:
        _REF[key] = Y.resample_ref.resample(_converted(w, h, n, flags)[1], size, crop, Y.LINEAR if linear else 0)
    return _frames(w, h, n), _REF[key]


def _device_case(nq, q, frames, want, layout, flags, pshift, oshift, size=None, crop=None, linear=True, fused=False):
    import torch
    src = _Planes(frames, layout, pshift)
    dst = _Stream([np.full(r.shape, -9, np.int32) for r in want], oshift, -9)
    why = (frames[0][0].shape, len(frames), layout, flags, pshift, oshift, size, crop, linear)
    assert all(p % 16 == pshift for p in src.y) and all(p % 16 == 4 * oshift for p in dst.ptrs), why
    torch.cuda.synchronize()
    if fused:
        nq.resample_frames_yuv_device(q, src.y, src.u, src.v, *src.geometry(), dst.ptrs, size, crop, linear, **_kw(flags))
    else:
        nq.frames_from_yuv_device(q, src.y, src.u, src.v, *src.geometry(), dst.ptrs, **_kw(flags))
    torch.cuda.synchronize()
    got = dst.read()
    assert (got == dst.expect(want)).all(), (why, int((got != dst.expect(want)).sum()))          # the whole buffer: guards included
    assert (src.read() == src.host).all(), why


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


SIZES = [(1, 1), (2, 2), (3, 3), (5, 2), (7, 3), (8, 4), (12, 5), (64, 6)]
SHIFTS = ((0, 0), (1, 0), (0, 1))                              # (plane pointers, outputs): aligned; planes one byte on; outputs one word on


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_conversion_equals_the_restatement_in_every_layout(nq, q, size):
    """Widths 8, 12 and 64 take the wide paths when planes and outputs are aligned (i420, i420pad4: planar; nv12, nv21:
    interleaved; 12 x 5 ends in an odd row), and the byte path when a pointer is shifted, with odd strides (i420pad5) and with two
    unrelated planes of step 2 (split2); every other width takes the byte path."""
    w, h = size
    for n in (1, 2, 5):
        for flags in FLAG_WORDS:
            frames, want = _converted(w, h, n, flags)
            assert all(r.shape == (h, w) and (r.view(np.uint32) >> 24 == 255).all() for r in want)
            for layout in LAYOUTS:
                for pshift, oshift in SHIFTS:
                    _device_case(nq, q, frames, want, layout, flags, pshift, oshift)


def test_conversion_of_more_items_than_the_grid_holds(nq, q):
    """The grid is capped at YUV_MAX_BLOCKS workgroups of YUV_THREADS items, which then stride over the rest.  Byte path (an item is a
    pixel): 2 frames of 513 x 512.  Wide paths (an item is 4 x 2 pixels): 2 frames of 2052 x 1024."""
    cap = YUV_MAX_BLOCKS * YUV_THREADS
    assert cap == 2048 * 256
    for (w, h), layouts in (((513, 512), ("i420", "nv12")), ((2052, 1024), ("nv12", "i420"))):
        items = 2 * w * h if w % 4 else 2 * (w // 4) * (h // 2)
        assert cap < items < cap + cap // 256
        frames, want = _converted(w, h, 2, Y.BT709)
        for layout in layouts:
            _device_case(nq, q, frames, want, layout, Y.BT709, 0, 0)


# (source width, height) -> (target width, height); 4100 x 2 is 4099 x 2 on the wide paths: five chunks of 1024 columns
SHAPES = [((1, 1), (1, 1)), ((2, 1), (1, 1)), ((7, 3), (7, 3)), ((8, 8), (4, 4)), ((13, 9), (5, 4)), ((67, 5), (3, 5)),
          ((256, 64), (100, 7)), ((4099, 2), (1, 1)), ((4100, 2), (1, 1)), ((2, 2050), (1, 1))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_fused_call_equals_the_restatement(nq, q, shape):
    (w, h), size = shape
    for linear in (True, False):
        for flags in (0, Y.BT709 | Y.FULL_RANGE):
            frames, want = _reduced(w, h, 2, flags, size, None, linear)
            assert all(r.shape == (size[1], size[0]) for r in want)
            for layout in ("nv12", "i420"):
                for pshift, oshift in ((0, 0), (1, 1)):
                    _device_case(nq, q, frames, want, layout, flags, pshift, oshift, size, None, linear, fused=True)


def test_fused_call_with_more_work_items_than_the_grid_holds(nq, q):
    """A work item is (frame, output row, block of output columns) and the grid is capped at YR_MAX_BLOCKS workgroups: 5 frames of
    YR_MAX_BLOCKS / 5 + 60 rows.  Width 8: the wide paths; width 5: the byte path."""
    rows = YR_MAX_BLOCKS // 5 + 60
    assert 5 * rows > YR_MAX_BLOCKS == 8192
    for w, size, layout in ((8, (3, rows), "nv12"), (8, (2, rows - 1), "i420"), (5, (3, rows), "nv12")):
        frames, want = _reduced(w, rows, 5, Y.BT709, size, None, True)
        _device_case(nq, q, frames, want, layout, Y.BT709, 0, 0, size, None, True, fused=True)


# crop_x, crop_y of every parity: the chroma of crop pixel (j, i) is the frame's sample ((crop_x + j) >> 1, (crop_y + i) >> 1)
CROPS = [((13, 9), (cx, cy, 8, 6), (3, 4)) for cx in (2, 3) for cy in (0, 1)] + \
        [((256, 64), (cx, cy, 200, 50), (77, 13)) for cx in (4, 5) for cy in (2, 3)] + \
        [((256, 64), (255, 63, 1, 1), None), ((13, 9), (1, 1, 12, 8), (12, 8))]


@pytest.mark.parametrize("case", CROPS, ids=lambda c: "%dx%d-crop%d-%d" % (c[0][0], c[0][1], c[1][0], c[1][1]))
def test_fused_crops_of_every_parity(nq, q, case):
    (w, h), crop, size = case
    for linear in (True, False):
        frames, want = _reduced(w, h, 2, Y.FULL_RANGE, size, crop, linear)
        for layout in ("nv12", "nv21", "i420", "split2"):
            for pshift, oshift in ((0, 0), (1, 1)):
                _device_case(nq, q, frames, want, layout, Y.FULL_RANGE, pshift, oshift, size, crop, linear, fused=True)


def test_fused_call_equals_the_two_calls_it_is_defined_by(nq, q):
    import torch
    for (w, h), size, crop in (((256, 64), (100, 7), None), ((13, 9), (5, 4), (3, 1, 9, 7)), ((64, 6), (64, 6), None)):
        frames = _frames(w, h, 2)
        for layout in ("nv12", "i420", "i420pad5"):
            for linear in (True, False):
                src = _Planes(frames, layout, 0)
                full = _Stream([np.zeros((h, w), np.int32)] * 2, 0, -7)
                two = _Stream([np.zeros((size[1], size[0]), np.int32)] * 2, 0, -9)
                one = _Stream([np.zeros((size[1], size[0]), np.int32)] * 2, 0, -9)
                nq.frames_from_yuv_device(q, src.y, src.u, src.v, *src.geometry(), full.ptrs, bt709=True)
                nq.resample_frames_device(q, full.ptrs, w, h, two.ptrs, size, crop, linear)
                nq.resample_frames_yuv_device(q, src.y, src.u, src.v, *src.geometry(), one.ptrs, size, crop, linear, bt709=True)
                torch.cuda.synchronize()
                assert (one.read() == two.read()).all(), (w, h, layout, linear)
                assert (one.read() != -9).sum() == 2 * size[0] * size[1]


@pytest.mark.parametrize("layout", ["nv12", "nv21", "i420", "yv12"])
def test_host_forms_equal_the_device_forms(nq, layout):
    """... on strided views of one buffer per frame (yuv_planes), which are passed as they are, and on tight planes."""
    from nquant.android_amd import synth
    for (w, h), size, crop in (((12, 5), (5, 2), None), ((13, 9), (5, 4), (3, 1, 9, 7)), ((64, 6), (16, 3), None)):
        bufs = [synth.yuv420(w, h, 70 + i, layout) for i in range(3)]
        keep = [b.copy() for b in bufs]
        views = [nq.yuv_planes(b, w, h, layout) for b in bufs]
        tight = [tuple(np.ascontiguousarray(p) for p in f) for f in views]
        for flags in (0, Y.BT709 | Y.FULL_RANGE):
            want = Y.convert(tight, flags)                                                  # (what the device form gave above)
            for frames in (views, tight):
                got = nq.frames_from_yuv(frames, **_kw(flags))
                assert len(got) == 3 and all(g.dtype == np.int32 and (g == r).all() for g, r in zip(got, want)), (w, h, layout, flags)
            for linear in (True, False):
                small = Y.resample_ref.resample(want, size, crop, Y.LINEAR if linear else 0)
                for frames in (views, tight):
                    got = nq.resample_frames_yuv(frames, size, crop=crop, linear=linear, **_kw(flags))
                    assert all((g == r).all() for g, r in zip(got, small)), (w, h, layout, flags, linear)
        assert all((a == b).all() for a, b in zip(bufs, keep))
    # size=None and crop=None: the fused call at the frame's own size is the conversion
    assert all((a == b).all() for a, b in zip(nq.resample_frames_yuv(views, None), Y.convert(tight, 0)))


def _arranged(frames, arrangement):
    """The tight frames with their chroma planes as one of the four arrangements the host forms' staging tells apart."""
    out = []
    for y, u, v in frames:
        if arrangement in ("interleaved-uv", "interleaved-vu"):        # one span: the second plane begins one sample into the first
            c = np.stack((u, v) if arrangement == "interleaved-uv" else (v, u), axis=2)
            u, v = (c[:, :, 0], c[:, :, 1]) if arrangement == "interleaved-uv" else (c[:, :, 1], c[:, :, 0])
        elif arrangement == "planar-touching":                        # one span: v begins where u's span ends
            c = np.concatenate([u.ravel(), v.ravel()])
            u, v = c[:u.size].reshape(u.shape), c[u.size:].reshape(v.shape)
        else:                                                          # three allocations: two chroma spans
            u, v = u.copy(), v.copy()
        out.append((y.copy(), u, v))
    return out


@pytest.mark.parametrize("shape", [((8, 4), (4, 2)), ((5, 3), (2, 1))], ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
@pytest.mark.parametrize("arrangement", ["interleaved-uv", "interleaved-vu", "planar-touching", "separate"])
def test_host_forms_in_every_arrangement_of_the_planes(nq, arrangement, shape):
    """The staging of the host forms keeps what the kernels' paths need of each arrangement: 8 x 4 is eligible for the wide paths
    (interleaved with either plane first, planar), 5 x 3 takes the byte path.  1:1 and reducing, against the restatement."""
    (w, h), size = shape
    flags = Y.BT709
    frames, want = _converted(w, h, 3, flags)
    planes = _arranged(frames, arrangement)
    keep = [tuple(p.copy() for p in f) for f in planes]
    got = nq.frames_from_yuv(planes, **_kw(flags))
    assert len(got) == 3 and all((g == r).all() for g, r in zip(got, want)), (arrangement, shape)
    for linear in (True, False):
        small = _reduced(w, h, 3, flags, size, None, linear)[1]
        got = nq.resample_frames_yuv(planes, size, linear=linear, **_kw(flags))
        assert len(got) == 3 and all(g.shape == (size[1], size[0]) and (g == r).all() for g, r in zip(got, small)), (arrangement, shape, linear)
    assert all((a == b).all() for f, k in zip(planes, keep) for a, b in zip(f, k))


def test_invalid_arguments_then_a_valid_call(nq, hd):
    import torch
    L = hd._L
    w, h, n = 12, 8, 3
    cw2, ch2 = 6, 4
    geo = dict(cx=1, cy=2, cw=9, ch=5, dw=4, dh=3)
    frames = _frames(w, h, n)
    want = {False: Y.convert(frames, Y.BT709), True: Y.resample_ref.resample(Y.convert(frames, Y.BT709), (4, 3), (1, 2, 9, 5), Y.LINEAR)}
    # NV12 buffers with room behind the data; the outputs start as -9 and have room for a shifted pointer
    hs = [np.concatenate([y.reshape(-1), np.stack([u, v], -1).reshape(-1), np.zeros(16, np.uint8)]) for y, u, v in frames]
    ho = [np.full(w * h + 2, -9, np.int32) for _ in frames]
    ds = [torch.from_numpy(a).cuda() for a in hs]
    do = [torch.from_numpy(a).cuda() for a in ho]

    def ptrs(host):
        base = [a.ctypes.data if host else t.data_ptr() for a, t in zip(hs, ds)]
        return {"y": list(base), "u": [b + w * h for b in base], "v": [b + w * h + 1 for b in base],
                "dst": [a.ctypes.data if host else t.data_ptr() for a, t in zip(ho, do)]}

    def call(host, fused, n=n, w=w, h=h, ys=w, cs=2 * cw2, step=2, yflags=Y.BT709, flags=1, edit=None, null=None, **kw):
        g = dict(geo, **kw)
        p = ptrs(host)
        if edit:
            edit(p)
        arr = lambda v: (C.c_void_p * len(v))(*v)
        a = {k: (None if k == null else arr(v)) for k, v in p.items()}
        name = ("nq_resample_frames_yuv" if fused else "nq_frames_from_yuv") + ("" if host else "_device")
        head = (hd._h, n, a["y"], a["u"], a["v"], w, h, ys, cs, step, yflags)
        if fused:
            rc = getattr(L, name)(*head, g["cx"], g["cy"], g["cw"], g["ch"], a["dst"], g["dw"], g["dh"], flags)
        else:
            rc = getattr(L, name)(*head, a["dst"])
        torch.cuda.synchronize()
        return rc

    def state(host):
        if host:
            return [a.copy() for a in hs + ho]
        return [x.cpu().numpy().copy() for x in ds + do]

    def valid(host, fused):
        """A valid call gives the reference; then the outputs are put back to -9 for the rejected calls that follow."""
        assert call(host, fused) == 0
        got = state(host)
        px = want[fused][0].size
        for k in range(n):
            assert (got[n + k][:px] == want[fused][k].reshape(-1)).all() and (got[n + k][px:] == -9).all() and (got[k] == hs[k]).all()
        for a in ho: a[:] = -9
        if not host:
            for d, a in zip(do, ho): d.copy_(torch.from_numpy(a))

    def null_entry(key):
        def edit(p): p[key][1] = None
        return edit

    def off_by(key, nbytes):
        def edit(p): p[key][2] += nbytes
        return edit

    def into(key, nbytes):          # output 1 begins inside a plane of frame 0 (4-byte aligned: the frames' buffers are)
        def edit(p): p["dst"][1] = p[key][0] // 4 * 4 + nbytes
        return edit

    def same_output(p):             # outputs 0 and 2 overlap by one word
        p["dst"][2] = p["dst"][0] + 4 * 11

    both = [{"n": 0}, {"n": -2}, {"w": 0}, {"w": 65536}, {"h": 0}, {"h": 65536}, {"ys": w - 1}, {"ys": 0}, {"ys": -w}, {"step": 0}, {"step": 3},
            {"step": -1}, {"cs": 2 * (cw2 - 1)}, {"cs": 0}, {"step": 1, "cs": cw2 - 1}, {"yflags": 4}, {"yflags": 7}, {"yflags": -1},
            {"null": "y"}, {"null": "u"}, {"null": "v"}, {"null": "dst"},
            {"edit": null_entry("y")}, {"edit": null_entry("u")}, {"edit": null_entry("v")}, {"edit": null_entry("dst")},
            {"edit": off_by("dst", 2)}, {"edit": off_by("dst", 1)}, {"edit": off_by("dst", 3)},
            {"n": 2, "w": 32768, "h": 32768, "ys": 32768, "cs": 32768},                    # 2^31 pixels: one more than the limit
            {"edit": into("y", 8)}, {"edit": into("y", 4 * ((w * h - 1) // 4))}, {"edit": into("u", 4)},
            {"edit": into("v", 4 * ((2 * cw2 * ch2 - 1) // 4))}, {"edit": same_output}]
    fused_only = [{"cw": 0}, {"ch": 0}, {"cx": -1}, {"cy": -1}, {"cx": 4}, {"cy": 4}, {"cw": 12, "dw": 4}, {"ch": 7},   # empty / leaves the frame
                  {"dw": 0}, {"dh": 0}, {"dw": 10}, {"dh": 6}, {"dw": -1},                                             # target < 1 / larger than the crop
                  {"flags": 2}, {"flags": 3}, {"flags": -1}]
    for host in (True, False):
        for fused in (False, True):
            valid(host, fused)
            for kw in both + (fused_only if fused else []):
                before = state(host)
                rc = call(host, fused, **kw)
                assert rc == -1, (host, fused, kw)
                assert (L.nq_last_error(hd._h) or b"") != b""
                assert all((a == b).all() for a, b in zip(before, state(host))), (host, fused, kw)
            valid(host, fused)
            # the same planes for every frame are allowed: sources are only read
            def one_source(p):
                for k in ("y", "u", "v"): p[k][1] = p[k][2] = p[k][0]
            assert call(host, fused, edit=one_source) == 0
            got = state(host)
            px = want[fused][0].size
            assert all((got[n + k][:px] == want[fused][0].reshape(-1)).all() for k in range(n))
            valid(host, fused)


# ---- the converters: yuv= equals the converter on the converted (and reduced) frames ----
W, H, N, K = 24, 16, 3, 16


@pytest.fixture(scope="module")
def clip(nq):
    from nquant.android_amd import synth
    frames = [nq.yuv_planes(synth.yuv420(W, H, 90 + i, "nv12"), W, H, "nv12") for i in range(N)]
    return frames, nq.frames_from_yuv(frames, bt709=True), nq.resample_frames_yuv(frames, (12, 8), bt709=True)


def test_convert_frames_to_gif_and_apng_from_yuv(nq, clip):
    frames, full, small = clip
    assert all(f.shape == (H, W) for f in full) and all(s.shape == (8, 12) for s in small)
    assert all((a == b).all() for a, b in zip(full, Y.convert(frames, Y.BT709)))
    yuv = {"bt709": True}
    for convert in (nq.convert_frames_to_gif, nq.convert_frames_to_apng):
        want, wpal = convert(1, full, K, True)
        got, gpal = convert(1, frames, K, True, yuv=yuv)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
        want, wpal = convert(1, small, K, True)
        got, gpal = convert(1, frames, K, True, size=(12, 8), yuv=yuv)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
    # the other flag word gives other colours: the keyword reaches the kernel
    assert any((a != b).any() for a, b in zip(full, nq.frames_from_yuv(frames)))


def test_the_other_converters_from_yuv(nq, clip):
    frames, full, small = clip
    yuv = {"bt709": True}
    want = nq.convert_shots_to_gif(1, small, [0, 2], K, True)
    got = nq.convert_shots_to_gif(1, frames, [0, 2], K, True, size=(12, 8), yuv=yuv)
    assert got[0] == want[0] and all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got[1], want[1]))
    want = nq.convert_clip_to_gif(1, full, K, True, min_shot=2)
    got = nq.convert_clip_to_gif(1, frames, K, True, min_shot=2, yuv=yuv)
    assert got[0] == want[0] and got[2] == want[2]
    for convert, args in ((nq.convert_frames_refined, (K, True, 2)), (nq.convert_frames_ordered, (K, 8))):
        wpal, wouts = convert(1, small, *args)
        gpal, gouts = convert(1, frames, *args, size=(12, 8), yuv=yuv)
        assert (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
        assert all((a.index == b.index).all() and (a.argb == b.argb).all() for a, b in zip(gouts, wouts)), convert.__name__
