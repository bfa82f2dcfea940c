"""10-bit YUV input on the GPU (nq_frames_from_yuv16* / nq_resample_frames_yuv16*): the 1:1 conversion and the fused conversion +
reduction equal the restatement in yuv16_ref.py word for word -- the grid frame (every Y, the corners of the chroma square) in SDR, PQ
and HLG, limited and full range; samples in the high and in the low ten bits with junk in the other six; the four layouts with row
strides longer than the rows and poisoned padding, plane pointers on a 16-byte boundary and one sample behind it (the wide paths and
the one-pixel path on the same data), at the smallest shapes that reach each path, one item past a strip, more strips than the grid
holds and one frame past a launch group; crops of every parity; the fused call equals the two calls it is defined by; a caller's
stream and the NULL stream; the host forms equal the device forms and leave the library's device memory as it was; every rejected
argument leaves the buffers alone and is followed by a valid call; and the converters' yuv16= equals the converter on the converted
frames.  Guard words follow every output."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_ref
import yuv16_ref as Y
from conftest import ROOT

pytestmark = pytest.mark.gpu

GUARD = 24                                                     # words between two outputs of a buffer (a multiple of 8)
FILL = 0xA5A5                                                  # the words between and around the planes
LAYOUTS = ("p010", "p010_vu", "i010", "yv12_10")
SDR709, PQ2020, HLG2020F = Y.BT709 | Y.MSB, Y.BT2020 | Y.PQ | Y.MSB, Y.BT2020 | Y.HLG | Y.FULL_RANGE     # the last reads the LOW ten bits
MODES = (SDR709, PQ2020, HLG2020F)


def _constant(name):
    src = open(os.path.join(ROOT, "nquant.android_amd", "csrc", "nq_yuv16.hip")).read()
    m = re.search(r"constexpr (?:int|long long) %s = ([^;]+);" % name, src).group(1)
    return int(eval(m, {"Y16_THREADS": 256, "YR16_THREADS": 256}))


Y16_STRIP, Y16_MAX_BLOCKS, YR16_MAX_BLOCKS = _constant("Y16_STRIP"), _constant("Y16_MAX_BLOCKS"), _constant("YR16_MAX_BLOCKS")


def _kw(flags):
    return {"matrix": "bt2020" if flags & Y.BT2020 else "bt709" if flags & Y.BT709 else "bt601", "full_range": bool(flags & Y.FULL_RANGE),
            "transfer": "pq" if flags & Y.PQ else "hlg" if flags & Y.HLG else "sdr", "msb": bool(flags & Y.MSB)}


class _Planes:
    """The planes of n frames (tight (y, u, v) uint16 arrays of one size) in ONE device buffer of 16-bit words in `layout`, every plane
    `shift` samples behind a 16-byte boundary, FILL words everywhere else.  Rows are longer than their samples: y_stride = w + 4,
    c_stride = 2 cw2 + 4 (interleaved) or cw2 + 2 (planar), so the wide paths keep their alignment where the width allows them.
      p010     u, v interleaved, u first     p010_vu   v first
      i010     the u plane, then v's         yv12_10   the v plane, then u's
    `share`: every frame uses the planes of frame 0 (sources are only read)."""

    def __init__(self, frames, layout, shift, share=False):
        import torch
        h, w = frames[0][0].shape
        ch2, cw2 = (h + 1) // 2, (w + 1) // 2
        inter = layout in ("p010", "p010_vu")
        self.w, self.h = w, h
        self.y_stride, self.c_step = w + 4, 2 if inter else 1
        self.c_stride = 2 * cw2 + 4 if inter else cw2 + 2
        yspan = (h - 1) * self.y_stride + w
        cspan = (ch2 - 1) * self.c_stride + (cw2 - 1) * self.c_step + 1
        room = lambda words: (words + 7) // 8 * 8 + 16
        pos, places = 16, []
        for _ in (frames[:1] if share else frames):
            py = pos + shift
            pos += room(yspan)
            if inter:
                lo = pos + shift
                pos += room(cspan + 1)
                pu, pv = (lo, lo + 1) if layout == "p010" else (lo + 1, lo)
            else:
                a = pos + shift
                pos += room(cspan)
                b = pos + shift
                pos += room(cspan)
                pu, pv = (a, b) if layout == "i010" else (b, a)
            places.append((py, pu, pv))
        if share:
            places = places * len(frames)
        self.host = np.full(pos + 16, FILL, np.uint16)
        for (py, pu, pv), (y, u, v) in zip(places, frames):
            for off, plane, stride, step in ((py, y, self.y_stride, 1), (pu, u, self.c_stride, self.c_step), (pv, v, self.c_stride, self.c_step)):
                np.lib.stride_tricks.as_strided(self.host[off:], plane.shape, (2 * stride, 2 * step))[...] = plane
        self.dev = torch.from_numpy(self.host.view(np.int16).copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        base = self.dev.data_ptr()
        self.y, self.u, self.v = ([base + 2 * p[k] for p in places] for k in range(3))
        self.places = places

    def geometry(self):
        return self.w, self.h, self.y_stride, self.c_stride, self.c_step

    def read(self):
        return self.dev.cpu().numpy().view(np.uint16)


class _Stream:
    """n int32 arrays of one size in ONE device buffer, guard words before, between and after them; array i starts `shift` words
    behind a 16-byte boundary."""

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


def _frames(w, h, n, flags):
    """n frames of random samples where the flag word reads them, random junk in the other six bits; computed once."""
    key = ("frames", w, h, n, flags & Y.MSB)
    if key not in _REF:
        _REF[key] = [Y.random_planes(w, h, 1000 * w + 10 * h + i, flags) for i in range(n)]
    return _REF[key]


def _converted(w, h, n, flags):
    """(frames, their conversion by the restatement), computed once and left unchanged."""
    key = ("1:1", w, h, n, flags)
    if key not in _REF:
        _REF[key] = Y.convert(_frames(w, h, n, flags), flags)
    return _frames(w, h, n, flags), _REF[key]


def _reduced(w, h, n, flags, size, crop, linear):
    key = ("fused", w, h, n, flags, size, crop, linear)
    if key not in _REF:
        _REF[key] = resample_ref.resample(_converted(w, h, n, flags)[1], size, crop, Y.LINEAR if linear else 0)
    return _frames(w, h, n, flags), _REF[key]


def _device_case(nq, frames, want, layout, flags, pshift, oshift, size=None, crop=None, linear=True, fused=False, share=False, stream=0):
    import torch
    src = _Planes(frames, layout, pshift, share)
    dst = _Stream([np.full(r.shape, -9, np.int32) for r in want], oshift, -9)
    why = (frames[0][0].shape, len(frames), layout, flags, pshift, oshift, size, crop, linear)
    assert all(p % 16 == 2 * pshift for p in src.y) and all(p % 16 == 4 * oshift for p in dst.ptrs), why
    torch.cuda.synchronize()
    if fused:
        nq.resample_frames_yuv16_device(src.y, src.u, src.v, *src.geometry(), dst.ptrs, size, crop, linear, stream=stream, **_kw(flags))
    else:
        nq.frames_from_yuv16_device(src.y, src.u, src.v, *src.geometry(), dst.ptrs, stream=stream, **_kw(flags))
    torch.cuda.synchronize()
    got = dst.read()
    assert (got == dst.expect(want)).all(), (why, int((got != dst.expect(want)).sum()))          # the whole buffer: guards included
    assert (src.read() == src.host).all(), why


# ---- the grid frame: every Y against the corners of the chroma square and 55 seeded pairs, all three tables across their range ----
GRID_MODES = [(m | r, "sdr") for m in (0, Y.BT709) for r in (0, Y.FULL_RANGE)] + \
             [(Y.BT2020 | t | r, n) for t, n in ((Y.PQ, "pq"), (Y.HLG, "hlg")) for r in (0, Y.FULL_RANGE)]


@pytest.mark.parametrize("mode", GRID_MODES, ids=lambda m: "%s-%d" % (m[1], m[0]))
def test_grid_frame_in_every_mode(nq, mode):
    """1024 x 128, column x has Y = x, row pair r one chroma pair.  P010 with samples in the high bits on the wide path, I010 with
    samples in the low bits one sample off the boundary on the one-pixel path."""
    for msb, layout, pshift in ((Y.MSB, "p010", 0), (0, "i010", 1)):
        flags = mode[0] | msb
        key = ("grid", flags)
        if key not in _REF:
            frame = Y.grid_frame(flags)
            _REF[key] = ([frame], Y.convert([frame], flags))
        frames, want = _REF[key]
        assert want[0].shape == (128, 1024) and (want[0].view(np.uint32) >> 24 == 255).all()
        _device_case(nq, frames, want, layout, flags, pshift, 0)
    # neutral chroma (row pair 4) gives grey in every mode, and the modes differ
    px = _REF[("grid", mode[0] | Y.MSB)][1][0].view(np.uint32)
    row = px[8]
    assert ((row >> 16 & 255) == (row >> 8 & 255)).all() and ((row >> 8 & 255) == (row & 255)).all()


def test_samples_in_the_high_and_in_the_low_bits(nq):
    """The same samples with two sets of junk in the six ignored bits, in the high ten bits (NQ_YUV16_MSB) and in the low ten, give the
    same words."""
    w, h = 24, 10
    rng = np.random.default_rng(5)
    s = [rng.integers(0, 1024, shape, dtype=np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    want = None
    for msb in (Y.MSB, 0):
        for seed in (1, 2):
            junk = [np.random.default_rng(seed).integers(0, 64, p.shape, dtype=np.uint16) for p in s]
            frame = tuple((p << 6 | j) if msb else (j << 10 | p) for p, j in zip(s, junk))
            flags = Y.BT2020 | Y.PQ | msb
            ref = Y.convert([frame], flags)
            want = ref if want is None else want
            assert (ref[0] == want[0]).all()
            for layout, pshift in (("p010", 0), ("i010", 1)):
                _device_case(nq, [frame], want, layout, flags, pshift, 0)


SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (8, 2), (67, 9)]
SHIFTS = ((0, 0), (1, 0), (0, 1))                              # (plane pointers, outputs): aligned; planes one sample on; outputs one word on


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_conversion_equals_the_restatement_in_every_layout(nq, size):
    """Widths 4 and 8 take the wide paths when planes and outputs are aligned (p010, p010_vu: interleaved; i010, yv12_10: planar; 4 x 4
    and 8 x 2 have no odd row, 12 x 5 below has) and the one-pixel path when a pointer is shifted; every other width takes the one-pixel
    path."""
    w, h = size
    for n in (1, 3):
        for flags in MODES:
            frames, want = _converted(w, h, n, flags)
            assert all(r.shape == (h, w) and (r.view(np.uint32) >> 24 == 255).all() for r in want)
            for layout in LAYOUTS:
                for pshift, oshift in SHIFTS:
                    _device_case(nq, frames, want, layout, flags, pshift, oshift)


def test_conversion_with_an_odd_last_row_on_the_wide_paths(nq):
    for flags in MODES:
        frames, want = _converted(12, 5, 2, flags)
        for layout in LAYOUTS:
            for pshift, oshift in SHIFTS:
                _device_case(nq, frames, want, layout, flags, pshift, oshift)


def test_conversion_one_item_past_a_strip(nq):
    """A frame's items are cut into strips of Y16_STRIP.  One-pixel path (an item is a pixel): 41 x 25 = 1025 pixels.  Wide paths (an
    item is 4 x 2 pixels): 164 x 50 = 41 x 25 blocks; with the planes one sample on, the same data takes the one-pixel path."""
    assert Y16_STRIP == 1024 and 41 * 25 == Y16_STRIP + 1
    for (w, h), shifts in (((41, 25), ((0, 0),)), ((164, 50), ((0, 0), (1, 0)))):
        for flags in MODES:
            frames, want = _converted(w, h, 2, flags)
            for layout in LAYOUTS:
                for pshift, oshift in shifts:
                    _device_case(nq, frames, want, layout, flags, pshift, oshift)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_conversion_of_more_strips_than_the_grid_holds(nq, layout):
    """The grid is capped at Y16_MAX_BLOCKS workgroups, which then stride over the rest.  Eight frames that read the same planes, 257
    strips each, in every layout: 513 x 512 on the one-pixel path (SDR and PQ); 2052 x 1024 on the layout's wide path (PQ and SDR),
    and once more with the planes one sample on, where the same data takes the one-pixel path (eight times as many strips)."""
    assert Y16_MAX_BLOCKS == 2048
    for (w, h), modes, pshifts in (((513, 512), (SDR709, PQ2020), (0,)), ((2052, 1024), (PQ2020, SDR709), (0, 1))):
        items = w * h if w % 4 else (w // 4) * (h // 2)
        strips = 8 * ((items + Y16_STRIP - 1) // Y16_STRIP)
        assert Y16_MAX_BLOCKS < strips < Y16_MAX_BLOCKS + 16
        for flags in modes:
            frames, want = _converted(w, h, 1, flags)
            for pshift in pshifts if flags == modes[0] else (0,):
                _device_case(nq, frames * 8, want * 8, layout, flags, pshift, 0, share=True)


def test_seventeen_frames_are_two_launches(nq):
    for flags in (SDR709, PQ2020):
        frames, want = _converted(12, 6, 17, flags)
        for layout in ("p010", "i010"):
            for pshift in (0, 1):
                _device_case(nq, frames, want, layout, flags, pshift, 0)
        small = resample_ref.resample(want, (5, 3), None, Y.LINEAR)
        _device_case(nq, frames, small, "p010", flags, 0, 0, (5, 3), None, True, fused=True)


# (source width, height) -> (target width, height); 4100 x 2 is 4099 x 2 on the wide paths: five chunks of 1024 columns
SHAPES = [((64, 36), (16, 9)), ((67, 41), (13, 7)), ((12, 5), (12, 5)), ((1, 1), (1, 1)), ((4099, 2), (1, 1)), ((4100, 2), (1, 1))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_fused_call_equals_the_restatement(nq, shape):
    (w, h), size = shape
    for linear in (True, False):
        for flags in MODES:
            frames, want = _reduced(w, h, 2, flags, size, None, linear)
            assert all(r.shape == (size[1], size[0]) for r in want)
            for layout in ("p010", "p010_vu", "i010"):
                for pshift, oshift in ((0, 0), (1, 1)):
                    _device_case(nq, frames, want, layout, flags, pshift, oshift, size, None, linear, fused=True)


# crop_x, crop_y of every parity: the chroma of crop pixel (j, i) is the frame's sample ((crop_x + j) >> 1, (crop_y + i) >> 1)
CROPS = [((64, 36), (cx, cy, 40, 20), (9, 7)) for cx in (4, 5) for cy in (2, 3)] + \
        [((67, 41), (cx, cy, 30, 21), (13, 7)) for cx in (2, 3) for cy in (0, 1)] + \
        [((64, 36), (63, 35, 1, 1), None), ((67, 41), (1, 1, 66, 40), (66, 40))]


@pytest.mark.parametrize("case", CROPS, ids=lambda c: "%dx%d-crop%d-%d" % (c[0][0], c[0][1], c[1][0], c[1][1]))
def test_fused_crops_of_every_parity(nq, case):
    (w, h), crop, size = case
    for linear in (True, False):
        for flags in (PQ2020, HLG2020F):
            frames, want = _reduced(w, h, 2, flags, size, crop, linear)
            for layout in LAYOUTS:
                for pshift, oshift in ((0, 0), (1, 1)):
                    _device_case(nq, frames, want, layout, flags, pshift, oshift, size, crop, linear, fused=True)


def test_fused_call_with_more_work_items_than_the_grid_holds(nq):
    """A work item is (frame, output row, block of output columns) and the grid is capped at YR16_MAX_BLOCKS workgroups: 5 frames of
    YR16_MAX_BLOCKS / 5 + 60 rows.  Width 8: the wide paths; width 5: the one-pixel path."""
    rows = YR16_MAX_BLOCKS // 5 + 60
    assert 5 * rows > YR16_MAX_BLOCKS == 8192
    for w, size, layout in ((8, (3, rows), "p010"), (8, (2, rows - 1), "i010"), (5, (3, rows), "p010")):
        frames, want = _reduced(w, rows, 5, PQ2020, size, None, True)
        _device_case(nq, frames, want, layout, PQ2020, 0, 0, size, None, True, fused=True)


@pytest.fixture(scope="module")
def q(nq):
    quantizer = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    yield quantizer
    quantizer.close()


def test_fused_call_equals_the_two_calls_it_is_defined_by(nq, q):
    import torch
    for (w, h), size, crop in (((64, 36), (16, 9), None), ((67, 41), (13, 7), (3, 1, 60, 37)), ((12, 5), (12, 5), None)):
        for flags in (PQ2020, SDR709):
            frames = _frames(w, h, 2, flags)
            for layout in ("p010", "i010"):
                for linear in (True, False):
                    src = _Planes(frames, layout, 0)
                    full = _Stream([np.zeros((h, w), np.int32)] * 2, 0, -7)
                    two = _Stream([np.zeros((size[1], size[0]), np.int32)] * 2, 0, -9)
                    one = _Stream([np.zeros((size[1], size[0]), np.int32)] * 2, 0, -9)
                    nq.frames_from_yuv16_device(src.y, src.u, src.v, *src.geometry(), full.ptrs, **_kw(flags))
                    nq.resample_frames_device(q, full.ptrs, w, h, two.ptrs, size, crop, linear)
                    nq.resample_frames_yuv16_device(src.y, src.u, src.v, *src.geometry(), one.ptrs, size, crop, linear, **_kw(flags))
                    torch.cuda.synchronize()
                    assert (one.read() == two.read()).all(), (w, h, layout, linear, flags)
                    assert (one.read() != -9).sum() == 2 * size[0] * size[1]


@pytest.mark.parametrize("which", ["side", "null"])
def test_on_a_callers_stream_and_on_the_null_stream(nq, which):
    """The planes hold inverted samples until a copy queued on the stream, behind a short spin, makes them true; the two calls follow on
    that stream with no host wait, and the outputs are copied on it.  Work on any other stream would read the inverted samples or be
    overtaken by the snapshot."""
    import torch
    stream = torch.cuda.Stream() if which == "side" else torch.cuda.default_stream()
    handle = stream.cuda_stream
    assert (handle != 0) == (which == "side")
    w, h, n, size = 64, 36, 3, (16, 9)
    frames, want = _converted(w, h, n, PQ2020)
    small = _reduced(w, h, n, PQ2020, size, None, True)[1]
    true = _Planes(frames, "p010", 0)
    work = _Planes([tuple(p ^ np.uint16(0xFFC0) for p in f) for f in frames], "p010", 0)
    assert work.host.shape == true.host.shape
    full = _Stream([np.full(r.shape, -9, np.int32) for r in want], 0, -9)
    red = _Stream([np.full(r.shape, -9, np.int32) for r in small], 0, -9)
    snaps = [torch.empty_like(full.dev), torch.empty_like(red.dev)]
    for spin in (0, 2000000):                                   # the first round loads the kernels; the second runs behind the spin
        work.dev.copy_(torch.from_numpy(work.host.view(np.int16)).cuda())
        full.dev.copy_(torch.from_numpy(full.host).cuda())
        red.dev.copy_(torch.from_numpy(red.host).cuda())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if spin:
                torch.cuda._sleep(spin)
            work.dev.copy_(true.dev, non_blocking=True)
        nq.frames_from_yuv16_device(work.y, work.u, work.v, *work.geometry(), full.ptrs, stream=handle, **_kw(PQ2020))
        nq.resample_frames_yuv16_device(work.y, work.u, work.v, *work.geometry(), red.ptrs, size, stream=handle, **_kw(PQ2020))
        with torch.cuda.stream(stream):
            snaps[0].copy_(full.dev, non_blocking=True)
            snaps[1].copy_(red.dev, non_blocking=True)
        stream.synchronize()
        assert (snaps[0].cpu().numpy() == full.expect(want)).all(), (which, spin)
        assert (snaps[1].cpu().numpy() == red.expect(small)).all(), (which, spin)
    torch.cuda.synchronize()
    assert (work.read() == true.host).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_forms_equal_the_device_forms(nq, layout):
    """... on strided views of one buffer per frame (yuv16_planes with Android's byte strides), which are passed as they are, and on
    tight planes; the library holds as much device memory afterwards as before."""
    inter = layout.startswith("p010")
    for (w, h), size, crop in (((12, 5), (5, 2), None), ((13, 9), (5, 4), (3, 1, 9, 7)), ((64, 6), (16, 3), None)):
        cw2, ch2 = (w + 1) // 2, (h + 1) // 2
        ys, cs = 2 * w + 8, (4 if inter else 2) * cw2 + 8
        words = (h * ys + (1 if inter else 2) * ch2 * cs) // 2
        for flags in (PQ2020, HLG2020F, SDR709):
            rng = np.random.default_rng(70 + w)
            bufs = [rng.integers(0, 65536, words).astype(np.uint16) for _ in range(3)]
            keep = [b.copy() for b in bufs]
            views = [nq.yuv16_planes(b, w, h, layout, ys, cs) for b in bufs]
            tight = [tuple(np.ascontiguousarray(p) for p in f) for f in views]
            want = Y.convert(tight, flags)
            before = nq.device_bytes()
            for frames in (views, tight):
                got = nq.frames_from_yuv16(frames, **_kw(flags))
                assert len(got) == 3 and all(g.dtype == np.int32 and (g == r).all() for g, r in zip(got, want)), (w, h, layout, flags)
            for linear in (True, False):
                small = resample_ref.resample(want, size, crop, Y.LINEAR if linear else 0)
                for frames in (views, tight):
                    got = nq.resample_frames_yuv16(frames, size, crop=crop, linear=linear, **_kw(flags))
                    assert all((g == r).all() for g, r in zip(got, small)), (w, h, layout, flags, linear)
            assert nq.device_bytes() == before
            assert all((a == b).all() for a, b in zip(bufs, keep))
    # size=None and crop=None: the fused call at the frame's own size is the conversion
    assert all((a == b).all() for a, b in zip(nq.resample_frames_yuv16(views, None, **_kw(SDR709)), Y.convert(tight, SDR709)))


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
    (interleaved with either plane first, planar), 5 x 3 takes the one-pixel path.  1:1 and reducing, against the restatement."""
    (w, h), size = shape
    flags = PQ2020
    frames, want = _converted(w, h, 3, flags)
    planes = _arranged(frames, arrangement)
    keep = [tuple(p.copy() for p in f) for f in planes]
    got = nq.frames_from_yuv16(planes, **_kw(flags))
    assert len(got) == 3 and all((g == r).all() for g, r in zip(got, want)), (arrangement, shape)
    for linear in (True, False):
        small = _reduced(w, h, 3, flags, size, None, linear)[1]
        got = nq.resample_frames_yuv16(planes, size, linear=linear, **_kw(flags))
        assert len(got) == 3 and all(g.shape == (size[1], size[0]) and (g == r).all() for g, r in zip(got, small)), (arrangement, shape, linear)
    assert all((a == b).all() for f, k in zip(planes, keep) for a, b in zip(f, k))


def test_invalid_arguments_then_a_valid_call(nq):
    import torch
    L = nq.load_library()
    w, h, n = 12, 8, 3
    cw2, ch2 = 6, 4
    geo = dict(cx=1, cy=2, cw=9, ch=5, dw=4, dh=3)
    yflags = PQ2020
    frames = _frames(w, h, n, yflags)
    full = Y.convert(frames, yflags)
    want = {False: full, True: resample_ref.resample(full, (4, 3), (1, 2, 9, 5), Y.LINEAR)}
    # P010 buffers with room behind the data; the outputs start as -9 and have room for a shifted pointer
    hs = [np.concatenate([y.reshape(-1), np.stack([u, v], -1).reshape(-1), np.zeros(16, np.uint16)]) for y, u, v in frames]
    ho = [np.full(w * h + 2, -9, np.int32) for _ in frames]
    ds = [torch.from_numpy(a.view(np.int16)).cuda() for a in hs]
    do = [torch.from_numpy(a).cuda() for a in ho]
    count = torch.cuda.device_count()

    def ptrs(host):
        base = [a.ctypes.data if host else t.data_ptr() for a, t in zip(hs, ds)]
        return {"y": list(base), "u": [b + 2 * w * h for b in base], "v": [b + 2 * w * h + 2 for b in base],
                "dst": [a.ctypes.data if host else t.data_ptr() for a, t in zip(ho, do)]}

    def call(host, fused, n=n, w=w, h=h, ys=w, cs=2 * cw2, step=2, yflags=yflags, flags=1, device=0, edit=None, null=None, **kw):
        g = dict(geo, **kw)
        p = ptrs(host)
        if edit:
            edit(p)
        arr = lambda v: (C.c_void_p * len(v))(*v)
        a = {k: (None if k == null else arr(v)) for k, v in p.items()}
        name = ("nq_resample_frames_yuv16" if fused else "nq_frames_from_yuv16") + ("" if host else "_device")
        head = ((device,) if host else (device, None)) + (n, a["y"], a["u"], a["v"], w, h, ys, cs, step, yflags)
        if fused:
            rc = getattr(L, name)(*head, g["cx"], g["cy"], g["cw"], g["ch"], a["dst"], g["dw"], g["dh"], flags)
        else:
            rc = getattr(L, name)(*head, a["dst"])
        torch.cuda.synchronize()
        return rc

    def state(host):
        if host:
            return [a.copy() for a in hs + ho]
        return [x.cpu().numpy().copy() for x in ds] + [x.cpu().numpy().copy() for x in do]

    def valid(host, fused):
        """A valid call gives the reference; then the outputs are put back to -9 for the rejected calls that follow."""
        assert call(host, fused) == 0
        got = state(host)
        px = want[fused][0].size
        for k in range(n):
            assert (got[n + k][:px] == want[fused][k].reshape(-1)).all() and (got[n + k][px:] == -9).all()
            assert (got[k].view(np.uint16) == hs[k]).all()
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

    both = [{"n": 0}, {"n": -2}, {"n": 65536}, {"w": 0}, {"w": 65536}, {"h": 0}, {"h": 65536}, {"ys": w - 1}, {"ys": 0}, {"ys": -w}, {"step": 0},
            {"step": 3}, {"step": -1}, {"cs": 2 * (cw2 - 1)}, {"cs": 0}, {"step": 1, "cs": cw2 - 1}, {"yflags": 64}, {"yflags": 127}, {"yflags": -1},
            {"yflags": Y.BT709 | Y.BT2020}, {"yflags": Y.PQ | Y.HLG | Y.BT2020}, {"device": -1}, {"device": count},
            {"null": "y"}, {"null": "u"}, {"null": "v"}, {"null": "dst"},
            {"edit": null_entry("y")}, {"edit": null_entry("u")}, {"edit": null_entry("v")}, {"edit": null_entry("dst")},
            {"edit": off_by("y", 1)}, {"edit": off_by("u", 1)}, {"edit": off_by("v", 1)},
            {"edit": off_by("dst", 2)}, {"edit": off_by("dst", 1)}, {"edit": off_by("dst", 3)},
            {"n": 2, "w": 32768, "h": 32768, "ys": 32768, "cs": 32768},                    # 2^31 pixels: one more than the limit
            {"edit": into("y", 8)}, {"edit": into("y", 4 * ((2 * w * h - 1) // 4))}, {"edit": into("u", 4)},
            {"edit": into("v", 4 * ((2 * 2 * cw2 * ch2 - 1) // 4))}, {"edit": same_output}]
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
                assert (L.nq_last_error(None) or b"") != b""
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


# ---- the converters: yuv16= equals the converter on the converted (and reduced, and turned) frames ----
W, H, N, K = 24, 16, 3, 16


@pytest.fixture(scope="module")
def clip(nq):
    rng = np.random.default_rng(90)
    bufs = [(rng.integers(0, 1024, W * H + 2 * (W // 2) * (H // 2)) << 6).astype(np.uint16) for _ in range(N)]
    frames = [nq.yuv16_planes(b, W, H, "p010") for b in bufs]
    kw = {"transfer": "hlg"}
    return frames, kw, nq.frames_from_yuv16(frames, **kw), nq.resample_frames_yuv16(frames, (12, 8), **kw)


def test_convert_frames_to_gif_and_apng_from_yuv16(nq, clip):
    frames, kw, full, small = clip
    flags = Y.BT2020 | Y.HLG | Y.MSB
    assert all(f.shape == (H, W) for f in full) and all(s.shape == (8, 12) for s in small)
    assert all((a == b).all() for a, b in zip(full, Y.convert(frames, flags)))
    assert all((a == b).all() for a, b in zip(small, Y.resample(frames, (12, 8), None, flags)))
    for convert in (nq.convert_frames_to_gif, nq.convert_frames_to_apng):
        want, wpal = convert(1, full, K, True)
        got, gpal = convert(1, frames, K, True, yuv16=kw)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
        want, wpal = convert(1, small, K, True)
        got, gpal = convert(1, frames, K, True, size=(12, 8), yuv16=kw)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
    # another transfer gives other colours: the keyword reaches the kernel
    assert any((a != b).any() for a, b in zip(full, nq.frames_from_yuv16(frames, transfer="pq")))


def test_the_other_converters_and_orient_from_yuv16(nq, clip):
    frames, kw, full, small = clip
    for convert, args in ((nq.convert_frames_refined, (K, True, 2)), (nq.convert_frames_ordered, (K, 8))):
        wpal, wouts = convert(1, small, *args)
        gpal, gouts = convert(1, frames, *args, size=(12, 8), yuv16=kw)
        assert (np.asarray(gpal) == np.asarray(wpal)).all(), convert.__name__
        assert all((a.index == b.index).all() and (a.argb == b.argb).all() for a, b in zip(gouts, wouts)), convert.__name__
    # orient=6: size and crop are the oriented frame's; the route is the fused reduce of the frames as they lie, then orient_frames
    size, crop = (6, 10), (1, 2, 12, 20)                          # of the 16 x 24 oriented frame
    rect = nq.source_rect(W, H, 6, crop)
    lying = nq.resample_frames_yuv16(frames, (size[1], size[0]), crop=rect, **kw)
    turned = nq.orient_frames(lying, 6)
    assert all(t.shape == (size[1], size[0]) for t in turned)
    got = nq.resample_frames_yuv16(frames, size, crop=crop, orient=6, **kw)
    assert all((a == b).all() for a, b in zip(got, turned))
    # ... which is the full conversion, turned, then reduced (orientation moves words, and the reducer treats both axes alike)
    assert all((a == b).all() for a, b in zip(got, nq.resample_frames(full, size, crop=crop, orient=6)))
    want, wpal = nq.convert_frames_to_gif(1, turned, K, True)
    data, gpal = nq.convert_frames_to_gif(1, frames, K, True, size=size, crop=crop, orient=6, yuv16=kw)
    assert data == want and (np.asarray(gpal) == np.asarray(wpal)).all()
