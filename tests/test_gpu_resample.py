"""Frame reduction on the GPU (nq_resample_frames_device / nq_resample_frames): the output equals the restatement in resample_ref.py word
for word, in linear light and in stored values, at the smallest shapes that reach each path of the kernel (one pixel, a copy, integer
and fractional ratios on one or both axes, the 16-byte path and the one-pixel path, several workgroups, footprints longer than a chunk
across and longer than anything down, more work items than the grid holds), for n = 1, 2, 5, with crops, with 16-byte aligned frames
and frames offset by one element; the sources and the guard words around every output stay untouched; the host form equals the device
form; every rejected argument leaves the buffers alone and the handle usable; and the converters' size= / crop= equal resample_frames
followed by the converter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_ref as R
from conftest import ROOT
from nquant.android_amd import gif as G

pytestmark = pytest.mark.gpu

GUARD = 24                                                     # elements between two frames of a buffer (a multiple of 8)
MODES = (True, False)                                          # linear light, stored values


def _kernel_constants():
    """RS_THREADS, RS_CHUNK and RS_MAX_BLOCKS as nq_resample.hip defines them."""
    src = open(os.path.join(ROOT, "nquant.android_amd", "csrc", "nq_resample.hip")).read()
    threads = int(re.search(r"constexpr int RS_THREADS = (\d+);", src).group(1))
    m = re.search(r"constexpr int RS_CHUNK = (\d+) \* RS_THREADS;", src)
    blocks = int(re.search(r"constexpr long long RS_MAX_BLOCKS = (\d+);", src).group(1))
    return threads, int(m.group(1)) * threads, blocks


RS_THREADS, RS_CHUNK, RS_MAX_BLOCKS = _kernel_constants()

# (source width, height) -> (target width, height)
SHAPES = [((1, 1), (1, 1)), ((2, 1), (1, 1)), ((7, 3), (7, 3)), ((8, 8), (4, 4)), ((13, 9), (5, 4)), ((67, 5), (3, 5)),
          ((256, 64), (100, 7)), ((300, 200), (77, 51)), ((4099, 2), (1, 1)), ((2, 2050), (1, 1))]


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


_REF = {}


def _case(w, h, n, size, crop, linear):
    """(frames, reference) of a case, computed once."""
    key = (w, h, n, size, crop, linear)
    if key not in _REF:
        frames = [R.random_argb(w, h, 1000 * w + 10 * h + i) for i in range(n)]
        _REF[key] = frames, R.resample(frames, size, crop, R.LINEAR if linear else 0)
    return _REF[key]


class _Stream:
    """n int32 arrays of one size in ONE device buffer, guard elements before, between and after them; frame i starts `shift`
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


def _device_case(nq, q, frames, want, size, crop, linear, shift):
    import torch
    h, w = frames[0].shape
    src = _Stream(frames, shift, -7)
    dst = _Stream([np.full(r.shape, -9, np.int32) for r in want], shift, -9)
    why = (w, h, len(frames), size, crop, linear, shift)
    assert all(p % 16 == 4 * shift for p in src.ptrs + dst.ptrs), why
    torch.cuda.synchronize()
    nq.resample_frames_device(q, src.ptrs, w, h, dst.ptrs, size, crop, linear)
    torch.cuda.synchronize()
    got = dst.read()
    assert (got == dst.expect(want)).all(), (why, int((got != dst.expect(want)).sum()))          # the whole buffer: guards included
    assert (src.read() == src.host).all(), why


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_device_form_equals_the_restatement_on_both_paths(nq, shape):
    """Aligned frames take the 16-byte path where the width is a multiple of 4 (8, 256, 300) and the one-pixel path elsewhere; frames
    shifted by one element always take the one-pixel path.  4099 x 2 -> 1 x 1 walks five chunks of RS_CHUNK = 1024 columns."""
    (w, h), size = shape
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for n in (1, 2, 5):
            for linear in MODES:
                frames, want = _case(w, h, n, size, None, linear)
                assert all(r.shape == (size[1], size[0]) for r in want)
                for shift in (0, 1):
                    _device_case(nq, q, frames, want, size, None, linear, shift)
    finally:
        q.close()


def test_source_rows_longer_than_a_chunk(nq):
    """A workgroup stages the column sums of RS_CHUNK = 4 * RS_THREADS = 1024 source columns in LDS at once.  2 * RS_CHUNK + 37 columns
    reduced to 2 and to 3 give every output a footprint of more than a chunk, so each work item holds one output column and walks
    two or three chunks, and the seam column between two outputs lies inside a chunk for one of them and opens a chunk for the other.
    On the 16-byte path a chunk starts at a multiple of 4 columns, left of the footprint.  (The grid is capped at RS_MAX_BLOCKS = 8192
    workgroups: test_more_work_items_than_the_grid_holds.)"""
    assert RS_CHUNK == 4 * RS_THREADS == 1024
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for w in (2 * RS_CHUNK + 37, 2 * RS_CHUNK + 40):            # (the second: a multiple of 4, the 16-byte path when aligned)
            for size in ((2, 2), (3, 1)):
                for linear in MODES:
                    frames, want = _case(w, 3, 2, size, None, linear)
                    for shift in (0, 1):
                        _device_case(nq, q, frames, want, size, None, linear, shift)
        # ... and with a crop that starts at an odd column, so that the first chunk of the 16-byte path begins outside the crop
        w = 2 * RS_CHUNK + 40
        crop = (5, 1, w - 9, 2)
        frames, want = _case(w, 3, 2, (2, 1), crop, True)
        for shift in (0, 1):
            _device_case(nq, q, frames, want, (2, 1), crop, True, shift)
    finally:
        q.close()


@pytest.mark.parametrize("shape", [((1200, 4), (300, 2)), ((3001, 3), (700, 2)), ((600, 2), (600, 2))], ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_rows_of_several_column_blocks(nq, shape):
    """A work item holds at most RS_THREADS = 256 output columns, and no more than have their source span in one chunk: 300 outputs
    at ratio 4 are blocks of 255 and 45, 700 at ratio 4.29 blocks of 237, 600 copied blocks of 256, 256 and 88.  The column at a
    block's seam is read by both blocks."""
    (w, h), size = shape
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for linear in MODES:
            frames, want = _case(w, h, 2, size, None, linear)
            for shift in (0, 1):
                _device_case(nq, q, frames, want, size, None, linear, shift)
    finally:
        q.close()


def test_more_work_items_than_the_grid_holds(nq):
    """A work item is (frame, output row, block of output columns) and the grid is capped at RS_MAX_BLOCKS = 8192 workgroups, which
    then take items blockIdx.x, + gridDim.x, ...: 5 frames of RS_MAX_BLOCKS / 5 + 60 rows give 8490 items (chunk: RS_CHUNK = 1024
    source columns, one here)."""
    assert RS_MAX_BLOCKS == 8192
    rows = RS_MAX_BLOCKS // 5 + 60
    assert 5 * rows > RS_MAX_BLOCKS
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for w, size, modes in ((5, (3, rows), MODES), (4, (2, rows - 1), (True,))):          # (width 4: the 16-byte path when aligned)
            for linear in modes:
                frames, want = _case(w, rows, 5, size, None, linear)
                for shift in (0, 1):
                    _device_case(nq, q, frames, want, size, None, linear, shift)
    finally:
        q.close()


CROPS = [((300, 200), (5, 3, 200, 150), (77, 51)),            # an odd crop_x on aligned frames: the 16-byte path starts left of it
         ((300, 200), (177, 143, 123, 57), (50, 20)),         # touches the last row and column
         ((300, 200), (17, 9, 1, 1), (1, 1)),                 # one pixel
         ((300, 200), (299, 199, 1, 1), None),                # the last pixel, size=None: the crop's size
         ((67, 5), (1, 0, 66, 5), (66, 5))]                   # a copy of a crop


@pytest.mark.parametrize("case", CROPS, ids=lambda c: "%dx%d-crop%d" % (c[0][0], c[0][1], c[1][0]))
def test_crops(nq, case):
    (w, h), crop, size = case
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for linear in MODES:
            frames, want = _case(w, h, 2, size, crop, linear)
            assert all(r.shape == ((crop[3], crop[2]) if size is None else (size[1], size[0])) for r in want)
            for shift in (0, 1):
                _device_case(nq, q, frames, want, size, crop, linear, shift)
    finally:
        q.close()


def test_white_2048_square(nq):
    """The largest sums the tests reach: 2 S_c passes 2^46."""
    f = np.full((2048, 2048), -1, np.int32)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for size in ((1, 1), (2, 1)):
            for linear in MODES:
                want = [np.full((size[1], size[0]), -1, np.int32)]
                _device_case(nq, q, [f], want, size, None, linear, 0)
    finally:
        q.close()
    assert (nq.resample_frames([f], (2, 1))[0] == -1).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_host_form_equals_the_device_form(nq, shape):
    (w, h), size = shape
    for n in (1, 2, 5):
        for linear in MODES:
            frames, want = _case(w, h, n, size, None, linear)             # (what the device form gave above)
            keep = [f.copy() for f in frames]
            got = nq.resample_frames(frames, size, linear=linear)
            assert len(got) == n and all(g.dtype == np.int32 and (g == r).all() for g, r in zip(got, want)), (w, h, n, linear)
            assert all((a == b).all() for a, b in zip(frames, keep))
    frames, want = _case(300, 200, 2, (77, 51), (5, 3, 200, 150), True)
    assert all((g == r).all() for g, r in zip(nq.resample_frames(frames, (77, 51), crop=(5, 3, 200, 150)), want))
    frames, want = _case(300, 200, 2, None, (299, 199, 1, 1), False)
    assert all((g == r).all() for g, r in zip(nq.resample_frames(frames, None, crop=(299, 199, 1, 1), linear=False), want))


def test_four_host_forms_on_one_handle_leave_nothing_to_each_other(nq):
    """nq_resample_frames_oriented (code 6), nq_frames_from_yuv_oriented (code 5), nq_resample_frames and nq_orient_frames share the
    handle's staging buffers and each keeps a pointer table of its own: run one after the other on one handle, 3 frames of 8 x 4
    each (reduced to 4 x 2 where the call reduces), every one gives what it gives on a fresh handle."""
    from nquant.android_amd import orient, resample, yuv
    rng = np.random.default_rng(23)
    frames = [rng.integers(-2**31, 2**31, (4, 8)).astype(np.int32) for _ in range(3)]
    planes = [(rng.integers(0, 256, (4, 8), dtype=np.uint8), rng.integers(0, 256, (2, 4), dtype=np.uint8),
               rng.integers(0, 256, (2, 4), dtype=np.uint8)) for _ in range(3)]
    calls = [lambda h: resample._resample_host(h._L, h._h, h._check, frames, (2, 4), None, True, 6),       # (oriented: 4 x 8 -> 2 x 4)
             lambda h: yuv._yuv_host(h._L, h._h, h._check, planes, None, None, True, yuv.YUV_BT709, 5),
             lambda h: resample._resample_host(h._L, h._h, h._check, frames, (4, 2), None, True),
             lambda h: orient._orient_host(h._L, h._h, h._check, frames, 7)]
    shapes = [(4, 2), (8, 4), (2, 4), (8, 4)]
    shared = G._Handle()
    try:
        for k, (call, shape) in enumerate(zip(calls, shapes)):
            got = call(shared)
            fresh = G._Handle()
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want) == 3 and all(g.shape == shape and (g == w).all() for g, w in zip(got, want)), k
    finally:
        shared.close()


def test_invalid_arguments_then_a_valid_call(nq, hd):
    import torch
    L = hd._L
    w, h, n = 12, 8, 3
    geo = dict(cx=1, cy=2, cw=9, ch=5, dw=4, dh=3)
    frames, want = _case(w, h, n, (4, 3), (1, 2, 9, 5), True)
    # buffers with room for an odd pointer behind the data; the outputs start as -9
    hs = [np.concatenate([f.reshape(-1), [0, 0]]).astype(np.int32) for f in frames]
    ho = [np.full(4 * 3 + 2, -9, np.int32) for _ in frames]
    ds = [torch.from_numpy(a).cuda() for a in hs]
    do = [torch.from_numpy(a).cuda() for a in ho]

    def ptrs(host, which):
        arrs = {"src": (hs, ds), "dst": (ho, do)}[which][0 if host else 1]
        return [a.ctypes.data if host else a.data_ptr() for a in arrs]

    def call(host, n=n, w=w, h=h, flags=1, src=0, dst=0, edit=None, **kw):
        g = dict(geo, **kw)
        p = {k: ptrs(host, k) for k in ("src", "dst")}
        if edit:
            edit(p)
        arr = lambda v: (C.c_void_p * len(v))(*v)
        a_src = arr(p["src"]) if src == 0 else src
        a_dst = arr(p["dst"]) if dst == 0 else dst
        rc = getattr(L, "nq_resample_frames" if host else "nq_resample_frames_device")(
            hd._h, n, a_src, w, h, g["cx"], g["cy"], g["cw"], g["ch"], a_dst, g["dw"], g["dh"], flags)
        torch.cuda.synchronize()
        return rc

    def state(host):
        if host:
            return [a.copy() for a in hs + ho]
        return [x.cpu().numpy().copy() for x in ds + do]

    def valid(host):
        """A valid call gives the reference; then the outputs are put back to -9 for the rejected calls that follow."""
        assert call(host) == 0
        got = state(host)
        for k in range(n):
            assert (got[n + k][:12] == want[k].reshape(-1)).all() and (got[n + k][12:] == -9).all() and (got[k] == hs[k]).all()
        for a in ho: a[:] = -9
        if not host:
            for d, a in zip(do, ho): d.copy_(torch.from_numpy(a))

    def null_entry(key):
        def edit(p): p[key][1] = None
        return edit

    def off_by(key, nbytes):
        def edit(p): p[key][2] += nbytes
        return edit

    def alias(p):                   # output 1 begins inside source 0
        p["dst"][1] = p["src"][0] + 4 * (w * h - 2)

    def same_output(p):             # outputs 0 and 2 overlap by one word
        p["dst"][2] = p["dst"][0] + 4 * 11

    bad = [{"n": 0}, {"n": -2}, {"w": 0}, {"w": 65536}, {"h": 0}, {"h": 65536},
           {"cw": 0}, {"ch": 0}, {"cx": -1}, {"cy": -1}, {"cx": 4}, {"cy": 4}, {"cw": 12, "dw": 4}, {"ch": 7},       # empty / leaves the frame
           {"dw": 0}, {"dh": 0}, {"dw": 10}, {"dh": 6}, {"dw": -1},                                                   # target < 1 / larger than the crop
           {"flags": 2}, {"flags": 3}, {"flags": -1}, {"src": None}, {"dst": None},
           {"edit": null_entry("src")}, {"edit": null_entry("dst")},
           {"edit": off_by("src", 2)}, {"edit": off_by("dst", 2)}, {"edit": off_by("src", 1)}, {"edit": off_by("dst", 3)},
           {"n": 2, "w": 32768, "h": 32768},                   # 2^31 pixels: one more than the limit
           {"edit": alias}, {"edit": same_output}]
    for host in (True, False):
        valid(host)
        for kw in bad:
            before = state(host)
            rc = call(host, **kw)
            assert rc == -1, (host, kw)
            assert (L.nq_last_error(hd._h) or b"") != b""
            assert all((a == b).all() for a, b in zip(before, state(host))), (host, kw)
            valid(host)
        # the same source for every frame is allowed: sources are only read
        def one_source(p): p["src"][1] = p["src"][2] = p["src"][0]
        assert call(host, edit=one_source) == 0
        got = state(host)
        assert all((got[n + k][:12] == want[0].reshape(-1)).all() for k in range(n))
        valid(host)


# ---- the converters: size= / crop= equal resample_frames followed by the converter ----
W, H, N, K = 96, 80, 4, 32
SIZE, CROP = (40, 30), (7, 4, 80, 64)


@pytest.fixture(scope="module")
def clip(nq):
    frames = []
    for i in range(N):                                  # two shots of two frames: dark noise, then bright noise; frames of a shot differ in the low bits
        base = R.random_argb(W, H, 40 + i // 2, p_clear=0.0, p_opaque=1.0).view(np.uint32)
        base = (base & np.uint32(0xFF7F7F7F)) | np.uint32(0x00808080 * (i // 2))
        frames.append((base ^ np.uint32(0x00030201 * (i % 2))).view(np.int32))
    return frames, nq.resample_frames(frames, SIZE, crop=CROP), nq.resample_frames(frames, SIZE, crop=CROP, linear=False)


def test_convert_frames_to_gif_with_size_and_crop(nq, clip):
    frames, small, small_stored = clip
    assert all(s.shape == (SIZE[1], SIZE[0]) for s in small) and any((a != b).any() for a, b in zip(small, small_stored))
    for kw in ({}, {"delta": True}, {"delta": True, "hold": 3}, {"refine": 2}, {"lossy": 4}):
        want, wpal = nq.convert_frames_to_gif(1, small, K, True, **kw)
        got, gpal = nq.convert_frames_to_gif(1, frames, K, True, size=SIZE, crop=CROP, **kw)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all(), kw
    want, _ = nq.convert_frames_to_gif(1, small_stored, K, True)
    got, _ = nq.convert_frames_to_gif(1, frames, K, True, size=SIZE, crop=CROP, linear_resample=False)
    assert got == want
    # a crop alone keeps the crop's size; a size alone reduces the whole frame
    want, _ = nq.convert_frames_to_gif(0, nq.resample_frames(frames, None, crop=CROP), K, True)
    assert nq.convert_frames_to_gif(0, frames, K, True, crop=CROP)[0] == want
    want, _ = nq.convert_frames_to_gif(0, nq.resample_frames(frames, SIZE), K, True)
    assert nq.convert_frames_to_gif(0, frames, K, True, size=SIZE)[0] == want


def test_convert_clip_and_shots_to_gif_with_size_and_crop(nq, clip):
    frames, small, _ = clip
    want = nq.convert_clip_to_gif(1, small, K, True, min_shot=2)
    got = nq.convert_clip_to_gif(1, frames, K, True, min_shot=2, size=SIZE, crop=CROP)
    assert got[0] == want[0] and got[2] == want[2] and len(got[1]) == len(want[1])
    assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got[1], want[1]))
    assert want[2] == [0, 2]                                                           # the shots were found on the reduced frames
    want = nq.convert_shots_to_gif(1, small, [0, 2], K, True)
    got = nq.convert_shots_to_gif(1, frames, [0, 2], K, True, size=SIZE, crop=CROP)
    assert got[0] == want[0] and all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got[1], want[1]))


def test_convert_frames_to_apng_and_refined_with_size_and_crop(nq, clip):
    frames, small, _ = clip
    for kw in ({}, {"hold": 3}):
        want, wpal = nq.convert_frames_to_apng(1, small, K, True, **kw)
        got, gpal = nq.convert_frames_to_apng(1, frames, K, True, size=SIZE, crop=CROP, **kw)
        assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all(), kw
    wpal, wouts = nq.convert_frames_refined(1, small, K, True, 2)
    gpal, gouts = nq.convert_frames_refined(1, frames, K, True, 2, size=SIZE, crop=CROP)
    assert (np.asarray(gpal) == np.asarray(wpal)).all()
    assert all((a.index == b.index).all() and (a.argb == b.argb).all() for a, b in zip(gouts, wouts))


def test_without_size_and_crop_nothing_changes(nq, clip):
    frames, small, _ = clip
    assert nq.convert_frames_to_gif(1, small, K, True, size=None, crop=None)[0] == nq.convert_frames_to_gif(1, small, K, True)[0]
    assert nq.convert_frames_to_gif(1, small, K, True, delta=True, hold=3, size=None, crop=None)[0] == \
        nq.convert_frames_to_gif(1, small, K, True, delta=True, hold=3)[0]
    assert nq.convert_clip_to_gif(1, small, K, True, min_shot=2, size=None, crop=None)[0] == nq.convert_clip_to_gif(1, small, K, True, min_shot=2)[0]
    assert nq.convert_shots_to_gif(1, small, [0, 2], K, True, size=None, crop=None)[0] == nq.convert_shots_to_gif(1, small, [0, 2], K, True)[0]
    assert nq.convert_frames_to_apng(1, small, K, True, size=None, crop=None)[0] == nq.convert_frames_to_apng(1, small, K, True)[0]
    a, b = nq.convert_frames_refined(1, small, K, True, 2, size=None, crop=None), nq.convert_frames_refined(1, small, K, True, 2)
    assert (np.asarray(a[0]) == np.asarray(b[0])).all() and all((x.index == y.index).all() for x, y in zip(a[1], b[1]))
