"""Shot detection on the GPU (nq_frame_signatures* / nq_detect_shots*): the signatures equal the restatement in shots_ref.py exactly, at
the smallest shapes that reach each path of the kernel (one pixel, less than one vector group, whole groups only, a tail, several
workgroups per frame), on content that reaches each way a count is added (every lane its own value, runs of equal neighbours inside
a lane, a channel or a whole frame that is one value across a wave), with 16-byte aligned frames (vector path) and frames offset by
one element (scalar path); more frames than any per-block batching, and 20 000 frames; 81 920 pixels of ONE colour in four counters; a frame with
transparency; frames and guard elements untouched; the host form equals the device form; starts and scores of the two clips of the CPU
tests; every rejected argument leaves the outputs alone and the handle usable; and convert_clip_to_gif equals convert_shots_to_gif
with the starts it found."""
import ctypes as C

import numpy as np
import pytest

import shots_ref
from nquant.android_amd import gif as G
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (7, 3), (64, 64), (67, 5), (300, 200))      # (width, height)
NS = (1, 2, 5)
GUARD = 24                                                     # elements between two frames of a buffer (a multiple of 4)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _frame(w, h, kind, seed):
    """uint32 ARGB frames that reach the kernel's ways to count: 0 random in every channel; 1 opaque, g in runs of 1..6 equal
    neighbours, b one value except for a few pixels; 2 ONE colour; 3 two colours in long stretches."""
    rng = np.random.default_rng(seed)
    n = w * h
    if kind == 0:
        p = rng.integers(0, 2**32, n, dtype=np.uint64)
    elif kind == 1:
        g = np.repeat(rng.integers(0, 256, n), rng.integers(1, 7, n))[:n]
        b = np.where(rng.random(n) < 0.01, rng.integers(0, 256, n), 77)
        p = 255 << 24 | rng.integers(0, 256, n) << 16 | g << 8 | b
    elif kind == 2:
        p = np.full(n, int(rng.integers(0, 2**32)))
    else:
        p = np.where((np.arange(n) // 700) % 2 == 0, 0xFF102030, 0xFF10E030)
    return np.asarray(p).astype(np.uint32).reshape(h, w)


def _frames(w, h, n, seed):
    return [_frame(w, h, (seed + i) % 4, 100 * seed + i) for i in range(n)]


class _Stream:
    """n frames in ONE device buffer, guard elements before, between and after them; frame i starts `shift` elements behind a 16-byte
    boundary (the layout of the temporal hold's tests)."""

    def __init__(self, frames, shift):
        import torch
        px = frames[0].size
        pitch = (px + 7) // 8 * 8 + GUARD
        offs = [GUARD + i * pitch + shift for i in range(len(frames))]
        self.host = np.full(GUARD + len(frames) * pitch + 8, SENTINEL, np.uint32)
        for f, o in zip(frames, offs):
            self.host[o:o + px] = np.asarray(f).reshape(-1).view(np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = [self.dev.data_ptr() + 4 * o for o in offs]
        assert all(p % 16 == 4 * shift for p in self.ptrs)

    def unchanged(self):
        return (self.dev.cpu().numpy().view(np.uint32) == self.host).all()


def _device_case(nq, q, frames, why):
    w, h = frames[0].shape[1], frames[0].shape[0]
    want = shots_ref.signatures(frames)
    assert (want.sum(axis=2) == w * h).all()
    for shift in (0, 1):
        s = _Stream(frames, shift)
        got = nq.frame_signatures_device(q, s.ptrs, w, h)
        assert got.shape == want.shape and got.dtype == np.uint32
        assert (got == want).all(), (why, shift, np.argwhere(got != want)[:4].tolist())
        assert s.unchanged(), (why, shift)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_signatures_equal_the_restatement_on_both_paths(nq, shape):
    w, h = shape
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for n in NS:
            for seed in range(4):                   # every kind of content in every position of the sequence
                _device_case(nq, q, _frames(w, h, n, seed), (w, h, n, seed))
    finally:
        q.close()


def test_mixed_alignment_takes_the_scalar_path_with_the_same_result(nq):
    """One misaligned frame is enough."""
    import torch
    w, h, n = 67, 5, 3
    frames = _frames(w, h, n, 1)
    want = shots_ref.signatures(frames)
    bufs = [torch.from_numpy(np.concatenate([[SENTINEL] * 4, f.reshape(-1), [SENTINEL] * 4]).astype(np.uint32).view(np.int32)).cuda() for f in frames]
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for odd in range(n):
            ptrs = [b.data_ptr() + 16 for b in bufs]
            got0 = nq.frame_signatures_device(q, ptrs, w, h)
            # frame `odd` read one element early: its first pixel is the sentinel, its last one is left out
            ptrs[odd] -= 4
            shifted = list(frames)
            shifted[odd] = np.concatenate([[SENTINEL], frames[odd].reshape(-1)[:-1]]).astype(np.uint32).reshape(h, w)
            got1 = nq.frame_signatures_device(q, ptrs, w, h)
            assert (got0 == want).all() and (got1 == shots_ref.signatures(shifted)).all(), odd
    finally:
        q.close()


def test_more_frames_than_any_batching(nq):
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        _device_case(nq, q, _frames(7, 3, 40, 2), "40 frames")
    finally:
        q.close()


@pytest.mark.parametrize("shape", [(7, 3), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_many_frames_are_many_workgroups(nq, shape):
    """launch_signatures works bpf and the grid n * bpf out from n: with n = 20 000 the cap of workgroups per frame,
    ceil(8 * CUs / n), is 1 on any device of fewer than 2500 CUs, so bpf = 1 and the grid is 20 000 workgroups -- five hundred times
    the 40 frames of the test above, and at 64 x 64 (4096 pixels < SIG_MIN_PIXELS, bpf = 1 from the size as well) four rounds per
    workgroup on the vector path and sixteen on the scalar path.  The table names four frames, one of each kind of content, in a seeded random order; the expected signatures are
    shots_ref.signatures of the frames the table names (21 pixels: all 20 000; 64 x 64: the four, indexed by the same order)."""
    w, h = shape
    n = 20000
    pool = [_frame(w, h, kind, 60 + kind) for kind in range(4)]
    order = np.random.default_rng(w).integers(0, 4, n)
    assert len(set(order[:8].tolist())) > 1
    want = shots_ref.signatures([pool[i] for i in order]) if w * h < 100 else shots_ref.signatures(pool)[order]
    assert want.shape == (n, 4, 256) and (want.sum(axis=2) == w * h).all()
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for shift in (0, 1):
            s = _Stream(pool, shift)
            got = nq.frame_signatures_device(q, [s.ptrs[i] for i in order], w, h)
            assert got.shape == want.shape and got.dtype == np.uint32
            assert (got == want).all(), (shape, shift, np.argwhere(got != want)[:4].tolist())
            assert s.unchanged(), (shape, shift)
    finally:
        q.close()


def test_one_colour_fills_four_counters(nq):
    """512 x 160 frames of ONE colour: 81 920 pixels in four counters, more than a 16-bit counter holds."""
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        frames = [np.full((160, 512), c, np.uint32) for c in (0xFF336699, 0x00000000, 0xFFFFFFFF)]
        _device_case(nq, q, frames, "flat")
        got = nq.frame_signatures(frames)
        assert got[0, 1, 0x33] == got[0, 3, 0x99] == got[1, 0, 0] == got[2, 2, 255] == 81920 and int(got.sum()) == 12 * 81920
    finally:
        q.close()


def test_a_frame_with_transparency_counts_channels_as_stored(nq):
    w, h = 300, 200
    opaque = synth.gradient_noise(w, h, 5)
    frames = [synth.with_alpha(opaque, 3), opaque]
    al = frames[0].view(np.uint32) >> 24
    assert (al == 0).any() and ((al > 15) & (al < 0xE0)).any()
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        _device_case(nq, q, frames, "alpha")
        got = nq.frame_signatures(frames)
        assert (got[0, 1:] == got[1, 1:]).all() and got[1, 0, 255] == w * h and got[0, 0, 0] == int((al == 0).sum())
    finally:
        q.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_device_form(nq, shape):
    w, h = shape
    for n in NS:
        frames = _frames(w, h, n, n)
        keep = [f.copy() for f in frames]
        got = nq.frame_signatures(frames)
        assert (got == shots_ref.signatures(frames)).all(), (w, h, n)          # (what the device form gave above)
        assert all((a == b).all() for a, b in zip(frames, keep))
        got = nq.frame_signatures([f.view(np.int32) for f in frames])
        assert (got == shots_ref.signatures(frames)).all(), (w, h, n)


@pytest.mark.parametrize("clip", ["sprite_cut_clip", "slide_show"])
def test_detect_equals_the_restatement_on_the_clips(nq, hd, clip):
    frames = getattr(shots_ref, clip)()
    n, (h, w) = len(frames), frames[0].shape
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for shift in (0, 1):
            s = _Stream(frames, shift)
            for cut, min_shot in ((60, 1), (60, 2), (60, 3), (60, 8), (1000, 1), (0, 1)):
                starts, scores = nq.detect_shots_device(q, s.ptrs, w, h, cut=cut, min_shot=min_shot)
                assert (starts, scores.tolist()) == shots_ref.detect(frames, cut, min_shot), (clip, shift, cut, min_shot)
            assert s.unchanged()
        for cut, min_shot in ((60, 1), (60, 3)):
            starts, scores = nq.detect_shots(frames, cut=cut, min_shot=min_shot)
            assert (starts, scores.tolist()) == shots_ref.detect(frames, cut, min_shot), (clip, cut, min_shot)
        assert nq.detect_shots(frames)[0] == shots_ref.detect(frames, 60, 8)[0]
        # out_scores NULL is accepted, in both forms
        s = _Stream(frames, 0)
        for entry, ptrs in (("nq_detect_shots_device", s.ptrs), ("nq_detect_shots", [f.ctypes.data for f in frames])):
            starts, count = np.full(n + 1, -5, np.int32), C.c_int32(-5)
            rc = getattr(hd._L, entry)(hd._h, n, (C.c_void_p * n)(*ptrs), w, h, 60, 1, starts.ctypes.data, C.byref(count), None)
            assert rc == 0 and starts[:count.value].tolist() == shots_ref.detect(frames, 60, 1)[0] and (starts[count.value:] == -5).all()
    finally:
        q.close()
    if clip == "sprite_cut_clip":
        assert shots_ref.detect(frames, 60, 1) == ([0, 4], [0, 1, 1, 1, 94, 1, 1, 1])
    else:
        assert [shots_ref.detect(frames, 60, m)[0] for m in (1, 2, 3)] == [[0, 2, 4, 5], [0, 2, 4, 6], [0, 3, 6]]


def test_one_frame_is_one_shot(nq):
    f = _frame(7, 3, 0, 1)
    starts, scores = nq.detect_shots([f], cut=0, min_shot=1)
    assert starts == [0] and scores.tolist() == [0]


def test_invalid_arguments_then_a_valid_call(nq, hd):
    import torch
    L = hd._L
    w, h, n = 6, 4, 3
    frames = _frames(w, h, n, 0)
    want_sig = shots_ref.signatures(frames)
    want = shots_ref.detect(frames, 60, 1)
    hs = [np.concatenate([f.reshape(-1), [0, 0]]).astype(np.uint32) for f in frames]      # room for a 2-byte-off pointer
    ds = [torch.from_numpy(a.view(np.int32)).cuda() for a in hs]

    def call(host, detect, n=n, w=w, h=h, cut=60, min_shot=1, src=0, edit=None, sig=0, starts=0, count=0):
        p = [a.ctypes.data for a in hs] if host else [d.data_ptr() for d in ds]
        if edit:
            edit(p)
        a_src = (C.c_void_p * len(p))(*p) if src == 0 else src
        o_sig = np.full((n if n > 0 else 1) * 1024 + 8, SENTINEL, np.uint32)
        o_starts, o_scores, o_count = np.full(8, -5, np.int32), np.full(8, -5, np.int32), C.c_int32(-5)
        if detect:
            rc = getattr(L, "nq_detect_shots" if host else "nq_detect_shots_device")(
                hd._h, n, a_src, w, h, cut, min_shot, None if starts is None else o_starts.ctypes.data,
                None if count is None else C.byref(o_count), o_scores.ctypes.data)
        else:
            rc = getattr(L, "nq_frame_signatures" if host else "nq_frame_signatures_device")(hd._h, n, a_src, w, h,
                                                                                            None if sig is None else o_sig.ctypes.data)
        return rc, o_sig, o_starts, o_count.value, o_scores

    def state(host):
        return [a.copy() for a in hs] if host else [d.cpu().numpy().copy() for d in ds]

    def valid(host, detect):
        rc, sig, starts, count, scores = call(host, detect)
        assert rc == 0
        if detect:
            assert (starts[:count].tolist(), scores[:n].tolist()) == want and (starts[count:] == -5).all() and (scores[n:] == -5).all()
        else:
            assert (sig[:n * 1024].reshape(n, 4, 256) == want_sig).all() and (sig[n * 1024:] == SENTINEL).all()

    def null_entry(p): p[1] = None

    def off_by(nbytes):
        def edit(p): p[2] += nbytes
        return edit

    frames_bad = [{"n": 0}, {"n": -2}, {"w": 0}, {"w": 65536}, {"h": 0}, {"h": 65536}, {"src": None}, {"edit": null_entry},
                  {"edit": off_by(2)}, {"edit": off_by(1)}, {"n": 2, "w": 32768, "h": 32768}]       # 2^31 pixels: one more than the limit
    rule_bad = [{"cut": -1}, {"cut": 1001}, {"min_shot": 0}, {"min_shot": -1}, {"starts": None}, {"count": None}]
    for host in (True, False):
        for detect in (False, True):
            valid(host, detect)
            for kw in frames_bad + (rule_bad if detect else [{"sig": None}]):
                before = state(host)
                rc, sig, starts, count, scores = call(host, detect, **kw)
                assert rc == -1, (host, detect, kw)
                assert (sig == SENTINEL).all() and (starts == -5).all() and count == -5 and (scores == -5).all(), (host, detect, kw)
                assert (L.nq_last_error(hd._h) or b"") != b""
                assert all((a == b).all() for a, b in zip(before, state(host))), (host, detect, kw)
                valid(host, detect)


def test_clip_to_gif_finds_the_cut_and_equals_the_shots_call(nq):
    clip = shots_ref.sprite_cut_clip()
    kw = dict(seeds=[5] * 8, delays_cs=[4] * 8)
    data, palettes, starts = nq.convert_clip_to_gif(1, clip, 64, True, cut=60, min_shot=1, **kw)
    assert starts == [0, 4] and len(palettes) == 2
    assert not np.array_equal(np.asarray(palettes[0]), np.asarray(palettes[1]))
    want, want_palettes = nq.convert_shots_to_gif(1, clip, [0, 4], 64, True, **kw)
    assert data == want and all(np.array_equal(a, b) for a, b in zip(palettes, want_palettes))
    data, palettes, starts = nq.convert_clip_to_gif(1, clip, 64, True, cut=1000, min_shot=1, **kw)
    want, want_palettes = nq.convert_shots_to_gif(1, clip, [0], 64, True, **kw)
    assert starts == [0] and len(palettes) == 1 and data == want and np.array_equal(palettes[0], want_palettes[0])
