"""Temporal hold on the GPU (nq_hold_frames_device / nq_hold_frames): index maps, ARGB outputs and held counts equal the restatement in
hold_ref.py exactly, at the smallest shapes that reach each path of the kernel (one pixel, less than one vector group, whole groups
only, a tail, several blocks), with 16-byte aligned frames (vector path) and frames offset by one element (scalar path), with and
without outputs and counts; frame 0 and the guard elements around every frame stay untouched; the host form equals the device form;
every rejected argument leaves the buffers alone and the handle usable; and through convert_frames_to_gif / convert_frames_to_apng
the still background of a noisy sequence drops out of the file."""
import ctypes as C

import numpy as np
import pytest

import apng_ref
import gif_delta_ref
import hold_ref
from nquant.android_amd import gif as G

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (7, 3), (64, 64), (67, 5), (300, 200))      # (width, height)
NS = (1, 2, 5)
TS = (0, 3, 255)
GUARD = 24                                                     # elements between two frames of a buffer (a multiple of 8)


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _sequence(w, h, n, seed):
    """Random ARGB sources in which a seeded half of the pixels repeat the frame before within +-3 per channel (half of those bit for
    bit, so that threshold 0 holds some too); random indices below 256; random ARGB outputs."""
    rng = np.random.default_rng(seed)
    ch = rng.integers(0, 256, (h, w, 4))
    frames = []
    for i in range(n):
        if i:
            near = np.clip(ch + rng.integers(-3, 4, (h, w, 4)) * rng.integers(0, 2, (h, w, 1)), 0, 255)      # (half of them exactly)
            ch = np.where((rng.random((h, w)) < 0.5)[..., None], near, rng.integers(0, 256, (h, w, 4)))
        frames.append((ch[..., 0] << 24 | ch[..., 1] << 16 | ch[..., 2] << 8 | ch[..., 3]).astype(np.uint32).view(np.int32))
    idx = [rng.integers(0, 256, (h, w)).astype(np.uint16) for _ in range(n)]
    outs = [rng.integers(-2**31, 2**31, (h, w)).astype(np.int32) for _ in range(n)]
    return frames, idx, outs


class _Stream:
    """n arrays of one stream in ONE device buffer, guard elements before, between and after them; frame i starts `shift` elements
    behind a 16-byte boundary."""

    def __init__(self, arrays, shift, sentinel):
        import torch
        self.dtype = arrays[0].dtype
        px = arrays[0].size
        pitch = (px + 7) // 8 * 8 + GUARD
        self.offs = [GUARD + i * pitch + shift for i in range(len(arrays))]
        self.px = px
        self.host = np.full(GUARD + len(arrays) * pitch + 8, sentinel, self.dtype)
        self.fill(self.host, arrays)
        signed = self.host.view(np.int16 if self.dtype == np.uint16 else np.int32)
        self.dev = torch.from_numpy(signed.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = [self.dev.data_ptr() + self.host.itemsize * o for o in self.offs]

    def fill(self, buf, arrays):
        for a, o in zip(arrays, self.offs):
            buf[o:o + self.px] = np.asarray(a).reshape(-1)

    def expect(self, arrays):
        want = self.host.copy()
        self.fill(want, arrays)
        return want

    def read(self):
        return self.dev.cpu().numpy().view(self.dtype)


def _device_case(nq, q, frames, idx, outs, w, h, t, ref, shift, with_out, with_held):
    src = _Stream(frames, shift, -7)
    ind = _Stream(idx, shift, 0xFFFF)
    out = _Stream(outs, shift, -9) if with_out else None
    held = nq.hold_frames_device(q, src.ptrs, ind.ptrs, w, h, t, out.ptrs if out else None, counts=with_held)
    why = (w, h, len(frames), t, shift, with_out, with_held)
    if shift:
        assert all(p % 16 for p in src.ptrs + ind.ptrs), why
    else:
        assert not any(p % 16 for p in src.ptrs + ind.ptrs + (out.ptrs if out else [])), why
    ridx, rheld, rout = ref
    if with_held:
        assert held.tolist() == rheld, why
    else:
        assert held is None
    assert (ind.read() == ind.expect(ridx)).all(), why          # the whole buffer: guards and frame 0 included
    assert (src.read() == src.host).all(), why
    if out:
        assert (out.read() == out.expect(rout)).all(), why


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_device_form_equals_the_restatement_on_both_paths(nq, shape):
    w, h = shape
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for n in NS:
            frames, idx, outs = _sequence(w, h, n, 1000 * w + n)
            for t in TS:
                ref = hold_ref.hold(frames, idx, t, outs)
                assert ref[1][0] == 0 and (ref[0][0] == idx[0]).all() and (ref[2][0] == outs[0]).all()
                if n > 1 and t == 3:
                    assert 0 < ref[1][1] < w * h or w * h < 4                      # the case decides something
                for shift in (0, 1):
                    for with_out in (True, False):
                        for with_held in (True, False):
                            _device_case(nq, q, frames, idx, outs, w, h, t, ref, shift, with_out, with_held)
    finally:
        q.close()


def test_mixed_alignment_takes_the_scalar_path_with_the_same_result(nq):
    """One stream misaligned is enough: index maps offset by one element (2 bytes), everything else 16-byte aligned, and the reverse."""
    w, h, n, t = 67, 5, 5, 3
    frames, idx, outs = _sequence(w, h, n, 77)
    ref = hold_ref.hold(frames, idx, t, outs)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for s_src, s_idx, s_out in ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 3, 2)):
            src, ind, out = _Stream(frames, s_src, -7), _Stream(idx, s_idx, 0xFFFF), _Stream(outs, s_out, -9)
            held = nq.hold_frames_device(q, src.ptrs, ind.ptrs, w, h, t, out.ptrs)
            assert held.tolist() == ref[1]
            assert (ind.read() == ind.expect(ref[0])).all() and (out.read() == out.expect(ref[2])).all() and (src.read() == src.host).all()
    finally:
        q.close()


def test_long_sequence_counts_every_frame(nq):
    """A block collects the counts of 32 frames at a time before it adds them to the totals: 70 frames cross that boundary twice and
    end inside a round; two blocks on the vector path, six on the scalar path."""
    w, h, n, t = 67, 39, 70, 3
    frames, idx, outs = _sequence(w, h, n, 9)
    ref = hold_ref.hold(frames, idx, t, outs)
    assert all(0 < c < w * h for c in ref[1][1:])
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        for shift in (0, 1):
            _device_case(nq, q, frames, idx, outs, w, h, t, ref, shift, True, True)
    finally:
        q.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_device_form(nq, shape):
    w, h = shape
    for n in NS:
        frames, idx, outs = _sequence(w, h, n, 1000 * w + n)
        for t in TS:
            ridx, rheld, rout = hold_ref.hold(frames, idx, t, outs)          # (what the device form gave above)
            keep_idx, keep_out = [a.copy() for a in idx], [o.copy() for o in outs]
            got, held, gout = nq.hold_frames(frames, idx, t, out_argb=outs)
            assert held.tolist() == rheld, (w, h, n, t)
            assert all((a == b).all() for a, b in zip(got, ridx)) and all((a == b).all() for a, b in zip(gout, rout)), (w, h, n, t)
            assert all((a == b).all() for a, b in zip(idx, keep_idx)) and all((a == b).all() for a, b in zip(outs, keep_out))
            got, held = nq.hold_frames(frames, idx, t)
            assert held.tolist() == rheld and all((a == b).all() for a, b in zip(got, ridx)), (w, h, n, t)


def test_invalid_arguments_then_a_valid_call(nq, hd):
    import torch
    L = hd._L
    w, h, n, t = 6, 4, 3, 3
    frames, idx, outs = _sequence(w, h, n, 5)
    ridx, rheld, rout = hold_ref.hold(frames, idx, t, outs)
    # host buffers with room for an odd / 2-byte-off pointer behind the data
    hs = [np.concatenate([f.reshape(-1), [0, 0]]).astype(np.int32) for f in frames]
    hi = [np.concatenate([a.reshape(-1), [0, 0]]).astype(np.uint16) for a in idx]
    ho = [np.concatenate([o.reshape(-1), [0, 0]]).astype(np.int32) for o in outs]
    ds = [torch.from_numpy(a).cuda() for a in hs]
    di = [torch.from_numpy(a.view(np.int16)).cuda() for a in hi]
    do = [torch.from_numpy(a).cuda() for a in ho]

    def ptrs(host, which):
        arrs = {"src": (hs, ds), "idx": (hi, di), "out": (ho, do)}[which][0 if host else 1]
        return [a.ctypes.data if host else a.data_ptr() for a in arrs]

    def call(host, n=n, w=w, h=h, t=t, src=0, ind=0, out=0, edit=None):
        p = {k: ptrs(host, k) for k in ("src", "idx", "out")}
        if edit:
            edit(p)
        arr = lambda v: (C.c_void_p * len(v))(*v)
        a_src = arr(p["src"]) if src == 0 else src
        a_idx = arr(p["idx"]) if ind == 0 else ind
        a_out = arr(p["out"]) if out == 0 else out
        held = np.full(8, -5, np.int64)
        rc = getattr(L, "nq_hold_frames" if host else "nq_hold_frames_device")(hd._h, n, a_src, a_idx, a_out, w, h, t, held.ctypes.data)
        return rc, held

    def state(host):
        if host:
            return [a.copy() for a in hs + hi + ho]
        return [x.cpu().numpy().copy() for x in ds + di + do]

    def valid(host):
        """A valid call on fresh copies of the data gives the reference."""
        for a, f in zip(hs, frames): a[:w * h] = f.reshape(-1)
        for a, f in zip(hi, idx): a[:w * h] = f.reshape(-1)
        for a, f in zip(ho, outs): a[:w * h] = f.reshape(-1)
        if not host:
            for d, a in zip(ds + do, hs + ho): d.copy_(torch.from_numpy(a))
            for d, a in zip(di, hi): d.copy_(torch.from_numpy(a.view(np.int16)))
        rc, held = call(host)
        assert rc == 0 and held[:n].tolist() == rheld and (held[n:] == -5).all()
        got = state(host)
        for k in range(n):
            assert (got[n + k].view(np.uint16)[:w * h] == ridx[k].reshape(-1)).all() and (got[2 * n + k][:w * h] == rout[k].reshape(-1)).all()
        # put the inputs back for the rejected calls that follow
        for a, f in zip(hi, idx): a[:w * h] = f.reshape(-1)
        for a, f in zip(ho, outs): a[:w * h] = f.reshape(-1)
        if not host:
            for d, a in zip(do, ho): d.copy_(torch.from_numpy(a))
            for d, a in zip(di, hi): d.copy_(torch.from_numpy(a.view(np.int16)))

    def null_entry(key):
        def edit(p): p[key][1] = None
        return edit

    def off_by(key, nbytes):
        def edit(p): p[key][2] += nbytes
        return edit

    bad = [{"n": 0}, {"n": -2}, {"w": 0}, {"w": 65536}, {"h": 0}, {"h": 65536}, {"t": -1}, {"t": 256}, {"src": None}, {"ind": None},
           {"edit": null_entry("src")}, {"edit": null_entry("idx")}, {"edit": null_entry("out")},
           {"edit": off_by("idx", 1)}, {"edit": off_by("src", 2)}, {"edit": off_by("out", 2)}, {"edit": off_by("src", 1)},
           {"n": 2, "w": 32768, "h": 32768}]                   # 2^31 pixels: one more than the limit
    for host in (True, False):
        valid(host)
        for kw in bad:
            before = state(host)
            rc, held = call(host, **kw)
            assert rc == -1, (host, kw)
            assert (held == -5).all(), (host, kw)
            assert (L.nq_last_error(hd._h) or b"") != b""
            assert all((a == b).all() for a, b in zip(before, state(host))), (host, kw)
            valid(host)
        # out_argb NULL as a whole is the form without outputs, n = 1 does nothing
        rc, held = call(host, out=None)
        assert rc == 0 and held[:n].tolist() == rheld
        before = state(host)
        rc, held = call(host, n=1)
        assert rc == 0 and held[0] == 0 and (held[1:] == -5).all() and all((a == b).all() for a, b in zip(before, state(host)))
        valid(host)


# ---- the pipeline: a sprite over a still background with sensor-like noise ----
H, W, N, K, T = 80, 96, 4, 32, 4


@pytest.fixture(scope="module")
def footage(nq):
    frames, boxes = hold_ref.noisy_sprite_sequence(H, W, N, 21)
    seeds = [5] * N
    pal, outs = nq.convert_frames(1, frames, K, True, seeds=seeds)
    maps = [o.index for o in outs]
    want, held, _ = hold_ref.hold(frames, maps, T)
    return frames, boxes, seeds, pal, maps, want, held


def _inside(rect, boxes, i):
    x, y, w, h = rect
    ys, xs = np.nonzero(hold_ref.union_mask(H, W, boxes[i - 1], boxes[i]))
    return xs.min() <= x and x + w <= xs.max() + 1 and ys.min() <= y and y + h <= ys.max() + 1


def test_noisy_footage_to_delta_gif_keeps_only_the_sprite(nq, footage):
    frames, boxes, seeds, pal, maps, want, held = footage
    plain, pal0 = nq.convert_frames_to_gif(1, frames, K, True, seeds=seeds, delta=True)
    none, _ = nq.convert_frames_to_gif(1, frames, K, True, seeds=seeds, delta=True, hold=None)
    assert none == plain and plain == gif_delta_ref.encode(maps, pal)
    data, pal2 = nq.convert_frames_to_gif(1, frames, K, True, seeds=seeds, delta=True, hold=T)
    assert (np.asarray(pal2) == np.asarray(pal)).all() and (np.asarray(pal0) == np.asarray(pal)).all()
    canvases = gif_delta_ref.compose(data)
    assert len(canvases) == N
    for i, (c, m) in enumerate(zip(canvases, want)):
        assert (c == m).all(), i
    assert data == gif_delta_ref.encode(want, pal)
    _, _, parsed = gif_delta_ref.parse(data)
    for i in range(1, N):
        p = parsed[i]
        assert _inside((p["x"], p["y"], p["w"], p["h"]), boxes, i), (i, p["x"], p["y"], p["w"], p["h"])
    print("delta GIF bytes, hold off / hold=%d: %d / %d" % (T, len(plain), len(data)))
    assert len(data) < len(plain)
    got, counts = nq.hold_frames(frames, maps, T)
    assert counts.tolist() == held and all((a == b).all() for a, b in zip(got, want))


def test_noisy_footage_to_apng_keeps_only_the_sprite(nq, footage):
    frames, boxes, seeds, pal, maps, want, held = footage
    plain, pal0 = nq.convert_frames_to_apng(1, frames, K, True, seeds=seeds)
    none, _ = nq.convert_frames_to_apng(1, frames, K, True, seeds=seeds, hold=None)
    assert none == plain and plain == apng_ref.encode(maps, pal)
    data, pal2, rects = nq.convert_frames_to_apng(1, frames, K, True, seeds=seeds, hold=T, return_rects=True)
    assert (np.asarray(pal2) == np.asarray(pal)).all() and (np.asarray(pal0) == np.asarray(pal)).all()
    canvases = apng_ref.compose(data)
    assert len(canvases) == N
    for i, (c, m) in enumerate(zip(canvases, want)):
        assert (c == apng_ref.rgba_of(m, pal)).all(), i
    assert data == apng_ref.encode(want, pal)
    for i in range(1, N):
        assert _inside(tuple(rects[i].tolist()), boxes, i), (i, rects[i].tolist())
    print("APNG bytes, hold off / hold=%d: %d / %d" % (T, len(plain), len(data)))
    assert len(data) < len(plain)
