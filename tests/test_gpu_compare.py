"""The quality measurement on the GPU (nq_compare_frames / nq_compare_indexed and their _device forms) against the numpy restatement
tests/compare_ref.py: all 16 slots equal, for both flags and both forms, on both access paths, around the frames-per-launch constant
and past the grid cap; the plumbing (nothing allocated, guards intact, inputs unchanged); a caller's stream; and choose_colors."""
import ctypes as C

import numpy as np
import pytest

import compare_ref
import resample_ref
import stream_gate as G
from test_compare_cpu import BLACK, WHITE, _checker, _full, constants, sample

pytestmark = pytest.mark.gpu

PER_LAUNCH, GRID_CAP, STRIP, WAVES = constants()
# (width, height): 260 x 9 and 181 x 187 cross a wave's strip width / leave a partial last strip
SHAPES = [(1, 1), (7, 5), (8, 8), (9, 9), (45, 37), (64, 64), (STRIP + 4, 9), (181, 187)]
# widths the 16-byte path takes, 4 mod 8 among them
WIDE = [(4, 3), (8, 8), (12, 5), (64, 64), (STRIP + 4, 9), (2 * STRIP + 12, 17), (180, 187)]
GUARD = 32


def pair(w, h, seed):
    """A random pair with clear and semi-transparent pixels on either or both sides; the output shares most pixels with the source."""
    src = resample_ref.random_argb(w, h, seed)
    other = resample_ref.random_argb(w, h, seed + 7919)
    near = (src.view(np.uint32) ^ (other.view(np.uint32) & np.uint32(0x07070707))).view(np.int32)
    u = np.random.default_rng(seed + 1).random((h, w))
    return src, np.where(u < 0.5, near, np.where(u < 0.75, other, src))


class Dev:
    """Arrays of any sizes in ONE device buffer: array i starts shifts[i] elements behind a 16-byte boundary, guard elements around all."""

    def __init__(self, arrays, shifts, dtype):
        import torch
        per16 = 16 // np.dtype(dtype).itemsize
        self.offs, at = [], GUARD
        for a, s in zip(arrays, shifts):
            self.offs.append(at + s)
            at += (a.size + s + per16 - 1) // per16 * per16 + GUARD
        self.sizes = [a.size for a in arrays]
        sentinel = {2: 0xA5A5, 4: 0xA5A5A5A5, 8: -7}[np.dtype(dtype).itemsize]
        self.host = np.full(at, sentinel, dtype)
        for a, o in zip(arrays, self.offs):
            self.host[o:o + a.size] = np.ascontiguousarray(a).reshape(-1).view(dtype)
        signed = {2: np.int16, 4: np.int32, 8: np.int64}[np.dtype(dtype).itemsize]
        self.dev = torch.from_numpy(self.host.view(signed).copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = [self.dev.data_ptr() + np.dtype(dtype).itemsize * o for o in self.offs]

    def read(self):
        return self.dev.cpu().numpy().view(self.host.dtype)


def tab(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def run_device(nq, src, out, flags, shifts=None, palette=None, stream=None, check=True):
    """The device form on resident copies of the pairs (out: ARGB frames, or index maps with a palette); returns (status, (n, 16) slots).
    check: guards, inputs and the library's device memory are verified too."""
    import torch
    L = nq.load_library()
    n = len(src)
    shifts = [0] * n if shifts is None else shifts
    d_src = Dev(src, shifts, np.uint32)
    d_out = Dev(out, shifts, np.uint16 if palette is not None else np.uint32)
    d_res = Dev([np.full(16 * n, -7, np.int64)], [0], np.int64)
    w = np.array([f.shape[1] for f in src], np.int32)
    h = np.array([f.shape[0] for f in src], np.int32)
    torch.cuda.synchronize()
    before = nq.device_bytes()
    if palette is None:
        rc = L.nq_compare_frames_device(0, stream, n, tab(d_src.ptrs), tab(d_out.ptrs), w.ctypes.data, h.ctypes.data, flags, d_res.ptrs[0])
    else:
        pal = np.ascontiguousarray(palette).view(np.uint32)
        rc = L.nq_compare_indexed_device(0, stream, n, tab(d_src.ptrs), tab(d_out.ptrs), pal.ctypes.data, pal.size, w.ctypes.data, h.ctypes.data,
                                         flags, d_res.ptrs[0])
    torch.cuda.synchronize()
    got = d_res.read()
    if check:
        assert nq.device_bytes() == before
        assert (got[:GUARD] == -7).all() and (got[GUARD + 16 * n:] == -7).all(), "guard words around d_result"
        assert (d_src.read() == d_src.host).all() and (d_out.read() == d_out.host).all(), "a frame was written"
    return rc, got[GUARD:GUARD + 16 * n].reshape(n, 16).copy()


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: (frame, slot) %s differ: got %s, want %s" % (what, bad[:6].tolist(), got[got != want][:6].tolist(),
                                                                           want[got != want][:6].tolist())


_PAIRS = {}


def pairs(shapes):
    """(sources, outputs, {flags: reference}) of one pair per shape, computed once."""
    key = tuple(shapes)
    if key not in _PAIRS:
        ps = [pair(w, h, 1000 + 31 * i + w) for i, (w, h) in enumerate(shapes)]
        src, out = [p[0] for p in ps], [p[1] for p in ps]
        _PAIRS[key] = (src, out, {f: compare_ref.compare_frames(src, out, f) for f in (0, 1)})
    return _PAIRS[key]


# ---- against the restatement ----
@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("path", ["vector", "one pixel: shifted", "one pixel: odd widths"])
def test_frames_against_the_restatement(nq, path, flags):
    shapes = WIDE if path != "one pixel: odd widths" else SHAPES
    src, out, ref = pairs(shapes)
    rc, got = run_device(nq, src, out, flags, [1 if path == "one pixel: shifted" else 0] * len(src))
    assert rc == 0
    same(got, ref[flags], path)


def indexed_case(shapes, K, seed):
    rng = np.random.default_rng(seed)
    src = pairs(shapes)[0]
    pal = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    pal[K // 2] &= np.uint32(0x00FFFFFF)                 # a fully transparent entry
    pal[K - 1] = (pal[K - 1] & np.uint32(0x00FFFFFF)) | np.uint32(0x80000000)
    idx = [rng.integers(0, K, f.shape).astype(np.uint16) for f in src]
    return src, idx, pal


@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("K", [1, 2, 256])
@pytest.mark.parametrize("path", ["vector", "one pixel"])
def test_indexed_against_the_restatement(nq, path, K, flags):
    src, idx, pal = indexed_case(WIDE if path == "vector" else SHAPES, K, 50 + K)
    want = compare_ref.compare_indexed(src, idx, pal, flags)
    rc, got = run_device(nq, src, idx, flags, [0 if path == "vector" else 1] * len(src), palette=pal)
    assert rc == 0
    same(got, want, path)
    if K == 256 and flags == 1:                         # the host form, and the ARGB form of palette[index]
        same(np.stack([q.slots for q in nq.compare_indexed(src, idx, pal)]), want, "host form")
        same(np.stack([q.slots for q in nq.compare_frames(src, [pal[m] for m in idx])]), want, "palette[index]")


def test_an_index_past_the_palette(nq):
    """In the last frame: the host form returns NQ_ERR_INVALID after the run, every frame's slots are those of the definition (the index
    reads as the word 0); the device form, which waits for nothing, gives the same slots."""
    L = nq.load_library()
    src, idx, pal = indexed_case(SHAPES, 5, 77)
    idx = [m.copy() for m in idx]
    idx[-1][3, 2], idx[-1][100, 180] = 5, 40000
    want = compare_ref.compare_indexed(src, idx, pal)
    n = len(src)
    res = np.zeros((n, 16), np.int64)
    w, h = np.array([f.shape[1] for f in src], np.int32), np.array([f.shape[0] for f in src], np.int32)
    rc = L.nq_compare_indexed(0, n, tab([f.ctypes.data for f in src]), tab([m.ctypes.data for m in idx]), pal.ctypes.data, 5, w.ctypes.data,
                              h.ctypes.data, 1, res.ctypes.data)
    assert rc == -1 and b"frame %d" % (n - 1) in L.nq_last_error(None)
    same(res, want, "host form")
    with pytest.raises(nq.NqError) as e:
        nq.compare_indexed(src, idx, pal)
    assert e.value.status == -1
    rc, got = run_device(nq, src, idx, 1, [1] * n, palette=pal)
    assert rc == 0
    same(got, want, "device form")


@pytest.mark.parametrize("n", [1, 3, PER_LAUNCH, PER_LAUNCH + 1, 2 * PER_LAUNCH + 1])
def test_frame_counts_around_a_launch(nq, n):
    """Frames of different sizes in one call.  The first launch's frames all allow the 16-byte path; from the frames-per-launch
    constant on the call holds odd widths and shifted frames too, so one call mixes both paths."""
    shapes = [WIDE[(5 * i) % len(WIDE)] if i < PER_LAUNCH else SHAPES[(3 * i) % len(SHAPES)] for i in range(n)]
    ps = [pair(w, h, 3000 + i) for i, (w, h) in enumerate(shapes)]
    src, out = [p[0] for p in ps], [p[1] for p in ps]
    shifts = [0 if i < PER_LAUNCH else i % 2 for i in range(n)]
    rc, got = run_device(nq, src, out, 1, shifts)
    assert rc == 0
    same(got, compare_ref.compare_frames(src, out, 1), "n = %d" % n)
    if n == PER_LAUNCH + 1:
        same(np.stack([q.slots for q in nq.compare_frames(src, out)]), got, "host form")


def test_known_answers_through_the_library(nq):
    img = sample()
    src = [_full(16, 16, BLACK), _full(1, 1, BLACK), _checker(16, 16), img, _checker(16, 16)[:9, :9].copy()]
    out = [_full(16, 16, WHITE), _full(1, 1, WHITE), _checker(16, 16, WHITE, BLACK), img.copy(), _full(9, 9, BLACK)]
    q = nq.compare_frames(src, out)
    assert q[0].slots.tolist() == [256, 4, 0, 16646400, 16646400, 16646400, 255, 0, 17179344900, 17179344900, 17179344900, 12, 32765, 0, 0, 0]
    assert q[1].slots.tolist() == [1, 1, 0, 65025, 65025, 65025, 255, 0, 4294836225, 4294836225, 4294836225, 3, 32765, 0, 0, 0]
    assert q[2].slots.tolist() == [256, 4, 0, 16646400, 16646400, 16646400, 255, 0, 0, 0, 0, -130604, 65419, 0, 0, 0]
    want = np.zeros(16, np.int64)
    want[0], want[1], want[11] = 216810, 3410, 111738880
    assert q[3].slots.tolist() == want.tolist() and q[3].ssim == 1.0 and q[3].psnr == float("inf")
    assert q[4].pixels == 81 and q[4].blocks == 4 and q[4].deficit == 32768
    same(np.stack([r.slots for r in q]), compare_ref.compare_frames(src, out), "all five")


def test_one_frame_with_more_strips_than_the_grid_holds(nq):
    """GRID_CAP workgroups of WAVES waves take GRID_CAP * WAVES strips at a time; a frame of 8 strips per row and one row of strips more
    than that reaches the strip loop.  Its upper 512 rows are black against white, so that the sums pass 2^32 by far (the kernel's only
    32-bit partial sums are those of a lane's 32 pixels of one strip; everything a workgroup carries across strips is 64 bits wide)."""
    w = 8 * STRIP
    h = 8 * (GRID_CAP * WAVES // 8 + 1)
    assert (w // STRIP) * (h // 8) > GRID_CAP * WAVES and (w, h) == (2048, 2056)
    src, out = pair(w, h, 4242)
    src, out = src.copy(), out.copy()
    src[:512] = np.int32(BLACK - (1 << 32))
    out[:512] = -1
    want = compare_ref.compare(src, out, 1)
    assert want[3] > 1 << 34
    rc, got = run_device(nq, [src], [out], 1)
    assert rc == 0
    same(got, want[None], "2048 x 2056")


# ---- plumbing ----
def test_the_host_forms_give_back_their_device_memory(nq):
    src, out, ref = pairs(SHAPES)
    before = nq.device_bytes()
    same(np.stack([q.slots for q in nq.compare_frames(src, out, linear=False)]), ref[0], "host form")
    assert nq.device_bytes() == before


# ---- on a caller's stream ----
def test_on_a_callers_stream(nq):
    """The inputs are made true by copies queued on a side stream behind a gate spin; the call follows with no host wait and must return
    while the gate runs; the result is copied on that stream and checked after one synchronise."""
    import torch
    L = nq.load_library()
    stream = torch.cuda.Stream()
    cycles, ms = G.calibrate(stream)
    w, h, n = 48, 40, 3
    ps = [pair(w, h, 600 + i) for i in range(n)]
    src, out = [p[0] for p in ps], [p[1] for p in ps]
    want = compare_ref.compare_frames(src, out, 1)
    gate = G.Gate(stream, cycles)
    b_src = gate.input("argb", src, [G.invert_rgb(a) for a in src])
    b_out = gate.input("out_argb", out, [G.invert_rgb(a) for a in out])
    res = torch.full((GUARD + 16 * n + GUARD,), -7, dtype=torch.int64, device="cuda")
    snap = torch.empty_like(res)
    ws, hs = np.full(n, w, np.int32), np.full(n, h, np.int32)
    assert (compare_ref.compare_frames([G.invert_rgb(a) for a in src], out, 1) != want).any()      # the poison would show
    gate.arm(gate=False)                                # a first call of this shape loads the kernel: not under the gate
    assert L.nq_compare_frames_device(0, stream.cuda_stream, n, tab(b_src.ptrs), tab(b_out.ptrs), ws.ctypes.data, hs.ctypes.data, 1,
                                      res.data_ptr() + 8 * GUARD) == 0
    stream.synchronize()
    res.fill_(-7)
    gate.arm()
    rc = L.nq_compare_frames_device(0, stream.cuda_stream, n, tab(b_src.ptrs), tab(b_out.ptrs), ws.ctypes.data, hs.ctypes.data, 1,
                                    res.data_ptr() + 8 * GUARD)
    with torch.cuda.stream(stream):
        snap.copy_(res, non_blocking=True)
    gate.finish(True, "nq_compare_frames_device")
    assert rc == 0
    got = snap.cpu().numpy()
    assert (got[:GUARD] == -7).all() and (got[GUARD + 16 * n:] == -7).all()
    same(got[GUARD:GUARD + 16 * n].reshape(n, 16), want, "on a side stream")
    gate.check_inputs("nq_compare_frames_device")


# ---- end to end ----
_CONVERTED = {}


def converted(nq):
    if not _CONVERTED:
        from nquant.android_amd import synth
        frames = [synth.gradient_noise(64, 48, 11), synth.gradient_noise(64, 48, 12)]
        _CONVERTED["frames"] = frames
        _CONVERTED["result"] = nq.convert_frames(nq.NQ_KIND_LAB, frames, 16, True)
    return _CONVERTED["frames"], _CONVERTED["result"]


def test_a_conversion_measured_end_to_end(nq):
    frames, (palette, images) = converted(nq)
    want = compare_ref.compare_frames(frames, [im.argb for im in images], 1)
    same(np.stack([q.slots for q in nq.compare_frames(frames, [im.argb for im in images])]), want, "compare_frames")
    same(np.stack([q.slots for q in nq.compare_indexed(frames, [im.index for im in images], palette)]), want, "compare_indexed")
    assert 0 < want[0, 3] and want[0, 11] < 32768 * want[0, 1]


def test_choose_colors(nq):
    frames, _ = converted(nq)
    ladder = (4, 16, 64)
    K, palette, images, report, met = nq.choose_colors(nq.NQ_KIND_LAB, frames, ladder=ladder)
    assert (K, met) == (4, True) and list(report) == [4] and len(images) == 2 and palette.size <= 4
    # the reports of every K, from targets nobody reaches
    K, palette, images, full, met = nq.choose_colors(nq.NQ_KIND_LAB, frames, ladder=ladder, min_ssim=2.0)
    assert (K, met) == (64, False) and sorted(full) == list(ladder) and palette.size <= 64
    same(nq.Quality.total(nq.compare_frames(frames, [im.argb for im in images])).slots, full[64].slots, "the report of the last K")
    print({k: repr(q) for k, q in full.items()})
    for name, attr in (("min_psnr", "psnr"), ("min_ssim", "ssim"), ("min_lf_psnr", "lf_psnr")):
        values = {k: getattr(full[k], attr) for k in ladder}
        target = values[16]                              # what K = 16 reaches: the smallest K that meets it is 16, or a smaller one that does too
        K, palette, images, report, met = nq.choose_colors(nq.NQ_KIND_LAB, frames, ladder=ladder, **{name: target})
        assert met and getattr(report[K], attr) >= target
        assert K == min(k for k in ladder if values[k] >= target)
        assert all(getattr(report[k], attr) < target for k in report if k < K)
        assert sorted(report) == [k for k in ladder if k <= K]
        assert report[K].slots.tolist() == full[K].slots.tolist()       # deterministic
    best = max(full[k].psnr for k in ladder)
    K, _, _, report, met = nq.choose_colors(nq.NQ_KIND_LAB, frames, ladder=ladder, min_psnr=best + 1.0, min_ssim=0.0)
    assert (K, met) == (64, False) and sorted(report) == list(ladder)
