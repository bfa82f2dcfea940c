"""The ordered dither on the GPU (nq_dither_ordered_device / nq_dither_ordered / nq_convert_frames_ordered[_device]): index maps, ARGB
outputs and statistics equal the restatement in ordered_ref.py bit for bit, at the smallest shapes that reach each path of the kernel
(one pixel, a tail only, groups that straddle row ends, the mask period crossed on both axes, the four-pixel and the one-pixel path,
more groups than the grid holds in one round, more frames than workgroups), for n = 1, 3, 5 with mixed sizes, for palettes with
duplicates, pinned entries and no live entry; sources and the guard words around every output stay untouched; the host form equals the
device form; the convert form equals its three calls; every rejected argument leaves the buffers alone and the handle usable; and the
converters' ordered= keyword gives files that hold exactly these index maps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import apng_ref
import gif_delta_ref
import hold_ref
import ordered_ref as R
from conftest import ROOT
from nquant.android_amd import gif as G
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 24                                                     # elements between two frames of a buffer (a multiple of 8)
LIMITS = (0, 1, 40, 255)
SHAPES = [(1, 1), (5, 3), (67, 65), (130, 3), (4099, 2)]       # (width, height)


def _kernel_constants():
    """ORD_THREADS, ORD_MAX_BLOCKS and ORD_MIN_PIXELS as nq_ordered.hip defines them."""
    src = open(os.path.join(ROOT, "nquant.android_amd", "csrc", "nq_ordered.hip")).read()
    threads = int(re.search(r"constexpr int ORD_THREADS = (\d+);", src).group(1))
    blocks = int(re.search(r"constexpr long long ORD_MAX_BLOCKS = (\d+);", src).group(1))
    least = int(re.search(r"constexpr long long ORD_MIN_PIXELS = (\d+);", src).group(1))
    return threads, blocks, least


ORD_THREADS, ORD_MAX_BLOCKS, ORD_MIN_PIXELS = _kernel_constants()


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _frame(w, h, seed, alpha=True):
    img = synth.gradient_noise(w, h, seed)
    return synth.with_alpha(img, seed + 1, p_transparent=0.05, p_semi=0.1) if alpha else img


def _random_palette(K, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000)


_REF = {}


def _ref(key, frames, pal, limit):
    """The restatement's (index maps, ARGB outputs, stats) of a case, computed once."""
    if key not in _REF:
        _REF[key] = R.dither(frames, pal, limit)
    return _REF[key]


class _Stream:
    """Arrays of one element type (sizes may differ) in ONE device buffer, guard elements before, between and after them; array i
    starts `shift` elements behind a 16-byte boundary."""

    def __init__(self, arrays, shift, sentinel, dtype):
        import torch
        self.dtype = np.dtype(dtype)
        per16 = 16 // self.dtype.itemsize
        self.sizes = [int(np.asarray(a).size) for a in arrays]
        self.offs, at = [], GUARD
        for px in self.sizes:
            self.offs.append(at + shift)
            at += (px + per16 - 1) // per16 * per16 + GUARD
        self.host = np.full(at + per16, sentinel, self.dtype)
        self.fill(self.host, arrays)
        self.dev = torch.from_numpy(self.host.view(np.int16 if self.dtype.itemsize == 2 else np.int32).copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = [self.dev.data_ptr() + self.dtype.itemsize * o for o in self.offs]

    def fill(self, buf, arrays):
        for a, o, px in zip(arrays, self.offs, self.sizes):
            v = np.ascontiguousarray(a).reshape(-1)
            assert v.dtype.itemsize == self.dtype.itemsize
            buf[o:o + px] = v.view(self.dtype)

    def expect(self, arrays):
        want = self.host.copy()
        self.fill(want, arrays)
        return want

    def read(self):
        return self.dev.cpu().numpy().view(self.dtype)


def _device_case(nq, q, frames, pal, limit, want, shifts=(0, 0, 0), argb=True, stats=True, why=None):
    """One nq_dither_ordered_device call on guarded buffers; shifts: elements behind a 16-byte boundary of (sources, index maps, ARGB
    outputs).  Compares the whole buffers, guards included, and the statistics."""
    import torch
    widx, wout, wstats = want
    src = _Stream(frames, shifts[0], 0x55AA55AA, np.uint32)
    idx = _Stream([np.full(f.shape, 0xEEEE, np.uint16) for f in frames], shifts[1], 0xEEEE, np.uint16)
    out = _Stream([np.full(f.shape, 0x99999999, np.uint32) for f in frames], shifts[2], 0x99999999, np.uint32) if argb else None
    why = (why, [f.shape for f in frames][:6], len(frames), int(pal.size), limit, shifts, argb, stats)
    torch.cuda.synchronize()
    got = nq.dither_ordered_device(q, src.ptrs, [f.shape[1] for f in frames], [f.shape[0] for f in frames], pal, limit, idx.ptrs,
                                   out.ptrs if argb else None, return_stats=stats)
    torch.cuda.synchronize()
    gi = idx.read()
    assert (gi == idx.expect(widx)).all(), (why, int((gi != idx.expect(widx)).sum()))
    if argb:
        go = out.read()
        assert (go == out.expect(wout)).all(), (why, int((go != out.expect(wout)).sum()))
    assert (src.read() == src.host).all(), why
    if stats:
        assert got.tolist() == wstats.tolist(), why
    else:
        assert got is None


def _both_paths(nq, q, frames, pal, limit, want, why=None):
    _device_case(nq, q, frames, pal, limit, want, (0, 0, 0), why=why)             # the four-pixel path
    _device_case(nq, q, frames, pal, limit, want, (1, 1, 1), why=why)             # the one-pixel path


@pytest.fixture(scope="module")
def q(nq):
    quant = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    yield quant
    quant.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_frame_of_every_shape_on_both_paths(nq, q, shape):
    """1 x 1 and 5 x 3 are tail only on the four-pixel path (5 x 3: three whole groups and a tail of three); 67 x 65 crosses the mask
    period on both axes and its groups straddle row ends; 4099 x 2 has two workgroups' worth of groups."""
    w, h = shape
    frames = [_frame(w, h, 100 + w)]
    for K in (5, 64):
        pal = _random_palette(K, K + w)
        pal[1] &= np.uint32(0x00FFFFFF)
        for limit in (40, 255):
            _both_paths(nq, q, frames, pal, limit, _ref(("shape", shape, K, limit), frames, pal, limit))


@pytest.mark.parametrize("n", [1, 3, 5])
def test_several_frames_of_mixed_sizes_in_one_call(nq, q, n):
    frames = [_frame(w, h, 200 + i) for i, (w, h) in enumerate(SHAPES[:n])]
    if n == 5:
        frames = frames[::-1]
    pal = _random_palette(65, 7)
    for limit in (0, 255):
        _both_paths(nq, q, frames, pal, limit, _ref(("mixed", n, limit), frames, pal, limit))


def _palettes():
    out = {"K%d" % K: _random_palette(K, 300 + K) for K in (1, 2, 3, 5, 64, 65, 256)}
    dup = _random_palette(12, 31)
    dup[5] = dup[2]
    dup[9] = dup[2]
    dup[11] = dup[0]
    out["duplicates"] = dup
    first = _random_palette(16, 32)
    first[0] = 0x00FFFFFF
    out["clear-first"] = first
    mid = _random_palette(16, 33)
    mid[7] = 0x00102030
    mid[12] = 0x00000000
    out["clear-middle"] = mid
    out["all-clear"] = _random_palette(6, 34) & np.uint32(0x00FFFFFF)
    semi = np.random.default_rng(35).integers(0, 1 << 32, 40, dtype=np.uint64).astype(np.uint32) | np.uint32(0x01000000)
    out["semi"] = semi
    return out


PALETTES = _palettes()


@pytest.mark.parametrize("name", sorted(PALETTES))
def test_palettes_and_limits(nq, q, name):
    """A semi-transparent image (synth.with_alpha: alpha 0, in between and 255) and an opaque one, every limit."""
    pal = PALETTES[name]
    frames = [_frame(67, 65, 40), _frame(5, 3, 41, alpha=False)]
    for limit in LIMITS:
        want = _ref(("pal", name, limit), frames, pal, limit)
        _both_paths(nq, q, frames, pal, limit, want, name)
    if name in ("K5", "K64", "K256", "semi"):
        assert _REF[("pal", name, 255)][2][:, 0].sum() > 0                 # (something was mixed)


def test_an_index_pointer_that_is_2_byte_but_not_8_byte_aligned_takes_the_one_pixel_path(nq, q):
    frames = [_frame(67, 65, 40), _frame(5, 3, 41, alpha=False)]
    pal = PALETTES["K64"]
    want = _ref(("pal", "K64", 255), frames, pal, 255)
    for shifts in ((0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0), (1, 0, 0), (0, 0, 2), (2, 4, 2)):
        _device_case(nq, q, frames, pal, 255, want, shifts)


def test_outputs_are_the_same_with_and_without_argb_and_stats(nq, q):
    frames = [_frame(130, 3, 50), _frame(67, 65, 51)]
    pal = PALETTES["K65"]
    want = _ref(("outputs",), frames, pal, 40)
    for shifts in ((0, 0, 0), (1, 1, 1)):
        for argb in (True, False):
            for stats in (True, False):
                _device_case(nq, q, frames, pal, 40, want, shifts, argb, stats)


def test_more_groups_than_the_grid_holds_in_one_round(nq, q):
    """The grid is capped at ORD_MAX_BLOCKS = 2048 workgroups of ORD_THREADS = 256 lanes, which then stride over the groups: a frame of
    more than 4 * 2048 * 256 pixels gives every lane of the four-pixel path a second round, and the one-pixel path five."""
    assert (ORD_THREADS, ORD_MAX_BLOCKS, ORD_MIN_PIXELS) == (256, 2048, 1024)
    w = 2051
    h = 4 * ORD_MAX_BLOCKS * ORD_THREADS // w + 3
    assert w * h // 4 > ORD_MAX_BLOCKS * ORD_THREADS and w * h // ORD_MIN_PIXELS >= ORD_MAX_BLOCKS and w * h % 4 != 0
    frames = [synth.gradient_noise(w, h, 60)]
    pal = _random_palette(16, 61)
    _both_paths(nq, q, frames, pal, 255, _ref(("cap",), frames, pal, 255))


def test_more_frames_than_workgroups(nq, q):
    """3000 frames of 8 x 8: 192 000 pixels are 187 workgroups, each of which walks all 3000 table entries.  The frames repeat a pool of
    16, and equal frames have equal results (the index depends on the pixel, its coordinates and the palette only)."""
    n = 3000
    assert n * 64 // ORD_MIN_PIXELS < n
    pool = [_frame(8, 8, 70 + i) for i in range(16)]
    pal = PALETTES["clear-middle"]
    pidx, pout, pstats = R.dither(pool, pal, 255)
    pick = [i % 16 for i in range(n)]
    want = ([pidx[i] for i in pick], [pout[i] for i in pick], pstats[pick])
    _both_paths(nq, q, [pool[i] for i in pick], pal, 255, want)


def test_host_form_equals_the_device_form(nq):
    frames = [_frame(w, h, 200 + i) for i, (w, h) in enumerate(SHAPES)][::-1]
    pal = _random_palette(65, 7)
    for limit in (0, 255):
        widx, wout, wstats = _ref(("mixed", 5, limit), frames, pal, limit)       # (what the device form gave above)
        keep = [f.copy() for f in frames]
        images, stats = nq.dither_ordered(frames, pal, limit, return_stats=True)
        assert stats.tolist() == wstats.tolist()
        assert all((im.index == a).all() and (im.argb.view(np.uint32) == b).all() for im, a, b in zip(images, widx, wout))
        assert all((a == b).all() for a, b in zip(frames, keep))
        images = nq.dither_ordered(frames, pal, limit)
        assert all((im.index == a).all() and im.index.dtype == np.uint16 for im, a in zip(images, widx))


@pytest.mark.parametrize("kind", [0, 1])
def test_convert_form_equals_its_three_calls(nq, kind):
    import torch
    frames = [synth.gradient_noise(96, 80, 80 + i) for i in range(2)] + [_frame(40, 30, 83)]
    ws, hs = [f.shape[1] for f in frames], [f.shape[0] for f in frames]
    q = (nq.PnnLABQuantizer if kind else nq.PnnQuantizer)(frames[0])
    try:
        dev = [torch.from_numpy(f.copy()).cuda() for f in frames]
        src = [d.data_ptr() for d in dev]
        for nMax in (16, 256):
            for refine in (0, 2):
                pal = nq.pnnquan_frames_device(q, src, ws, hs, nMax)
                if refine:
                    pal = nq.refine_palette_device(q, src, ws, hs, pal, refine)[0]
                pal = np.asarray(pal).view(np.uint32)
                didx = [torch.zeros(f.size, dtype=torch.int16, device="cuda") for f in frames]
                dout = [torch.zeros(f.size, dtype=torch.int32, device="cuda") for f in frames]
                nq.dither_ordered_device(q, src, ws, hs, pal, 48, [d.data_ptr() for d in didx], [d.data_ptr() for d in dout])
                torch.cuda.synchronize()
                widx, wout, _ = R.dither(frames, pal, 48)
                assert all((d.cpu().numpy().view(np.uint16) == a.reshape(-1)).all() for d, a in zip(didx, widx))
                assert all((d.cpu().numpy().view(np.uint32) == a.reshape(-1)).all() for d, a in zip(dout, wout))
                # the device convert form, on fresh outputs
                cidx = [torch.full((f.size,), -1, dtype=torch.int16, device="cuda") for f in frames]
                cout = [torch.full((f.size,), -1, dtype=torch.int32, device="cuda") for f in frames]
                arr = lambda v: (C.c_void_p * len(v))(*v)
                cpal, K = np.zeros(256, np.uint32), C.c_int32(0)
                w32, h32 = np.array(ws, np.int32), np.array(hs, np.int32)
                rc = q._L.nq_convert_frames_ordered_device(q._h, len(frames), arr(src), w32.ctypes.data, h32.ctypes.data, nMax, refine, 48,
                                                           arr([d.data_ptr() for d in cout]), arr([d.data_ptr() for d in cidx]),
                                                           cpal.ctypes.data, C.byref(K))
                torch.cuda.synchronize()
                assert rc == 0 and K.value == pal.size and (cpal[:K.value] == pal).all(), (kind, nMax, refine)
                assert all((a.cpu() == b.cpu()).all() for a, b in zip(cidx, didx)) and all((a.cpu() == b.cpu()).all() for a, b in zip(cout, dout))
                # without the ARGB outputs
                for d in cidx: d.fill_(-1)
                rc = q._L.nq_convert_frames_ordered_device(q._h, len(frames), arr(src), w32.ctypes.data, h32.ctypes.data, nMax, refine, 48,
                                                           None, arr([d.data_ptr() for d in cidx]), cpal.ctypes.data, C.byref(K))
                torch.cuda.synchronize()
                assert rc == 0 and all((a.cpu() == b.cpu()).all() for a, b in zip(cidx, didx))
                # the host form
                hpal, outs = nq.convert_frames_ordered(kind, frames, nMax, 48, refine)
                assert (np.asarray(hpal).view(np.uint32) == pal).all()
                assert all((o.index == a).all() and (o.argb.view(np.uint32) == b).all() for o, a, b in zip(outs, widx, wout))
        assert all((d.cpu().numpy() == f).all() for d, f in zip(dev, frames))                 # the sources are only read
    finally:
        q.close()


def test_invalid_arguments_then_a_valid_call(nq, hd):
    import torch
    L = hd._L
    n, sizes = 3, [(12, 8), (5, 3), (7, 9)]
    frames = [_frame(w, h, 90 + i) for i, (w, h) in enumerate(sizes)]
    pal = PALETTES["clear-middle"]
    widx, wout, wstats = R.dither(frames, pal, 40)
    px = [f.size for f in frames]
    # buffers with room for an odd pointer behind the data; the outputs start as sentinels
    hs = [np.concatenate([f.reshape(-1).view(np.uint32), [0, 0]]).astype(np.uint32) for f in frames]
    hi = [np.full(p + 4, 0xEEEE, np.uint16) for p in px]
    ho = [np.full(p + 2, 0x99999999, np.uint32) for p in px]
    ds = [torch.from_numpy(a.view(np.int32)).cuda() for a in hs]
    di = [torch.from_numpy(a.view(np.int16)).cuda() for a in hi]
    do = [torch.from_numpy(a.view(np.int32)).cuda() for a in ho]
    hpal = pal.copy()

    def ptrs(host, which):
        arrs = {"src": (hs, ds), "idx": (hi, di), "out": (ho, do)}[which][0 if host else 1]
        return [a.ctypes.data if host else a.data_ptr() for a in arrs]

    def call(host, convert=False, n=n, w=None, h=None, K=None, limit=40, nMax=16, refine=1, src=0, idx=0, out=0, palette=0, stats=True,
             okay=0, edit=None):
        p = {k: ptrs(host, k) for k in ("src", "idx", "out")}
        if edit:
            edit(p)
        arr = lambda v: (C.c_void_p * len(v))(*v)
        a_src = arr(p["src"]) if src == 0 else src
        a_idx = arr(p["idx"]) if idx == 0 else idx
        a_out = arr(p["out"]) if out == 0 else out
        w32 = np.array([s[0] for s in sizes] if w is None else w, np.int32)
        h32 = np.array([s[1] for s in sizes] if h is None else h, np.int32)
        st = np.full(2 * 3, -5, np.int64)
        if convert:
            cpal, cK = np.full(256, 0x12345678, np.uint32), C.c_int32(-5)
            rc = getattr(L, "nq_convert_frames_ordered" if host else "nq_convert_frames_ordered_device")(
                hd._h, n, a_src, None if w == 0 else w32.ctypes.data, None if h == 0 else h32.ctypes.data, nMax, refine, limit, a_out, a_idx,
                None if palette is None else cpal.ctypes.data, None if okay is None else C.byref(cK))
            if rc != 0:
                assert (cpal == 0x12345678).all() and cK.value == -5
        else:
            rc = getattr(L, "nq_dither_ordered" if host else "nq_dither_ordered_device")(
                hd._h, n, a_src, None if w == 0 else w32.ctypes.data, None if h == 0 else h32.ctypes.data,
                None if palette is None else hpal.ctypes.data, int(pal.size) if K is None else K, limit, a_out, a_idx,
                st.ctypes.data if stats else None)
        torch.cuda.synchronize()
        return rc, st

    def state(host):
        if host:
            return [a.copy() for a in hs + hi + ho]
        return [x.cpu().numpy().copy() for x in ds + di + do]

    def valid(host):
        """A valid call gives the reference; then the outputs are put back to their sentinels for the rejected calls that follow."""
        rc, st = call(host)
        assert rc == 0 and st.tolist() == wstats.reshape(-1).tolist()
        got = state(host)
        for k in range(n):
            assert (got[k].view(np.uint32) == hs[k]).all()
            assert (got[n + k].view(np.uint16)[:px[k]] == widx[k].reshape(-1)).all() and (got[n + k].view(np.uint16)[px[k]:] == 0xEEEE).all()
            assert (got[2 * n + k].view(np.uint32)[:px[k]] == wout[k].reshape(-1)).all() and (got[2 * n + k].view(np.uint32)[px[k]:] == 0x99999999).all()
        for a in hi: a[:] = 0xEEEE
        for a in ho: a[:] = 0x99999999
        if not host:
            for d, a in zip(di, hi): d.copy_(torch.from_numpy(a.view(np.int16)))
            for d, a in zip(do, ho): d.copy_(torch.from_numpy(a.view(np.int32)))

    def null_entry(key):
        def edit(p): p[key][1] = None
        return edit

    def off_by(key, nbytes):
        def edit(p): p[key][2] += nbytes
        return edit

    def alias_index(p):             # index map 1 begins inside source 0
        p["idx"][1] = p["src"][0] + 4 * (px[0] - 2)

    def alias_out(p):               # output 2 begins inside index map 0
        p["out"][2] = p["idx"][0] + 4

    def same_index(p):              # index maps 0 and 2 overlap by one element
        p["idx"][2] = p["idx"][0] + 2 * (px[0] - 1)

    def same_out(p):                # outputs 0 and 1 are one buffer
        p["out"][1] = p["out"][0]

    shared = [{"n": 0}, {"n": -2}, {"w": [12, 0, 7]}, {"w": [12, 5, 65536]}, {"h": [0, 3, 9]}, {"h": [8, 65536, 9]}, {"h": [8, -1, 9]},
              {"n": 2, "w": [32768, 32768, 7], "h": [32768, 32768, 9]},         # 2^31 pixels: one more than the limit
              {"limit": -1}, {"limit": 256}, {"src": None}, {"idx": None}, {"w": 0}, {"h": 0},
              {"edit": null_entry("src")}, {"edit": null_entry("idx")}, {"edit": null_entry("out")},
              {"edit": off_by("src", 2)}, {"edit": off_by("src", 1)}, {"edit": off_by("out", 2)}, {"edit": off_by("out", 3)},
              {"edit": off_by("idx", 1)}, {"edit": off_by("idx", 3)},
              {"edit": alias_index}, {"edit": alias_out}, {"edit": same_index}, {"edit": same_out}]
    plain = [{"K": 0}, {"K": 257}, {"K": -1}, {"palette": None}]
    conv = [{"nMax": 257}, {"nMax": 0}, {"refine": -1}, {"refine": 65}, {"palette": None}, {"okay": None}]
    for host in (True, False):
        valid(host)
        for convert, bad in ((False, shared + plain), (True, shared + conv)):
            for kw in bad:
                before = state(host)
                rc, st = call(host, convert, **kw)
                assert rc == -1, (host, convert, kw)
                assert (st == -5).all(), (host, convert, kw)
                assert (L.nq_last_error(hd._h) or b"") != b""
                assert all((a == b).all() for a, b in zip(before, state(host))), (host, convert, kw)
                valid(host)
        # d_out_argb NULL as a whole is the form without outputs; the same source for every frame of one size is allowed
        before = state(host)
        rc, st = call(host, out=None)
        assert rc == 0 and st.tolist() == wstats.reshape(-1).tolist()
        got = state(host)
        assert all((a == b).all() for a, b in zip(before[2 * n:], got[2 * n:]))
        assert all((got[n + k].view(np.uint16)[:px[k]] == widx[k].reshape(-1)).all() for k in range(n))
        valid(host)


# ---- end to end: a sprite moving over a still background, no noise, no hold, no seeds ----
H, W, N, K = 80, 96, 4, 32


@pytest.fixture(scope="module")
def clip():
    back = synth.gradient_noise(W, H, 21)
    boxes = [(7 + 13 * i, 9 + 5 * i, 12, 12) for i in range(N)]
    frames = []
    for x, y, w, h in boxes:
        f = back.copy()
        f[y:y + h, x:x + w] = np.int32(-1 ^ 0x0000FF00)          # 0xFFFF00FF
        frames.append(f)
    return frames, boxes


def _inside(rect, boxes, i):
    x, y, w, h = rect
    ys, xs = np.nonzero(hold_ref.union_mask(H, W, boxes[i - 1], boxes[i]))
    return xs.min() <= x and x + w <= xs.max() + 1 and ys.min() <= y and y + h <= ys.max() + 1


def test_ordered_frames_to_delta_gif_and_apng_keep_only_the_sprite(nq, clip):
    frames, boxes = clip
    pal, outs = nq.convert_frames_ordered(1, frames, K, 32)
    maps = [o.index for o in outs]
    widx, wout, _ = R.dither(frames, np.asarray(pal).view(np.uint32), 32)
    assert all((m == a).all() for m, a in zip(maps, widx)) and all((o.argb.view(np.uint32) == a).all() for o, a in zip(outs, wout))
    assert any((widx[0] != R.dither(frames[:1], np.asarray(pal).view(np.uint32), 0)[0][0]).reshape(-1))          # (it does dither)
    data, gpal = nq.convert_frames_to_gif(1, frames, K, True, ordered=32, delta=True)
    assert (np.asarray(gpal) == np.asarray(pal)).all()
    canvases = gif_delta_ref.compose(data)
    assert len(canvases) == N and all((c == m).all() for c, m in zip(canvases, maps))
    _, _, parsed = gif_delta_ref.parse(data)
    for i in range(1, N):
        p = parsed[i]
        assert _inside((p["x"], p["y"], p["w"], p["h"]), boxes, i), (i, p["x"], p["y"], p["w"], p["h"])
    assert data == gif_delta_ref.encode(maps, pal)
    # dither, mode and tile take no part
    assert nq.convert_frames_to_gif(0 + 1, frames, K, False, ordered=32, delta=True, mode=nq.MODE_LOOKUP_ONLY, tile=(16, 16))[0] == data
    apng, apal, rects = nq.convert_frames_to_apng(1, frames, K, True, ordered=32, return_rects=True)
    assert (np.asarray(apal) == np.asarray(pal)).all()
    canvases = apng_ref.compose(apng)
    assert len(canvases) == N and all((c == apng_ref.rgba_of(m, pal)).all() for c, m in zip(canvases, maps))
    for i in range(1, N):
        assert _inside(tuple(rects[i].tolist()), boxes, i), (i, rects[i].tolist())


def test_the_keyword_combines_with_hold_lossy_refine_and_size(nq, clip):
    frames, boxes = clip
    pal, outs = nq.convert_frames_ordered(1, frames, K, 32, refine=2)
    data, gpal = nq.convert_frames_to_gif(1, frames, K, True, ordered=32, refine=2, delta=True)
    assert (np.asarray(gpal) == np.asarray(pal)).all() and data == gif_delta_ref.encode([o.index for o in outs], pal)
    held, _, _ = hold_ref.hold(frames, [o.index for o in outs], 3)
    data, _ = nq.convert_frames_to_gif(1, frames, K, True, ordered=32, refine=2, delta=True, hold=3)
    assert data == gif_delta_ref.encode(held, pal)
    small = nq.resample_frames(frames, (48, 40))
    want, wpal = nq.convert_frames_to_gif(1, small, K, True, ordered=32, delta=True, lossy=8)
    got, gpal = nq.convert_frames_to_gif(1, frames, K, True, ordered=32, delta=True, lossy=8, size=(48, 40))
    assert got == want and (np.asarray(gpal) == np.asarray(wpal)).all()
    spal, souts = nq.convert_frames_ordered(1, frames, K, 32, size=(48, 40))
    assert (np.asarray(spal) == np.asarray(wpal)).all() and souts[0].index.shape == (40, 48)
    # one palette per shot
    data, pals = nq.convert_shots_to_gif(1, frames, [0, 2], K, True, ordered=32)
    for (a, b), p in zip(((0, 2), (2, 4)), pals):
        assert (np.asarray(p) == np.asarray(nq.convert_frames_ordered(1, frames[a:b], K, 32)[0])).all()
    got = nq.convert_clip_to_gif(1, frames, K, True, ordered=32)
    assert got[0] == nq.convert_shots_to_gif(1, frames, got[2], K, True, ordered=32)[0]


def test_ordered_none_is_the_call_without_the_keyword(nq, clip):
    frames, _ = clip
    seeds = [5] * N
    assert nq.convert_frames_to_gif(1, frames, K, True, seeds=seeds, delta=True, ordered=None)[0] == \
        nq.convert_frames_to_gif(1, frames, K, True, seeds=seeds, delta=True)[0]
    assert nq.convert_frames_to_gif(1, frames, K, True, ordered=None)[0] == nq.convert_frames_to_gif(1, frames, K, True)[0]
    assert nq.convert_frames_to_gif(1, frames, K, True, delta=True, hold=3, refine=1, ordered=None)[0] == \
        nq.convert_frames_to_gif(1, frames, K, True, delta=True, hold=3, refine=1)[0]
    assert nq.convert_frames_to_apng(1, frames, K, True, seeds=seeds, ordered=None)[0] == nq.convert_frames_to_apng(1, frames, K, True, seeds=seeds)[0]
    assert nq.convert_shots_to_gif(1, frames, [0, 2], K, True, ordered=None)[0] == nq.convert_shots_to_gif(1, frames, [0, 2], K, True)[0]
    assert nq.convert_clip_to_gif(1, frames, K, True, ordered=None)[0] == nq.convert_clip_to_gif(1, frames, K, True)[0]
