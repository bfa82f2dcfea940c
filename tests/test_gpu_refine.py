"""Palette refinement on the GPU (nq_refine_palette* / nq_convert_frames_refined*): palette, every sse[j], counts and passes equal
the restatement in refine_ref.py exactly -- at the smallest shapes that reach each path of the kernel (one pixel, less than one
vector group, a tail, whole groups only, several workgroups), with 16-byte aligned frames (vector path) and frames offset by one
element (scalar path), frames of different sizes in one call, K = 1 .. 256; alpha (pinned entries, uncounted pixels, no live entry);
ties and empty entries; sums above 2^32; tens of thousands of small frames, which carry every workgroup through the flush inside
the round loop; the early stop; frames untouched; every rejected argument leaves the outputs alone and the
handle usable; convert_frames_refined is the composition of pnnquan_frames_device, the restatement and dither_device; and the GIF /
APNG wrappers pass `refine` on."""
import ctypes as C

import numpy as np
import pytest

import apng_ref
import gif_ref
import refine_ref
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 24                                                     # elements between two frames of a buffer (a multiple of 4)
SENTINEL = 0x5A5A5A5A
PARAM_FIELDS = ["kind", "nMaxColors", "hasSemiTransparency", "transparentPixelIndex", "transparentColor", "isNano", "texicab", "quan_rt",
                "maxbins", "paletteLength", "PR", "PG", "PB", "PA", "ratio", "weight"]


class _Stream:
    """Frames of any sizes in ONE device buffer, guard elements before, between and after them; every frame starts `shift` elements
    behind a 16-byte boundary."""

    def __init__(self, frames, shift):
        import torch
        offs, at = [], GUARD
        for f in frames:
            offs.append(at + shift)
            at += (f.size + 7) // 8 * 8 + GUARD
        self.host = np.full(at + 8, SENTINEL, np.uint32)
        for f, o in zip(frames, offs):
            self.host[o:o + f.size] = np.asarray(f).reshape(-1).view(np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = [self.dev.data_ptr() + 4 * o for o in offs]
        assert all(p % 16 == 4 * shift for p in self.ptrs)
        self.widths = [f.shape[1] for f in frames]
        self.heights = [f.shape[0] for f in frames]

    def unchanged(self):
        return (self.dev.cpu().numpy().view(np.uint32) == self.host).all()


@pytest.fixture(scope="module")
def q(nq):
    quant = nq.PnnLABQuantizer(np.zeros((2, 2), np.int32))
    yield quant
    quant.close()


def _opaque_palette(K, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000)


def _same(got, want, why):
    pal, sse, cnt, passes = got
    wpal, wsse, wcnt, wpasses = want
    assert pal.dtype == np.uint32 and sse.dtype == np.int64 and cnt.dtype == np.int64
    assert pal.tolist() == wpal.tolist(), why
    assert sse.tolist() == wsse.tolist(), why
    assert cnt.tolist() == wcnt.tolist(), why
    assert passes == wpasses, why


def _device_case(nq, q, frames, palette, iterations, why, want=None):
    """Both access paths against the restatement; the frames and the guard elements stay as they were.  Returns the restatement's result."""
    want = want or refine_ref.refine(frames, palette, iterations)
    for shift in (0, 1):
        s = _Stream(frames, shift)
        keep = np.array(palette).copy()
        got = nq.refine_palette_device(q, s.ptrs, s.widths, s.heights, palette, iterations)
        _same(got, want, (why, shift))
        assert (np.asarray(palette) == keep).all() and s.unchanged(), (why, shift)
    return want


SHAPES = ((1, 1), (3, 1), (5, 3), (257, 3), (64, 64), (96, 80))      # (width, height)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_equals_the_restatement_at_every_geometry(nq, q, shape):
    w, h = shape
    img = synth.gradient_noise(w, h, 3)
    for K in (1, 2, 255, 256):
        palette = _opaque_palette(K, 10 * w + K)
        for iterations in (0, 1, 6):
            want = _device_case(nq, q, [img], palette, iterations, (w, h, K, iterations))
            assert want[1].size == iterations + 1 and (np.diff(want[1]) <= 0).all()


def test_several_workgroups_and_rounds(nq, q):
    """300 x 200 is three workgroups on either path, with a last round that is not full; the second frame is two colours in stretches
    of 700 pixels: waves whose pixels all go to one entry beside waves that straddle a change."""
    img = synth.gradient_noise(300, 200, 4)
    two = np.where((np.arange(300 * 200) // 700) % 2 == 0, 0xFF102030, 0xFF10E030).astype(np.uint32).reshape(200, 300)
    for K in (16, 256):
        _device_case(nq, q, [img, two], _opaque_palette(K, K), 2, K)


def test_frames_of_three_sizes_in_one_call(nq, q):
    frames = [synth.gradient_noise(1, 1, 5), synth.uniform_rgb(7, 5, 6), synth.gradient_noise(64, 48, 7)]
    for iterations in (0, 1, 6):
        want = _device_case(nq, q, frames, _opaque_palette(16, 8), iterations, iterations)
        _same(nq.refine_palette(frames, _opaque_palette(16, 8), iterations), want, "host form")
    assert nq.palette_error(frames, _opaque_palette(16, 8)) == int(refine_ref.refine(frames, _opaque_palette(16, 8), 0)[1][0])


def test_one_misaligned_frame_takes_the_scalar_path_with_the_same_result(nq, q):
    import torch
    frames = [synth.gradient_noise(67, 5, 9 + i) for i in range(3)]
    palette = _opaque_palette(64, 9)
    want = refine_ref.refine(frames, palette, 3)
    bufs = [torch.from_numpy(np.concatenate([[SENTINEL] * 4, f.reshape(-1).view(np.uint32), [SENTINEL] * 4]).astype(np.uint32).view(np.int32)).cuda()
            for f in frames]
    ptrs = [b.data_ptr() + 16 for b in bufs]
    _same(nq.refine_palette_device(q, ptrs, [67] * 3, [5] * 3, palette, 3), want, "aligned")
    # frame 1 read one element early: its first pixel is the sentinel, its last one is left out
    ptrs[1] -= 4
    shifted = list(frames)
    shifted[1] = np.concatenate([[SENTINEL], frames[1].reshape(-1).view(np.uint32)[:-1]]).astype(np.uint32).reshape(5, 67)
    _same(nq.refine_palette_device(q, ptrs, [67] * 3, [5] * 3, palette, 3), refine_ref.refine(shifted, palette, 3), "one frame off")


def test_alpha_pinned_entries_and_uncounted_pixels(nq, q):
    img = synth.with_alpha(synth.gradient_noise(96, 80, 11), 11)
    al = img.view(np.uint32) >> 24
    assert (al == 0).any() and ((al > 15) & (al < 0xE0)).any()
    rng = np.random.default_rng(12)
    palette = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32) | np.uint32(0x01000000)
    palette[0] &= np.uint32(0x00FFFFFF)                         # pinned entries: the first one and one in the middle
    palette[17] = np.uint32(0x00808080)
    want = _device_case(nq, q, [img], palette, 4, "alpha")
    pal, sse, cnt, passes = want
    assert pal[0] == palette[0] and pal[17] == palette[17] and cnt[0] == cnt[17] == 0
    assert ((pal >> 24) == (palette >> 24)).all() and cnt.sum() == int((al != 0).sum())
    # a frame whose pixels all have alpha 0; beside a counted frame, and alone
    clear = (synth.gradient_noise(33, 9, 13).view(np.uint32) & np.uint32(0x00FFFFFF)).reshape(9, 33)
    _device_case(nq, q, [clear, img], palette, 2, "clear + alpha")
    want = _device_case(nq, q, [clear], palette, 3, "clear")
    assert (want[0] == palette).all() and (want[1] == 0).all() and want[3] == 1
    # a palette with no live entry
    want = _device_case(nq, q, [img], np.array([0x00123456, 0x00FFFFFF], np.uint32), 3, "no live entry")
    assert want[0].tolist() == [0x00123456, 0x00FFFFFF] and (want[1] == 0).all() and (want[2] == 0).all() and want[3] == 1


def test_ties_go_to_the_lower_index_and_empty_entries_stay(nq, q):
    img = synth.gradient_noise(64, 64, 14)
    palette = _opaque_palette(8, 15)
    palette[5] = palette[2]                                     # duplicates: the lower index takes every pixel
    palette = np.concatenate([palette, np.array([0x10FFFFFF], np.uint32)])     # far from every (opaque) pixel
    pal, sse, cnt, passes = _device_case(nq, q, [img], palette, 0, "ties, measured")
    assert cnt[2] > 0 and cnt[5] == 0 and cnt[8] == 0
    # the update moves entry 2 away from its twin, which got nothing and stays (and may get pixels in the next pass)
    pal, sse, cnt, passes = _device_case(nq, q, [img], palette, 1, "ties")
    assert pal[5] == palette[5] and pal[2] != palette[2]
    assert cnt[8] == 0 and pal[8] == 0x10FFFFFF


def test_sums_wider_than_32_bits(nq, q):
    """One flat opaque-white 4096 x 4200 frame against the entry 0xFF000000: the channel sum is 4.39e9.  The expected values are the
    closed form."""
    import torch
    w, h = 4096, 4200
    frame = torch.full((h * w,), -1, dtype=torch.int32, device="cuda")
    assert frame.data_ptr() % 16 == 0
    for ptr, hh in ((frame.data_ptr(), h), (frame.data_ptr() + 4, h)):      # the vector path; the scalar path, one pixel short of the buffer
        ww = w if ptr % 16 == 0 else w - 1
        pal, sse, cnt, passes = nq.refine_palette_device(q, [ptr], [ww], [hh], np.array([0xFF000000], np.uint32), 1)
        n = ww * hh
        assert cnt.tolist() == [n] and sse.tolist() == [3 * 65025 * n, 0] and pal.tolist() == [0xFFFFFFFF] and passes == 2
        if ww == w:
            assert n == 17203200 and 255 * n > 2**32
    assert bool((frame == -1).all())


# ---- the flush inside the round loop, in the kernel as it ships ----
FLUSH_PIXELS, REF_THREADS = 1 << 24, 256            # nq_refine.hip's values; test_refine_cpu.py holds the source to them
MANY = {"vector": (0, 40000, 4), "scalar": (1, 140000, 1)}      # path: elements behind a 16-byte boundary, frames, pixels per lane and round
DRAW = (0.25, 0.25, 0.10, 0.20, 0.20)               # how often the table names each of the first five frames of the pool
MARK, MARK_ENTRY = 0x01285AC8, 0x013C46B4           # the marker frame's one colour (alpha 1; b = 200) and the palette entry only it reaches


def _pool():
    """Five small frames: 64 x 32 is 512 vector groups (two workgroups with all four waves counting); 33 x 31 is 255 groups and a tail
    of 3; 1 x 1 is a tail alone; 16 x 16 of one colour takes the wave-match add; 9 x 7 holds pixels with alpha 0 (its other pixels are
    opaque: the marker's entry must stay the marker's).  The sixth is the marker, 64 x 32 of MARK."""
    pool = [synth.gradient_noise(64, 32, 41), synth.gradient_noise(33, 31, 42), synth.gradient_noise(1, 1, 43),
            np.full((16, 16), 0xFF2060A0, np.uint32), synth.with_alpha(synth.gradient_noise(9, 7, 44), 44, p_transparent=0.1, p_semi=0.0),
            np.full((32, 64), MARK, np.uint32)]
    al = pool[4].view(np.uint32) >> 24
    assert (al == 0).any() and (al == 255).any() and ((al == 0) | (al == 255)).all()
    return pool


@pytest.mark.parametrize("K,iterations", [(16, 0), (16, 3), (256, 1)])
@pytest.mark.parametrize("path", sorted(MANY))
def test_many_small_frames_pass_the_flush_inside_the_round_loop(nq, q, path, K, iterations):
    """The cap: a workgroup flushes its 32-bit LDS counters inside the round loop once `seen` would pass REF_FLUSH_PIXELS = 2^24, and
    `seen` grows by REF_THREADS * G = 1024 (vector path) or 256 (scalar path) per round whether or not the round's lanes hold pixels.
    A frame of G pixels or more costs every workgroup at least one round, so the number of frames alone carries a workgroup past the
    flush: it comes at the top of round 16 384 and 32 768 (counted from 0) on the vector path, 65 536 and 131 072 on the scalar path.
    40 000 frames x 1024 = 40 960 000 and 140 000 x 256 = 35 840 000 both exceed 2 x 2^24 = 33 554 432; the 1 x 1 frames, which cost the
    vector path no round (0 groups; workgroup 0 a tail round), are drawn less often than the others so that the frames that do cost
    one, counted below, still exceed 32 768.  Workgroup 0 adds a round per frame with a tail and so flushes at other rounds than the rest.
    The table names five frames of one small buffer in a seeded random order, so the round in front of a flush is not always the same
    frame's.  Exact against refine_weighted (test_refine_cpu.py holds that equal to refine() of the expanded sequence).

    What makes a lost add visible.  Every frame of the pool occurs thousands of times, and the outputs are counts, errors and ROUNDED
    means: one LDS add lost in front of a flush (the failure DESIGN.md 5d records: the b sums of the round before) moves no mean of
    such an entry.  So the round in front of each flush of the workgroups other than 0 (on the scalar path: of all of them) is the
    marker: a flat frame that occurs only there, whose pixels are the only ones its palette entry gets.  One wave's b sum less and
    that entry's blue drops by 200 * 256 / 4096 = 12 (vector path; the marker's groups 256 .. 511 are workgroup 1's) or by 200 * 64 /
    4096 = 3 (scalar path; 256 pixels each for workgroups 0 .. 7), which the palette and sse[1..] show for iterations >= 1."""
    shift, n, G = MANY[path]
    assert n * REF_THREADS * G > 2 * FLUSH_PIXELS
    pool = _pool()
    sizes = np.array([f.size for f in pool])
    order = np.random.default_rng(n).choice(5, n, p=DRAW)
    # the marker in front of both flushes: the frame that is round 16 384 k - 1 (65 536 k - 1) of the workgroups other than 0 costs them
    # a round, and so does the marker that takes its place
    between = FLUSH_PIXELS // (REF_THREADS * G)
    cost = np.cumsum(sizes[order] >= G)
    slots = [int(np.flatnonzero(cost == between * k)[0]) for k in (1, 2)]
    order[slots] = 5
    assert (np.cumsum(sizes[order] >= G) == cost).all() and slots[1] < n - 1
    weights = np.bincount(order, minlength=len(pool))
    assert (weights > 0).all() and weights[5] == 2
    # rounds of a workgroup other than 0 (one per frame with a whole group: 512 groups are one round of two workgroups or more), and
    # of workgroup 0, which also takes the tails
    rounds = int(weights[sizes >= G].sum())
    rounds0 = rounds + int(weights[sizes % G != 0].sum())
    assert rounds * REF_THREADS * G > 2 * FLUSH_PIXELS
    assert rounds0 > rounds if G > 1 else rounds0 == rounds == n
    assert int((weights * sizes).sum()) // 16384 >= 8          # (launch_refine: eight workgroups at the least)
    palette = _opaque_palette(K, 50 + K)
    palette[K - 1] = MARK_ENTRY
    want = refine_ref.refine_weighted(pool, weights, palette, iterations)
    assert iterations == 0 or want[3] > 1                      # an update after a flushed pass is part of the result
    assert want[2][K - 1] == 2 * 2048 and (iterations == 0 or want[0][K - 1] == MARK)      # the marker's pixels and no others
    s = _Stream(pool, shift)
    ptrs = [s.ptrs[i] for i in order]
    keep = palette.copy()
    got = nq.refine_palette_device(q, ptrs, [s.widths[i] for i in order], [s.heights[i] for i in order], palette, iterations)
    _same(got, want, (path, K, iterations))
    assert int(got[2].sum()) == int((weights * [int(((f.view(np.uint32) >> 24) != 0).sum()) for f in pool]).sum())
    assert (palette == keep).all() and s.unchanged()


def test_a_fixed_point_stops_after_one_pass(nq, q):
    img = synth.few_colors(64, 40, 16, 7)
    palette = np.unique(img.view(np.uint32))
    want = _device_case(nq, q, [img], palette, 64, "fixed point")
    assert want[3] == 1 and (want[1] == 0).all() and want[1].size == 65 and (want[0] == palette).all()


def test_invalid_arguments_then_a_valid_call(nq, q):
    import torch
    L = q._L
    frames = [synth.gradient_noise(6, 4, 17 + i) for i in range(3)]
    n = len(frames)
    palette = _opaque_palette(4, 18)
    want = refine_ref.refine(frames, palette, 2)
    hs = [np.concatenate([f.reshape(-1).view(np.uint32), [0, 0]]).astype(np.uint32) for f in frames]      # room for a 2-byte-off pointer
    ds = [torch.from_numpy(a.view(np.int32)).cuda() for a in hs]

    def call(host, n=n, w=(6,) * 3, h=(4,) * 3, K=4, it=2, src=0, edit=None, pal=0, sse=0, passes=0, ptrs=None):
        p = ptrs or ([a.ctypes.data for a in hs] if host else [d.data_ptr() for d in ds])
        if edit:
            edit(p)
        a_src = (C.c_void_p * len(p))(*p) if src == 0 else src
        o_pal = np.full(260, SENTINEL, np.uint32)
        o_pal[:4] = palette
        o_sse, o_cnt, o_passes = np.full(70, -5, np.int64), np.full(260, -5, np.int64), C.c_int32(-5)
        a_w, a_h = np.array(w, np.int32), np.array(h, np.int32)
        rc = getattr(L, "nq_refine_palette" if host else "nq_refine_palette_device")(
            q._h, n, a_src, a_w.ctypes.data, a_h.ctypes.data, None if pal is None else o_pal.ctypes.data,
            K, it, None if sse is None else o_sse.ctypes.data, o_cnt.ctypes.data, None if passes is None else C.byref(o_passes))
        return rc, o_pal, o_sse, o_cnt, o_passes.value

    def state(host):
        return [a.copy() for a in hs] if host else [d.cpu().numpy().copy() for d in ds]

    def valid(host):
        rc, o_pal, o_sse, o_cnt, o_passes = call(host)
        assert rc == 0 and o_pal[:4].tolist() == want[0].tolist() and (o_pal[4:] == SENTINEL).all()
        assert o_sse[:3].tolist() == want[1].tolist() and (o_sse[3:] == -5).all()
        assert o_cnt[:4].tolist() == want[2].tolist() and (o_cnt[4:] == -5).all() and o_passes == want[3]

    def null_entry(p): p[1] = None

    def off_by(nbytes):
        def edit(p): p[2] += nbytes
        return edit

    assert 4 * 65535 * 8193 > 2**31 - 1 >= 3 * 65535 * 8193
    for host in (True, False):
        one = [hs[0].ctypes.data if host else ds[0].data_ptr()]
        bad = [{"it": -1}, {"it": 65}, {"K": 0}, {"K": 257}, {"n": 0}, {"n": -2}, {"w": (6, 0, 6)}, {"h": (4, 4, 0)}, {"w": (65536, 6, 6)},
               {"src": None}, {"edit": null_entry}, {"edit": off_by(2)}, {"edit": off_by(1)}, {"pal": None}, {"sse": None}, {"passes": None},
               # rejected from the sizes alone: the one small frame stands in for all four and is never read
               {"n": 4, "w": (65535,) * 4, "h": (8193,) * 4, "ptrs": one * 4}]
        valid(host)
        for kw in bad:
            before = state(host)
            rc, o_pal, o_sse, o_cnt, o_passes = call(host, **kw)
            assert rc == -1, (host, kw)
            assert o_pal[:4].tolist() == palette.tolist() and (o_pal[4:] == SENTINEL).all() and (o_sse == -5).all() and (o_cnt == -5).all() \
                and o_passes == -5, (host, kw)
            assert (L.nq_last_error(q._h) or b"") != b""
            assert all((a == b).all() for a, b in zip(before, state(host))), (host, kw)
            valid(host)
    # out_counts may be NULL
    sse, passes, pal = np.zeros(3, np.int64), C.c_int32(0), palette.copy()
    src = (C.c_void_p * n)(*[d.data_ptr() for d in ds])
    a_w, a_h = np.array((6,) * 3, np.int32), np.array((4,) * 3, np.int32)
    assert L.nq_refine_palette_device(q._h, n, src, a_w.ctypes.data, a_h.ctypes.data, pal.ctypes.data, 4, 2, sse.ctypes.data, None, C.byref(passes)) == 0
    assert pal.tolist() == want[0].tolist() and sse.tolist() == want[1].tolist() and passes.value == want[3]


# ---- convert_frames_refined: pnnquan_frames_device, the passes, dither_device ----
def _convert_frames():
    return [synth.gradient_noise(64, 48, 20 + i) for i in range(3)]


@pytest.mark.parametrize("dither", [True, False], ids=["dither", "nodither"])
@pytest.mark.parametrize("K", [16, 256])
@pytest.mark.parametrize("kind", [0, 1], ids=["rgb", "lab"])
def test_convert_frames_refined_is_the_composition(nq, kind, K, dither):
    import torch
    frames = _convert_frames()
    seeds = [31, 32, 33]
    cls = nq.PnnLABQuantizer if kind else nq.PnnQuantizer
    # refine = 0: convert_frames, in every output
    pal0, outs0 = nq.convert_frames(kind, frames, K, dither, seeds=seeds)
    pal, outs = nq.convert_frames_refined(kind, frames, K, dither, 0, seeds=seeds)
    assert (pal == pal0).all()
    for a, b in zip(outs, outs0):
        assert (a.index == b.index).all() and (a.argb == b.argb).all()
    # refine = 4
    s = _Stream(frames, 0)
    qp = cls(frames[0])
    qr = cls(frames[0])
    try:
        base = nq.pnnquan_frames_device(qp, s.ptrs, s.widths, s.heights, K)
        assert (base == pal0).all()
        want_pal = refine_ref.refine(frames, base, 4)[0]
        assert (want_pal != base.view(np.uint32)).any()
        out = [torch.zeros(f.size, dtype=torch.int32, device="cuda") for f in frames]
        idx = [torch.zeros(f.size, dtype=torch.int16, device="cuda") for f in frames]
        src = (C.c_void_p * 3)(*s.ptrs)
        dst = (C.c_void_p * 3)(*[t.data_ptr() for t in out])
        didx = (C.c_void_p * 3)(*[t.data_ptr() for t in idx])
        got_pal, got_K = np.zeros(max(K, 2), np.int32), C.c_int32(0)
        a_w, a_h, a_seeds = np.array(s.widths, np.int32), np.array(s.heights, np.int32), np.array(seeds, np.int64)
        qr._check(qr._L.nq_convert_frames_refined_device(qr._h, 3, src, a_w.ctypes.data, a_h.ctypes.data, K, 4, int(dither),
                                                         a_seeds.ctypes.data, nq.MODE_PARALLEL_TILED, dst, didx,
                                                         got_pal.ctypes.data, C.byref(got_K)))
        torch.cuda.synchronize()
        got_pal = got_pal[:got_K.value]
        assert (got_pal.view(np.uint32) == want_pal).all()
        for f in PARAM_FIELDS:
            assert getattr(qr.params, f) == getattr(qp.params, f), f
        # every frame: those params, that palette, that seed through the stand-alone dither
        for i, f in enumerate(frames):
            qi = cls(f)
            try:
                qi.set_params(qr.params)
                o = torch.zeros(f.size, dtype=torch.int32, device="cuda")
                x = torch.zeros(f.size, dtype=torch.int16, device="cuda")
                qi.dither_device(s.ptrs[i], got_pal, dither, o.data_ptr(), x.data_ptr(), seed=seeds[i])
                torch.cuda.synchronize()
                assert bool((o == out[i]).all()) and bool((x == idx[i]).all()), i
            finally:
                qi.close()
        assert s.unchanged()
        # the host form gives the same
        pal4, outs4 = nq.convert_frames_refined(kind, frames, K, dither, 4, seeds=seeds)
        assert (pal4.view(np.uint32) == want_pal).all()
        for i, o in enumerate(outs4):
            assert (o.argb.reshape(-1) == out[i].cpu().numpy()).all() and (o.index.reshape(-1) == idx[i].cpu().numpy().view(np.uint16)).all(), i
    finally:
        qp.close()
        qr.close()


def test_convert_frames_refined_rejects_bad_refine(nq):
    frames = _convert_frames()
    with pytest.raises(ValueError):
        nq.convert_frames_refined(1, frames, 16, True, 65)
    with pytest.raises(ValueError):
        nq.convert_frames_refined(1, frames, 16, True, -1)
    with pytest.raises(nq.NqError) as e:
        nq.convert_frames_refined(1, frames, 300, True, 2)
    assert e.value.status == -1
    pal, outs = nq.convert_frames_refined(1, frames, 300, True, 0)      # (refine = 0 keeps convert_frames' range)
    assert len(outs) == 3


# ---- the wrappers pass `refine` on ----
def test_gif_and_apng_with_refine(nq):
    frames = _convert_frames()
    seeds = [5, 5, 5]
    for kind in (0, 1):
        pal, outs = nq.convert_frames_refined(kind, frames, 64, True, 4, seeds=seeds)
        data, got_pal = nq.convert_frames_to_gif(kind, frames, 64, True, seeds=seeds, refine=4)
        assert (got_pal == pal).all()
        screen, table, gframes = gif_ref.parse(data)
        rgb = (pal.view(np.uint32)[:, None] >> np.array([16, 8, 0], np.uint32)) & 255
        assert bytes(table[:3 * len(pal)]) == rgb.astype(np.uint8).tobytes()
        assert len(gframes) == 3 and all((g["index"] == o.index).all() for g, o in zip(gframes, outs))
        a, pa = nq.convert_frames_to_gif(kind, frames, 64, True, seeds=seeds, refine=0)
        b, pb = nq.convert_frames_to_gif(kind, frames, 64, True, seeds=seeds)
        assert a == b and (pa == pb).all() and a != data

        data, got_pal = nq.convert_frames_to_apng(kind, frames, 64, True, seeds=seeds, refine=4)
        assert (got_pal == pal).all()
        canvases = apng_ref.compose(data)
        assert len(canvases) == 3 and all((c == apng_ref.rgba_of(o.index, pal)).all() for c, o in zip(canvases, outs))
        a, pa = nq.convert_frames_to_apng(kind, frames, 64, True, seeds=seeds, refine=0)
        b, pb = nq.convert_frames_to_apng(kind, frames, 64, True, seeds=seeds)
        assert a == b and (pa == pb).all() and a != data

    # per shot, over that shot's frames
    clip = frames + [synth.uniform_rgb(64, 48, 40 + i) for i in range(2)]
    data, palettes = nq.convert_shots_to_gif(1, clip, [0, 3], 64, True, seeds=[5] * 5, refine=4)
    assert (palettes[0] == nq.convert_frames_refined(1, clip[:3], 64, True, 4, seeds=[5] * 3)[0]).all()
    assert (palettes[1] == nq.convert_frames_refined(1, clip[3:], 64, True, 4, seeds=[5] * 2)[0]).all()
    plain, _ = nq.convert_shots_to_gif(1, clip, [0, 3], 64, True, seeds=[5] * 5)
    same, _ = nq.convert_shots_to_gif(1, clip, [0, 3], 64, True, seeds=[5] * 5, refine=0)
    assert plain == same and plain != data
    data2, palettes2, starts = nq.convert_clip_to_gif(1, clip, 64, True, cut=60, min_shot=1, seeds=[5] * 5, refine=4)
    assert starts == [0, 3] and data2 == data and all((a == b).all() for a, b in zip(palettes2, palettes))
