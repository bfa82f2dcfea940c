"""One palette for a sequence of frames (nq_pnnquan_frames_device / nq_convert_frames_device / nq_convert_frames): the palette and
params equal the oracle's pnnquan of the concatenated frames, every frame equals the oracle's dither of that frame with the shared
palette and params, n = 1 equals nq_convert_device in every output."""
import ctypes as C

import numpy as np
import pytest

from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

SEQ, TILED, LOOKUP = 0, 1, 2
PARAM_FIELDS = ["kind", "nMaxColors", "hasSemiTransparency", "transparentPixelIndex", "transparentColor", "isNano", "texicab", "quan_rt",
                "maxbins", "paletteLength", "PR", "PG", "PB", "PA", "ratio", "weight"]


def _copy_params(src, dst_cls):
    p = dst_cls()
    for f, _ in dst_cls._fields_:
        setattr(p, f, getattr(src, f))
    return p


def _cls(nq, kind):
    return nq.PnnLABQuantizer if kind else nq.PnnQuantizer


class _DevFrames:
    """The frames in ONE device buffer with a one-pixel gap after each: frame pointers are 4-byte aligned only (the frame passes'
    scalar heads and tails), and the frames are not a contiguous copy of the sequence."""

    def __init__(self, frames):
        import torch
        self.shapes = [f.shape for f in frames]
        self.offsets, off = [], 0
        for f in frames:
            self.offsets.append(off)
            off += f.size + 1
        host = np.full(off, 0x7F00FF00, np.int32)
        for f, o in zip(frames, self.offsets):
            host[o:o + f.size] = f.reshape(-1)
        self.buf = torch.from_numpy(host).cuda()
        self.out = torch.zeros(off, dtype=torch.int32, device="cuda")
        self.idx = torch.zeros(off, dtype=torch.int16, device="cuda")
        self.widths = [s[1] for s in self.shapes]
        self.heights = [s[0] for s in self.shapes]

    def ptrs(self, t):
        return [t.data_ptr() + 4 * o if t.element_size() == 4 else t.data_ptr() + 2 * o for o in self.offsets]

    def result(self, i):
        import torch
        torch.cuda.synchronize()
        o, (h, w) = self.offsets[i], self.shapes[i]
        return (self.out[o:o + h * w].cpu().numpy().reshape(h, w), self.idx[o:o + h * w].cpu().numpy().view(np.uint16).reshape(h, w))

    def guard_intact(self):
        import torch
        torch.cuda.synchronize()
        return all(int(self.buf[o + h * w]) == 0x7F00FF00 for o, (h, w) in zip(self.offsets, self.shapes))


def _oracle_sequence(oracle, kind, frames, K):
    """Oracle pnnquan of the concatenated sequence, laid out as one column (pnnquan reads only the pixel sequence)."""
    concat = np.concatenate([f.reshape(-1) for f in frames]).reshape(-1, 1)
    oq = oracle.OracleQuantizer(kind, concat)
    oq.prescan(K)
    pal = oq.pnnquan(K)
    return oq, pal


def _assert_params(got, want, distinct=False):
    for f in PARAM_FIELDS + (["distinctColors"] if distinct else []):
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))


def _auto_tile(w, h):
    t = 8 if ((w + 7) // 8) * ((h + 7) // 8) >= 131072 else 4
    return (min(t, w), min(t, h))


def _semi(img, seed, every=13):
    """img with every `every`-th pixel semi-transparent (alpha 0x80), no alpha == 0 pixel."""
    u = img.view(np.uint32).reshape(-1).copy()
    sel = np.arange(u.size) % every == seed % every
    u[sel] = (u[sel] & np.uint32(0xFFFFFF)) | np.uint32(0x80000000)
    return u.view(np.int32).reshape(img.shape)


def _few(w, h, colours, seed):
    z = synth.splitmix64(seed, w * h)
    pick = (z % np.uint64(len(colours))).astype(np.int64)
    return np.asarray(colours, np.uint32)[pick].view(np.int32).reshape(h, w)


def _colour_set(n, seed):
    z = synth.splitmix64(seed, n)
    return [0xFF000000 | (int(v) & 0xFFFFFF) for v in z]


# ---------------------------------------------------------------------------------------------------------------------------------
# n = 1: nq_convert_device in every output
# ---------------------------------------------------------------------------------------------------------------------------------
N1_CASES = [  # kind, K, dither, image
    (1, 256, True, lambda: synth.gradient_noise(96, 80, 1)),
    (1, 256, False, lambda: synth.gradient_noise(96, 80, 2)),        # BlueNoise post-pass: the weight from distinctColors
    (0, 64, True, lambda: synth.uniform_rgb(80, 64, 3)),
    (1, 2, True, lambda: synth.with_alpha(synth.gradient_noise(64, 48, 4), 4)),   # nMaxColors <= 2 rewrite
]


@pytest.mark.parametrize("kind,K,dither,mk", N1_CASES)
def test_one_frame_equals_convert_device(nq, kind, K, dither, mk):
    import torch
    img = mk()
    h, w = img.shape
    seed = 21
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    outs = [torch.zeros(w * h, dtype=torch.int32, device="cuda") for _ in range(2)]
    idxs = [torch.zeros(w * h, dtype=torch.int16, device="cuda") for _ in range(2)]
    q1 = _cls(nq, kind)(img, mode=TILED, seed=seed)
    pal1 = q1.convert_device(d_img.data_ptr(), K, dither, outs[0].data_ptr(), idxs[0].data_ptr())
    q2 = _cls(nq, kind)(img, mode=TILED, seed=seed)
    pal2 = nq.convert_frames_device(q2, [d_img.data_ptr()], [w], [h], K, dither, [outs[1].data_ptr()], [idxs[1].data_ptr()], seeds=[seed])
    torch.cuda.synchronize()
    assert len(pal1) == len(pal2) and (pal1 == pal2).all()
    _assert_params(q2.params, q1.params, distinct=True)
    assert torch.equal(outs[0], outs[1]) and torch.equal(idxs[0], idxs[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# palette + params vs the oracle's pnnquan of the concatenated sequence
# ---------------------------------------------------------------------------------------------------------------------------------
def _alpha_early_frames():
    """The last alpha == 0 pixel lies in frame 0, the last semi-transparent pixel in frame 2."""
    f0 = synth.with_alpha(synth.gradient_noise(40, 30, 31), 31, p_transparent=0.02, p_semi=0.0)
    f1 = synth.gradient_noise(37, 29, 32)
    f2 = _semi(synth.gradient_noise(41, 23, 33), 33)
    return [f0, f1, f2]


PAL_CASES = [  # name, kind, K, frames, compare distinctColors (the few-colours path counts the sequence)
    ("lab256_equal", 1, 256, lambda: [synth.gradient_noise(64, 48, 100 + i) for i in range(8)], False),
    ("lab256_odd_sizes", 1, 256, lambda: [synth.gradient_noise(97, 64, 5), synth.gradient_noise(64, 81, 6), synth.uniform_rgb(33, 17, 7),
                                          synth.uniform_rgb(1, 5, 8)], False),
    ("rgb256", 0, 256, lambda: [synth.uniform_rgb(53, 47, 9), synth.gradient_noise(64, 48, 10), synth.uniform_rgb(31, 7, 11)], False),
    ("lab64_alpha_early", 1, 64, _alpha_early_frames, False),
    ("lab64_transparent_only", 1, 64, lambda: [synth.gradient_noise(45, 31, 40), synth.with_alpha(synth.gradient_noise(39, 27, 41), 41, 0.03, 0.0),
                                              synth.gradient_noise(35, 21, 42)], False),
    ("lab256_semi", 1, 256, lambda: [synth.with_alpha(synth.gradient_noise(48, 40, 50 + i), 50 + i) for i in range(3)], False),
    ("rgb64_semi", 0, 64, lambda: [synth.with_alpha(synth.uniform_rgb(43, 35, 55 + i), 55 + i) for i in range(3)], False),
    ("lab32_keys1555", 1, 32, lambda: [synth.gradient_noise(50, 38, 60 + i) for i in range(4)], False),
    ("few_union_fits", 1, 64, lambda: [_few(23, 19, _colour_set(40, 70)[5 * i:5 * i + 12], 71 + i) for i in range(5)], True),
    ("few_union_exceeds", 1, 16, lambda: [_few(29, 17, _colour_set(48, 80)[12 * i:12 * i + 12], 81 + i) for i in range(4)], False),
]


@pytest.mark.parametrize("name,kind,K,mk,distinct", PAL_CASES, ids=[c[0] for c in PAL_CASES])
def test_palette_and_params_vs_oracle_on_concatenation(nq, oracle, name, kind, K, mk, distinct):
    frames = mk()
    oq, want = _oracle_sequence(oracle, kind, frames, K)
    d = _DevFrames(frames)
    q = _cls(nq, kind)(frames[0])
    got = nq.pnnquan_frames_device(q, d.ptrs(d.buf), d.widths, d.heights, K)
    assert len(got) == len(want) and (got == want).all()
    _assert_params(q.params, oq.params, distinct=distinct)
    if name == "few_union_fits":
        assert q.params.distinctColors <= K
    if name == "few_union_exceeds":
        assert len(np.unique(np.concatenate([f.reshape(-1) for f in frames]))) > K and all(len(np.unique(f)) <= K for f in frames)


def test_palette_of_1080p_panning_frames_equals_concatenated_copy(nq, oracle):
    """16 x 1920x1080 frames panning across one larger image (8 px per frame): the frames call == nq_pnnquan_device on a concatenated
    device copy (GPU vs GPU, exact), and the palette and scalars equal the oracle's."""
    import torch
    W, H, n = 1920, 1080, 16
    big = synth.gradient_noise_torch(W + 8 * (n - 1), H, 97).reshape(H, -1)
    frames_t = [big[:, 8 * t:8 * t + W].contiguous() for t in range(n)]
    concat = torch.cat([f.reshape(-1) for f in frames_t])
    q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
    got = nq.pnnquan_frames_device(q, [f.data_ptr() for f in frames_t], [W] * n, [H] * n, 256)
    got_params = q.params
    qc = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), width=1, height=1)
    qc.width, qc.height = 1, W * H * n
    want = qc.pnnquan_device(concat.data_ptr(), 256)
    assert len(got) == len(want) and (got == want).all()
    _assert_params(got_params, qc.params)
    oq = oracle.OracleQuantizer(1, concat.cpu().numpy().reshape(-1, 1))
    oq.prescan(256)
    pal = oq.pnnquan(256)
    assert (got == pal).all()
    _assert_params(got_params, oq.params)


# ---------------------------------------------------------------------------------------------------------------------------------
# every frame vs the oracle's dither of that frame with the shared palette and params
# ---------------------------------------------------------------------------------------------------------------------------------
def _mixed_frames(seed):
    return [synth.gradient_noise(64, 48, seed), synth.uniform_rgb(50, 37, seed + 1), synth.gradient_noise(33, 17, seed + 2),
            synth.gradient_noise(3, 2, seed + 3)]


DITHER_CASES = [  # name, kind, K, dither, mode, frames
    ("lab256_dither", 1, 256, True, TILED, lambda: _mixed_frames(200)),
    ("lab256_bluenoise", 1, 256, False, TILED, lambda: _mixed_frames(210)),
    ("lab64_semi_bluenoise", 1, 64, False, TILED, lambda: [synth.with_alpha(synth.gradient_noise(48, 40, 220 + i), 220 + i) for i in range(3)]),
    ("rgb64_dither", 0, 64, True, TILED, lambda: _mixed_frames(230)),
    ("lab256_lookup", 1, 256, False, LOOKUP, lambda: _mixed_frames(240)),
    ("lab64_sequential", 1, 64, True, SEQ, lambda: [synth.gradient_noise(32, 24, 250), synth.uniform_rgb(21, 19, 251)]),
    ("rgb16_sequential", 0, 16, True, SEQ, lambda: [synth.uniform_rgb(24, 20, 260), synth.gradient_noise(17, 23, 261)]),
]


def _oracle_frame(oracle, nq, kind, frame, K, shared, seed, pal, dither, mode, tile=None, rows=None):
    oq = oracle.OracleQuantizer(kind, frame, seed=seed)
    oq.prescan(K)
    oq.set_params(shared)
    oq.set_seed(seed)
    h, w = frame.shape
    if mode == LOOKUP:
        idx = oq.nearest_index(pal, frame.reshape(-1)).reshape(frame.shape).astype(np.int32)
        return pal[idx], idx
    if mode == SEQ:
        return oq.dither(pal, dither)
    tile = tile or _auto_tile(w, h)
    if rows is not None:
        return oq.dither_tile_rows(pal, dither, tile, rows[0], rows[1])
    return oq.dither(pal, dither, tile=tile)


@pytest.mark.parametrize("name,kind,K,dither,mode,mk", DITHER_CASES, ids=[c[0] for c in DITHER_CASES])
def test_frames_vs_oracle(nq, oracle, name, kind, K, dither, mode, mk):
    frames = mk()
    seeds = [1000 + 7 * i for i in range(len(frames))]
    oq, want_pal = _oracle_sequence(oracle, kind, frames, K)
    shared = oq.params
    d = _DevFrames(frames)
    q = _cls(nq, kind)(frames[0], mode=mode)
    pal = nq.convert_frames_device(q, d.ptrs(d.buf), d.widths, d.heights, K, dither, d.ptrs(d.out), d.ptrs(d.idx), seeds=seeds)
    assert (pal == want_pal).all()
    if kind == 1 and not dither and mode == TILED:
        # the BlueNoise weight counts the SEQUENCE's distinct colours (here more than any frame holds)
        assert q.params.distinctColors == shared.distinctColors
        if name == "lab256_bluenoise":
            assert all(len(np.unique(f)) < shared.distinctColors for f in frames)
    for i, f in enumerate(frames):
        want_argb, want_idx = _oracle_frame(oracle, nq, kind, f, K, shared, seeds[i], pal, dither, mode)
        got_argb, got_idx = d.result(i)
        assert (got_idx.astype(np.int32) == want_idx).all(), "frame %d index" % i
        assert (got_argb == want_argb).all(), "frame %d argb" % i
    assert d.guard_intact()


def test_fast_kernel_on_and_off_and_1080p_rows_vs_oracle(nq, oracle):
    """16 x 1080p panning frames, LAB 256 + dither, with the specialised dither kernel on and off: same results, and a few tile rows
    of every frame equal the oracle's tiled dither with the shared palette."""
    import torch
    W, H, n = 1920, 1080, 16
    big = synth.gradient_noise_torch(W + 8 * (n - 1), H, 98).reshape(H, -1)
    frames_t = [big[:, 8 * t:8 * t + W].contiguous() for t in range(n)]
    seeds = [500 + i for i in range(n)]
    results = []
    for fast in (1, 0):
        q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
        q.set_option(nq.host.OPT_FAST_DITHER, fast)
        outs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(n)]
        idxs = [torch.zeros(W * H, dtype=torch.int16, device="cuda") for _ in range(n)]
        pal = nq.convert_frames_device(q, [f.data_ptr() for f in frames_t], [W] * n, [H] * n, 256, True, [o.data_ptr() for o in outs],
                                       [i.data_ptr() for i in idxs], seeds=seeds)
        torch.cuda.synchronize()
        results.append((pal, outs, idxs, q.params))
    (pal, outs, idxs, params), (pal0, outs0, idxs0, _) = results
    assert (pal == pal0).all()
    for a, b in zip(outs + idxs, outs0 + idxs0):
        assert torch.equal(a, b)
    concat = torch.cat([f.reshape(-1) for f in frames_t]).cpu().numpy().reshape(-1, 1)
    oq = oracle.OracleQuantizer(1, concat)
    oq.prescan(256)
    want_pal = oq.pnnquan(256)
    assert (pal == want_pal).all()
    shared = oq.params
    tile = _auto_tile(W, H)
    for i in range(0, n, 5):
        frame = frames_t[i].cpu().numpy()
        got_argb = outs[i].cpu().numpy().reshape(H, W)
        got_idx = idxs[i].cpu().numpy().view(np.uint16).reshape(H, W)
        for r in (0, 131, H // tile[1] - 1):
            want_argb, want_idx = _oracle_frame(oracle, nq, 1, frame, 256, shared, seeds[i], pal, True, TILED, tile=tile, rows=(r, 1))
            y0, y1 = r * tile[1], (r + 1) * tile[1]
            assert (got_idx[y0:y1].astype(np.int32) == want_idx[y0:y1]).all(), (i, r)
            assert (got_argb[y0:y1] == want_argb[y0:y1]).all(), (i, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# host form, invalid input
# ---------------------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form_and_leaves_inputs(nq):
    frames = _mixed_frames(300)
    copies = [f.copy() for f in frames]
    seeds = [9, 8, 7, 6]
    pal_h, imgs = nq.convert_frames(1, frames, 256, True, seeds=seeds)
    assert all((a == b).all() for a, b in zip(frames, copies))
    d = _DevFrames(frames)
    q = nq.PnnLABQuantizer(frames[0])
    pal_d = nq.convert_frames_device(q, d.ptrs(d.buf), d.widths, d.heights, 256, True, d.ptrs(d.out), d.ptrs(d.idx), seeds=seeds)
    assert (pal_h == pal_d).all()
    for i, im in enumerate(imgs):
        argb, idx = d.result(i)
        assert (im.argb == argb).all() and (im.index == idx).all()


def test_invalid_input_and_the_handle_converts_afterwards(nq):
    img = synth.gradient_noise(40, 32, 400)
    q = nq.PnnLABQuantizer(img)
    L = q._L
    pal = np.zeros(256, np.int32)
    K = C.c_int32(0)
    seeds = np.zeros(4, np.int64)

    def call(n, ptrs, ws, hs):
        src = (C.c_void_p * max(n, 1))(*ptrs)
        dst = (C.c_void_p * max(n, 1))(*ptrs)
        w = np.asarray(ws, np.int32)
        h = np.asarray(hs, np.int32)
        a = L.nq_pnnquan_frames_device(q._h, n, src, w.ctypes.data, h.ctypes.data, 256, pal.ctypes.data, C.byref(K))
        b = L.nq_convert_frames_device(q._h, n, src, w.ctypes.data, h.ctypes.data, 256, 1, seeds.ctypes.data, TILED, dst, None,
                                       pal.ctypes.data, C.byref(K))
        return a, b

    fake = 1 << 40     # never dereferenced: the size check comes first
    assert call(2, [fake, fake], [65535, 65535], [32768, 32768]) == (-1, -1)      # 2^32 - ... > 2^31 - 1 pixels
    assert call(3, [fake, fake, fake], [46341, 46341, 1], [46341, 1, 1]) == (-1, -1)
    assert call(2, [fake, None], [8, 8], [8, 8]) == (-1, -1)
    assert call(0, [None], [8], [8]) == (-1, -1)
    assert call(-1, [None], [8], [8]) == (-1, -1)
    out = q.convert(256, True)
    ref = nq.PnnLABQuantizer(img).convert(256, True)
    assert (out.palette == ref.palette).all() and (out.argb == ref.argb).all()
