"""GIF files with one colour table per frame on the GPU (nq_encode_gif_local* / nq_encode_gif_local_delta*): bytes and rectangles equal
the restatement in gif_local_ref.py for every K of the definition within one file, every shape, segment length and both thresholds; the
named edge cases of "changed by colour"; frames at odd 2-byte offsets in device memory, never written; long chains with K alternating
255 / 256; frames larger than one grid stride of the two delta passes and more frame pairs than their grid has rows (the LDS tables
refilled inside a live workgroup); the lossy bound on Pillow's canvases; every invalid input followed by a valid call; one palette per shot through
convert_shots_to_gif."""
import ctypes as C

import numpy as np
import pytest

import gif_local_cases as cases
import gif_local_ref as R
from gif_delta_cases import (BIG_H, BIG_RECTS, BIG_W, GRID_Y, MANY_FRAMES, ROWS, device_pool, many_rows, palette_of, past_one_grid_stride,
                             pillow_canvases)
from nquant.android_amd import gif as G
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 777), (37, 91), (128, 128))


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _enc(hd, maps, pals, delays=None, loop=0, S=0, lossy=0, delta=False):
    """(file, rectangles or None) through the host form on the module's handle."""
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    ptrs = [a.ctypes.data for a in maps]
    if delta:
        h, w = maps[0].shape
        return G._encode_local(hd._L, hd._h, "nq_encode_gif_local_delta", ptrs, w, h, pals, delays, loop, S, lossy, hd._check, True)
    w = np.array([a.shape[1] for a in maps], np.int32)
    h = np.array([a.shape[0] for a in maps], np.int32)
    return G._encode_local(hd._L, hd._h, "nq_encode_gif_local", ptrs, w, h, pals, delays, loop, S, lossy, hd._check, False)


def _rects(rects):
    return [tuple(r) for r in rects.tolist()]


def _within(canvases, want, lossy, why):
    assert len(canvases) == len(want), why
    for i, (c, f) in enumerate(zip(canvases, want)):
        assert c.shape == f.shape and np.abs(c.astype(int) - f.astype(int)).max() <= lossy, (why, i)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("delta", [False, True])
def test_bytes_and_rectangles_equal_the_restatement(hd, shape, delta):
    """All ten K in one file: with S = 7 the four chains of a workgroup sit in frames with different m and tables."""
    h, w = shape
    rng = np.random.default_rng(1000 * delta + 7 * h + w)
    ks = cases.MIXED_KS if h * w < 10000 else cases.SHORT_KS
    frames, pals = cases.mixed(h, w, rng, ks, near=True)
    delays = [(7 * i) % 11 for i in range(len(frames))]
    want_rgb = cases.shown(frames, pals)
    substituted = 0
    for S in (1, 7, 4096, 0, h * w):
        for lossy in (0, 16):
            want, subs = (R.encode_delta if delta else R.encode)(frames, pals, delays, 0, S, lossy)
            got, rects = _enc(hd, frames, pals, delays, 0, S, lossy, delta)
            assert got == want, (shape, delta, S, lossy, len(got), len(want), subs)
            if delta:
                assert _rects(rects) == R.rectangles(frames, pals), (shape, S, lossy)
            assert len(got) <= R.max_bytes([f.shape for f in frames], S)
            substituted += subs
        _within(R.compose(got), want_rgb, 16, (shape, delta, S))
    assert substituted > 0 or h * w == 1, shape


def test_named_edge_cases(hd):
    rng = np.random.default_rng(21)
    for name, (frames, pals, rects) in cases.edge_cases(rng).items():
        for S in (0, 7):
            for lossy in (0, 16):
                got, r = _enc(hd, frames, pals, [2, 3], -1, S, lossy, True)
                assert got == R.encode_delta(frames, pals, [2, 3], -1, S, lossy)[0], (name, S, lossy)
                assert _rects(r) == R.rectangles(frames, pals) and (rects is None or _rects(r) == rects), name
            assert R.encode(frames, pals, [2, 3], -1, S)[0] == _enc(hd, frames, pals, [2, 3], -1, S)[0], name
        _within(pillow_canvases(got), cases.shown(frames, pals), 16, name)
    # one frame: the local form, through both calls
    f, p = frames[:1], pals[:1]
    got, r = _enc(hd, f, p, S=7, delta=True)
    assert got == R.encode(f, p, segment_pixels=7)[0] == _enc(hd, f, p, S=7)[0] and _rects(r) == [(0, 0, 31, 19)]
    # full frames keep real transparency, per frame: t differs from frame to frame
    pa, pb = palette_of(9, rng), palette_of(5, rng)
    pa[3] &= 0x00FFFFFF
    pb[0] &= 0x00FFFFFF
    maps = [rng.integers(0, 9, (19, 31)), rng.integers(0, 5, (7, 40)), rng.integers(0, 17, (3, 3))]
    for lossy in (0, 255):
        got, _ = _enc(hd, maps, [pa, pb, pals[0]], [1, 2, 3], 4, 7, lossy)
        assert got == R.encode(maps, [pa, pb, pals[0]], [1, 2, 3], 4, 7, lossy)[0], lossy
        parsed = R.parse(got)[1]
        assert [x.get("transparency") for x in parsed] == [3, 0, None]
        assert ((parsed[0]["index"] == 3) == (maps[0] == 3)).all() and ((parsed[1]["index"] == 0) == (maps[1] == 0)).all()


def test_device_form_at_odd_offsets_leaves_the_frames_alone(nq, hd):
    import torch
    rng = np.random.default_rng(4)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    for h, w in ((37, 91), (64, 63)):
        frames, pals = cases.mixed(h, w, rng, cases.SHORT_KS, near=True)
        offs, off = [], 1
        for i, f in enumerate(frames):
            offs.append(off)
            off += f.size + 2 * (i % 5) + 1
            off += 1 - off % 2
        host = np.full(off + 8, 0xFFFF, np.uint16)
        for f, o in zip(frames, offs):
            host[o:o + f.size] = f.reshape(-1)
        buf = torch.from_numpy(host.view(np.int16)).cuda()
        ptrs = [buf.data_ptr() + 2 * o for o in offs]
        assert all(p % 4 == 2 for p in ptrs) and len({p % 16 for p in ptrs}) > 1
        delays = list(range(len(frames)))
        for S, lossy in ((0, 0), (7, 16), (1000, 0), (0, 16)):
            got, rects = nq.encode_gif_local_delta_device(q, ptrs, w, h, pals, delays, 0, S, return_rects=True, lossy=lossy)
            assert got == R.encode_delta(frames, pals, delays, 0, S, lossy)[0], (h, w, S, lossy)
            assert _rects(rects) == R.rectangles(frames, pals)
            got = nq.encode_gif_local_device(q, ptrs, [w] * len(frames), [h] * len(frames), pals, delays, 0, S, lossy=lossy)
            assert got == R.encode(frames, pals, delays, 0, S, lossy)[0], (h, w, S, lossy)
        assert nq.encode_gif_local_delta(frames, pals, delays) == R.encode_delta(frames, pals, delays)[0]
        assert nq.encode_gif_local(frames, pals, delays) == R.encode(frames, pals, delays)[0]
        assert (buf.cpu().numpy().view(np.uint16) == host).all()
    q.close()


def test_noise_in_long_chains_with_K_alternating_255_and_256(hd):
    rng = np.random.default_rng(2)
    ks = (255, 256, 255, 256)
    frames = [rng.integers(0, K, (300, 500)) for K in ks]
    pals = [0xFF000000 | np.arange(K) * 0x010203 for K in ks]
    want_rgb = cases.shown(frames, pals)
    for delta in (False, True):
        got, rects = _enc(hd, frames, pals, S=65536, delta=delta)
        assert got == (R.encode_delta if delta else R.encode)(frames, pals, None, 0, 65536)[0], delta
        _within(pillow_canvases(got), want_rgb, 0, delta)
        assert len(got) <= R.max_bytes([f.shape for f in frames], 65536)


# ---- past the launch caps of the difference and body kernels ----
@pytest.mark.parametrize("S", [0, 65536])
@pytest.mark.parametrize("K", [17, 256])
def test_frames_and_bodies_past_one_grid_stride(nq, hd, K, S):
    """The cap: gridDim.x of gif_diff_local_kernel and gif_body_local_kernel is at most 1024 workgroups of 256 threads of 8 pixels,
    2 097 152 pixels; beyond it a thread takes the step c += gridDim.x * blockDim.x.  The 1449 x 1450 sequence of
    test_gpu_gif_delta.py (2 101 050 pixels; gif_delta_cases.past_one_grid_stride), here with frames 4 and 5 under a table that is a
    permutation of the one before, their indices permuted to match: every index of frame 4 in front of the cap differs from frame 3's,
    and the rectangle is still the block behind the cap, because "differs" is judged on the colour.  Host form and device form (odd 2-byte offsets)."""
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng)
    assert len(set((pal & 0xFFFFFF).tolist())) == K
    frames = past_one_grid_stride(K, rng)
    perm = np.roll(np.arange(K), 1).astype(np.uint16)   # entry perm[j] of the new table is entry j of the old: no fixed point
    pal2 = np.empty_like(pal)
    pal2[perm] = pal
    frames[4], frames[5] = perm[frames[4]], perm[frames[5]]
    assert (frames[4][:BIG_H - 2] != frames[3][:BIG_H - 2]).all()
    pals = [pal] * 4 + [pal2] * 2
    assert R.rectangles(frames, pals) == BIG_RECTS
    delays = [3, 0, 7, 1, 65535, 2]
    want = R.encode_delta(frames, pals, delays, 0, S)[0]
    got, rects = _enc(hd, frames, pals, delays, 0, S, 0, True)
    assert _rects(rects) == BIG_RECTS
    assert got == want, (K, S, len(got), len(want))
    buf, host, ptrs = device_pool(frames)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        got, rects = nq.encode_gif_local_delta_device(q, ptrs, BIG_W, BIG_H, pals, delays, 0, S, return_rects=True)
    finally:
        q.close()
    assert _rects(rects) == BIG_RECTS
    assert got == want, (K, S, len(got), len(want))
    assert (buf.cpu().numpy().view(np.uint16) == host).all()
    _within(pillow_canvases(got), cases.shown(frames, pals), 0, (K, S))


def test_more_frame_pairs_than_grid_rows(nq):
    """The cap: gridDim.y of the same two kernels is at most 65 535, one frame pair (one body) each; beyond it a workgroup takes the step
    f += gridDim.y and load_tables refills both LDS colour tables between its barriers while the workgroup is still alive.  65 540
    frames of 3 x 1 are 65 539 pairs: blockIdx.y = 0 .. 3 take a second pair.  The table length alternates between 3 and 4, the table
    contents come from a pool of four that share some colours and never repeat from one frame to the next, so both LDS tables change
    at every step; the pointer table names eight rows of one small device buffer in a seeded random order."""
    n = MANY_FRAMES
    assert n - 1 > GRID_Y
    rng = np.random.default_rng(66)
    pool = [palette_of(4, rng) for _ in range(4)]
    pool[1][0], pool[2][1], pool[3][2] = pool[0][0], pool[0][1], pool[1][1]     # a colour two tables share, at the same index or another
    pool[3][0] = pool[2][2]
    which = np.cumsum(rng.integers(1, 4, n)) % 4               # steps of 1 .. 3 modulo 4: no table twice in a row
    assert (which[1:] != which[:-1]).all()
    pals = [pool[c][:3 + i % 2] for i, c in enumerate(which)]
    pick = many_rows(n, rng, lambda i: 3 + i % 2)
    frames = [ROWS[i].reshape(1, 3) for i in pick]
    assert all(int(f.max()) < len(p) for f, p in zip(frames[:64], pals[:64]))
    delays = (np.arange(n) % 7).tolist()
    want = R.encode_delta(frames, pals, delays, 0, 0)[0]
    buf, host, ptrs = device_pool(list(ROWS))
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        got, rects = nq.encode_gif_local_delta_device(q, [ptrs[i] for i in pick], 3, 1, pals, delays, 0, 0, return_rects=True)
    finally:
        q.close()
    assert got == want, (len(got), len(want))
    # the file is the restatement's, so the rectangles in it are R.rectangles(frames, pals): one parse gives them and the canvases
    screen, parsed = R.parse(got)
    want_rects = [(p["x"], p["y"], p["w"], p["h"]) for p in parsed]
    assert want_rects[:64] == R.rectangles(frames[:64], pals[:64]) and want_rects[GRID_Y - 2:] == R.rectangles(frames[GRID_Y - 3:], pals[GRID_Y - 3:])[1:]
    assert _rects(rects) == want_rects
    assert any(r != (0, 0, 1, 1) for r in want_rects[GRID_Y + 1:])      # frames 65 536 .. 65 539: the second step has work
    own = np.array(R.compose_parsed(screen, parsed))
    colours = np.array(pool)[which[:, None], ROWS[pick]]       # (n, 3): what every frame shows (cases.shown, for all frames at once)
    shown = np.stack([(colours >> 16) & 255, (colours >> 8) & 255, colours & 255], -1).reshape(n, 1, 3, 3)
    assert own.shape == shown.shape and (own == shown).all()
    assert (shown[:64] == np.array(cases.shown(frames[:64], pals[:64]))).all()
    assert (buf.cpu().numpy().view(np.uint16) == host).all()


@pytest.mark.parametrize("delta", [False, True])
def test_lossy_bound_on_pillows_canvases(hd, delta):
    rng = np.random.default_rng(6)
    frames, pals = cases.mixed(37, 91, rng, near=True)
    lossless, _ = _enc(hd, frames, pals, delta=delta)
    _within(pillow_canvases(lossless), cases.shown(frames, pals), 0, delta)
    for lossy in (16, 40):
        got, _ = _enc(hd, frames, pals, lossy=lossy, delta=delta)
        want, subs = (R.encode_delta if delta else R.encode)(frames, pals, None, 0, 0, lossy)
        assert got == want and subs > 0 and len(got) <= len(lossless)
        _within(pillow_canvases(got), cases.shown(frames, pals), lossy, (delta, lossy))


def test_invalid_inputs_then_a_valid_call(hd):
    L = hd._L
    a = np.zeros((4, 6), np.uint16)
    a[1, 2] = 2
    b = a.copy()
    b[2, 3] = 1
    pals = np.array([[0xFF000000, 0xFFFFFFFF, 0xFF808080, 0], [0xFF000000, 0xFFFFFFFF, 0xFF808080, 0xFF112233]], np.uint32)
    plist = [pals[0, :3], pals[1]]
    Ks = [3, 4]

    def call(entry, n=2, w=6, h=4, pals=pals, stride=4, K=Ks, delays=None, loop=0, S=0, lossy=0, maps=None, cap=1 << 16, out=None, src=0,
             size_ptr=True):
        delta = "delta" in entry
        maps = [a, b] if maps is None else maps
        if src == 0:
            src = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in (maps * max(n, 1))[:max(n, 1)]])
        d = None if delays is None else np.array(delays, np.int32)
        k = None if K is None else np.array(K, np.int32)
        buf = np.zeros(max(cap, 1), np.uint8) if out is None else out
        size = C.c_int64(-7)
        rects = np.full((max(n, 1), 4), -9, np.int32)
        ws, hs = np.full(max(n, 1), w, np.int32), np.full(max(n, 1), h, np.int32)
        sizes = (w, h) if delta else (ws.ctypes.data, hs.ctypes.data)
        rc = getattr(L, entry)(hd._h, n, src, *sizes, None if pals is None else pals.ctypes.data, stride, None if k is None else k.ctypes.data,
                               None if d is None else d.ctypes.data, loop, S, lossy, buf.ctypes.data, cap, C.byref(size) if size_ptr else None,
                               *((rects.ctypes.data,) if delta else ()))
        return rc, size.value, buf, rects

    clear = pals.copy()
    clear[1, 1] &= 0x00FFFFFF
    for entry, ref in (("nq_encode_gif_local", R.encode), ("nq_encode_gif_local_delta", R.encode_delta)):
        delta = "delta" in entry
        want = ref([a, b], plist)[0]

        def valid():
            rc, size, buf, rects = call(entry)
            assert rc == 0 and bytes(buf[:size]) == want, entry
            if delta:
                assert rects.tolist() == [[0, 0, 6, 4], [3, 2, 1, 1]]

        valid()
        bad = [{"K": [0, 3]}, {"K": [3, 257]}, {"K": None}, {"pals": None}, {"stride": 3}, {"lossy": -1}, {"lossy": 256}, {"n": 0}, {"n": -3},
               {"w": 0}, {"h": 65536}, {"S": -1}, {"loop": -2}, {"loop": 65536}, {"delays": [0, -1]}, {"delays": [65536, 0]}, {"src": None},
               {"cap": -1}]
        if delta:
            bad.append({"pals": clear})
        for kw in bad:
            rc, size, buf, rects = call(entry, **kw)
            assert rc == -1, (entry, kw)
            assert size == -7 and (rects == -9).all() and not buf.any(), (entry, kw)     # rejected before any work
            valid()
        assert call(entry, size_ptr=False)[0] == -1
        valid()
        if not delta:                                # full frames take the transparent entry
            rc, size, buf, _ = call(entry, pals=clear)
            assert rc == 0 and bytes(buf[:size]) == R.encode([a, b], [clear[0, :3], clear[1]])[0]
        else:                                        # and so does one delta frame
            rc, size, buf, rects = call(entry, n=1, pals=clear[1:], K=[4])
            assert rc == 0 and bytes(buf[:size]) == R.encode([a], [clear[1]])[0] and rects.tolist() == [[0, 0, 6, 4]]
        # an index >= its own frame's K: 3 is valid in frame 1 (K = 4) and not in frame 0 (K = 3)
        ok = [a.copy(), b.copy()]
        ok[1][3, 5] = 3
        rc, size, buf, _ = call(entry, maps=ok)
        assert rc == 0 and bytes(buf[:size]) == ref(ok, plist)[0], entry
        for which, at, v in ((0, (3, 5), 3), (1, (3, 5), 4), (1, (0, 0), 300), (0, (2, 3), 256 + 1)):
            maps = [a.copy(), b.copy()]
            maps[which][at] = v
            for lossy in (0, 16):
                assert call(entry, maps=maps, lossy=lossy)[0] == -1, (entry, which, at)
                msg = (L.nq_last_error(hd._h) or b"").decode()
                assert "index" in msg and ("frame %d" % which) in msg, msg
            valid()
        # cap smaller than the file: the size is reported, out is untouched
        small = np.full(len(want) - 1, 0xAB, np.uint8)
        rc, size, _, _ = call(entry, cap=len(want) - 1, out=small)
        assert rc == -1 and size == len(want) and (small == 0xAB).all()
        # an odd and a NULL frame pointer
        raw = np.zeros(a.size + 1, np.uint16)
        odd = np.frombuffer(raw.data, np.uint8)[1:1 + 2 * a.size]
        assert call(entry, maps=[a, odd])[0] == -1
        assert call(entry, src=(C.c_void_p * 2)(a.ctypes.data, None))[0] == -1
        valid()


# ---- the pipeline: two shots, a sprite over each shot's own background ----
W, H, SPRITE = 128, 96, 16


def _sprite_at(i):
    return 9 + 23 * (i % 4), 13 + 17 * (i % 4)


def _two_shots():
    rng = np.random.default_rng(8)
    sprite = (0xFF000000 | rng.integers(0, 1 << 24, (SPRITE, SPRITE))).astype(np.int64).astype(np.uint32).view(np.int32)
    frames = []
    for i in range(8):
        f = synth.gradient_noise(W, H, 31 + 40 * (i // 4)).copy()
        x, y = _sprite_at(i)
        f[y:y + SPRITE, x:x + SPRITE] = sprite
        frames.append(f)
    return frames


def _rgb(argb):
    argb = np.asarray(argb).view(np.uint32)
    return np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255], -1).astype(np.uint8)


@pytest.mark.parametrize("tile", [(4, 4), (8, 8)])
def test_one_palette_per_shot(nq, tile):
    kind, K = 1, 64
    frames = _two_shots()
    seeds, delays = [5] * 8, [4] * 8
    data, pals = nq.convert_shots_to_gif(kind, frames, [0, 4], K, True, delays_cs=delays, seeds=seeds, tile=tile)
    maps, per_frame, outs = [], [], []
    for k, (a, b) in enumerate(((0, 4), (4, 8))):
        pal, o = nq.convert_frames(kind, frames[a:b], K, True, seeds=seeds[a:b], tile=tile)
        assert (np.asarray(pal) == np.asarray(pals[k])).all()
        maps += [x.index for x in o]
        outs += o
        per_frame += [pal] * (b - a)
    assert len(pals) == 2 and not np.array_equal(pals[0], pals[1])
    assert data == R.encode_delta(maps, per_frame, delays)[0]
    rects = R.rectangles(maps, per_frame)
    parsed = R.parse(data)[1]
    assert [(p["x"], p["y"], p["w"], p["h"]) for p in parsed] == rects
    tw, th = tile
    for i in (1, 2, 3, 5, 6, 7):
        inside = np.zeros((H, W), bool)                      # the sprite's old and new place, each expanded to tile boundaries
        for x, y in (_sprite_at(i - 1), _sprite_at(i)):
            inside[y // th * th:-(-(y + SPRITE) // th) * th, x // tw * tw:-(-(x + SPRITE) // tw) * tw] = True
        ys, xs = np.nonzero(inside)
        x, y, w, h = rects[i]
        assert xs.min() <= x and x + w <= xs.max() + 1 and ys.min() <= y and y + h <= ys.max() + 1, (i, rects[i])
    ys, xs = np.nonzero(R.changed(maps, per_frame, 4))       # the cut: the changed region by colour
    assert rects[4] == (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) and rects[4][2] * rects[4][3] > W * H // 2
    for i, (g, c, o) in enumerate(zip(pillow_canvases(data), R.compose(data), outs)):
        assert (c == _rgb(o.argb)).all() and (g == _rgb(o.argb)).all(), i
    # against one shared palette at the same K (printed, not asserted)
    shared, _ = nq.convert_frames_to_gif(kind, frames, K, True, delays_cs=delays, seeds=seeds, tile=tile, delta=True)
    src = [_rgb(f).astype(np.int64) for f in frames]
    sse = lambda gif: sum(int(((c.astype(np.int64) - s) ** 2).sum()) for c, s in zip(pillow_canvases(gif), src))
    print("tile %s: per-shot palettes %d bytes, squared RGB error %d; one shared palette %d bytes, squared RGB error %d"
          % (tile, len(data), sse(data), len(shared), sse(shared)))
    # full frames, a hold per shot and a threshold go through the same handle
    full, _ = nq.convert_shots_to_gif(kind, frames, [0, 4], K, True, delays_cs=delays, seeds=seeds, tile=tile, delta=False)
    assert full == R.encode(maps, per_frame, delays)[0]
    held = []
    for a, b in ((0, 4), (4, 8)):
        held += nq.hold_frames(frames[a:b], maps[a:b], 4)[0]
    lossy, _ = nq.convert_shots_to_gif(kind, frames, [0, 4], K, True, delays_cs=delays, seeds=seeds, tile=tile, hold=4, lossy=16)
    assert lossy == R.encode_delta(held, per_frame, delays, 0, 0, 16)[0]
