"""Delta-mode GIF encoding on the GPU (nq_encode_gif_delta / nq_encode_gif_delta_device): the bytes and the rectangles equal the
restatement in gif_delta_ref.py for every K, segment length, shape and kind of change tried; frames at odd 2-byte offsets in device
memory, never written; Pillow composes every file back to the frames; frames larger than one grid stride of the difference and body
kernels and more frame pairs than their grid has rows; a sprite animation through convert_frames_to_gif(delta=True)
stores only the tiles the sprite touched; every invalid input, each followed by a valid call on the same handle."""
import ctypes as C

import numpy as np
import pytest

import gif_delta_ref
import gif_ref
from nquant.android_amd import gif as G
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL")

from gif_delta_cases import (BIG_H, BIG_RECTS, BIG_W, GRID_Y, KS, MANY_FRAMES, ROWS, device_pool, many_rows, palette_of,  # noqa: E402
                             past_one_grid_stride, pillow_canvases, rgb_of, sequence)

SHAPES = ((1, 1), (1, 777), (37, 91), (256, 256))


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _decodes(gif, frames, pal, why):
    """Pillow and the restatement's own parser compose the file back to the frames."""
    got, own = pillow_canvases(gif), gif_delta_ref.compose(gif)
    assert len(got) == len(own) == len(frames), why
    for i, (g, c, f) in enumerate(zip(got, own, frames)):
        assert (c == f).all() and (g == rgb_of(f, pal)).all(), (why, i)


def _enc(hd, maps, pal, delays=None, loop=0, S=0):
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    h, w = maps[0].shape
    return G._encode_delta(hd._L, hd._h, "nq_encode_gif_delta", [a.ctypes.data for a in maps], w, h, pal, delays, loop, S, hd._check)


@pytest.mark.parametrize("K", KS)
def test_bytes_and_rectangles_equal_the_restatement(hd, K):
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng)
    for h, w in SHAPES:
        frames = sequence(h, w, K, rng)
        delays = [(7 * i) % 11 for i in range(len(frames))]
        for S in (1, 7, 4096, 0, h * w):
            got, rects = _enc(hd, frames, pal, delays, 0, S)
            want = gif_delta_ref.encode(frames, pal, delays_cs=delays, loop=0, segment_pixels=S)
            assert [tuple(r) for r in rects.tolist()] == gif_delta_ref.rectangles(frames), (K, h, w, S)
            assert got == want, (K, h, w, S, len(got), len(want))
            assert len(got) <= gif_ref.max_bytes([f.shape for f in frames], S)
            _decodes(got, frames, pal, (K, h, w, S))


def test_one_frame_and_two_frames(hd):
    rng = np.random.default_rng(5)
    K = 17
    pal = palette_of(K, rng)
    a = rng.integers(0, K, (37, 91))
    got, rects = _enc(hd, [a], pal, S=7)
    assert got == gif_ref.encode(a, pal, segment_pixels=7) and rects.tolist() == [[0, 0, 91, 37]]
    for loop in (0, 5, -1):
        got, rects = _enc(hd, [a, a], pal, [3, 65535], loop)
        assert got == gif_delta_ref.encode([a, a], pal, delays_cs=[3, 65535], loop=loop)
        assert rects.tolist() == [[0, 0, 91, 37], [0, 0, 1, 1]]
        _decodes(got, [a, a], pal, loop)
    b = a.copy()
    b[20:30, 40:80] = (b[20:30, 40:80] + 1) % K
    got, rects = _enc(hd, [a, b], pal, S=7)
    assert got == gif_delta_ref.encode([a, b], pal, segment_pixels=7) and rects.tolist() == [[0, 0, 91, 37], [40, 20, 40, 10]]
    _decodes(got, [a, b], pal, "two frames")


def test_noise_that_changes_everywhere_in_long_chains(hd):
    rng = np.random.default_rng(2)
    for K in (255, 256):
        frames = [rng.integers(0, K, (300, 500)) for _ in range(3)]
        pal = 0xFF000000 | np.arange(K)
        for S in (65536, 0):
            got, _ = _enc(hd, frames, pal, S=S)
            assert got == gif_delta_ref.encode(frames, pal, segment_pixels=S), (K, S)
            _decodes(got, frames, pal, (K, S))


def test_device_form_at_odd_offsets_leaves_the_frames_alone(nq, hd):
    import torch
    rng = np.random.default_rng(4)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    for (h, w), K in (((37, 91), 17), ((1, 777), 255), ((64, 63), 256), ((1, 1), 3)):
        frames = sequence(h, w, K, rng)
        pal = palette_of(K, rng)
        # one device buffer, every frame at an odd uint16 offset (2-byte but not 4-byte aligned) that differs modulo 16 bytes from
        # frame to frame, sentinels in between
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
        for S in (0, 7, 1000):
            got, rects = nq.encode_gif_delta_device(q, ptrs, w, h, pal, delays, 0, S, return_rects=True)
            assert got == gif_delta_ref.encode(frames, pal, delays_cs=delays, loop=0, segment_pixels=S), (h, w, K, S)
            assert [tuple(r) for r in rects.tolist()] == gif_delta_ref.rectangles(frames)
            _decodes(got, frames, pal, (h, w, K, S))
        assert nq.encode_gif_delta(frames, pal, delays) == gif_delta_ref.encode(frames, pal, delays_cs=delays)
        assert (buf.cpu().numpy().view(np.uint16) == host).all()
    q.close()


# ---- past the launch caps of the difference and body kernels ----
@pytest.mark.parametrize("S", [0, 65536])
@pytest.mark.parametrize("K", [17, 256])
def test_frames_and_bodies_past_one_grid_stride(nq, hd, K, S):
    """The cap: gridDim.x of gif_diff_kernel and gif_body_kernel is at most 1024 workgroups of 256 threads of 8 pixels, 2 097 152
    pixels; beyond it a thread takes the step c += gridDim.x * blockDim.x.  1449 x 1450 = 2 101 050 pixels, rows 1448 and 1449 wholly
    behind the cap (gif_delta_cases.past_one_grid_stride): a change found only there, a whole-frame body longer than one stride, a
    block in front of the cap and one behind it.  Host form and device form (every frame at an odd 2-byte offset)."""
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng)
    frames = past_one_grid_stride(K, rng)
    assert gif_delta_ref.rectangles(frames) == BIG_RECTS
    delays = [3, 0, 7, 1, 65535, 2]
    want = gif_delta_ref.encode(frames, pal, delays_cs=delays, loop=0, segment_pixels=S)
    got, rects = _enc(hd, frames, pal, delays, 0, S)
    assert [tuple(r) for r in rects.tolist()] == BIG_RECTS
    assert got == want, (K, S, len(got), len(want))
    buf, host, ptrs = device_pool(frames)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        got, rects = nq.encode_gif_delta_device(q, ptrs, BIG_W, BIG_H, pal, delays, 0, S, return_rects=True)
    finally:
        q.close()
    assert [tuple(r) for r in rects.tolist()] == BIG_RECTS
    assert got == want, (K, S, len(got), len(want))
    assert (buf.cpu().numpy().view(np.uint16) == host).all()
    canvases = pillow_canvases(got)
    assert len(canvases) == len(frames)
    for i, (g, f) in enumerate(zip(canvases, frames)):
        assert (g == rgb_of(f, pal)).all(), (K, S, i)


def test_more_frame_pairs_than_grid_rows(nq):
    """The cap: gridDim.y of the same two kernels is at most 65 535, one frame pair (one body) each; beyond it a workgroup takes the step
    f += gridDim.y.  65 540 frames of 3 x 1 are 65 539 pairs: blockIdx.y = 0 .. 3 take a second pair.  The pointer table names eight
    rows of one small device buffer in a seeded random order (most neighbours differ, some are equal)."""
    n, K = MANY_FRAMES, 4
    assert n - 1 > GRID_Y
    rng = np.random.default_rng(65)
    pal = palette_of(K, rng)
    pick = many_rows(n, rng)
    frames = [ROWS[i].reshape(1, 3) for i in pick]
    want_rects = gif_delta_ref.rectangles(frames)
    assert len(set(want_rects[GRID_Y + 1:])) > 1               # frames 65 536 .. 65 539: the second step has work, not all of it equal
    delays = (np.arange(n) % 7).tolist()
    want = gif_delta_ref.encode(frames, pal, delays_cs=delays, loop=0)
    buf, host, ptrs = device_pool(list(ROWS))
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        got, rects = nq.encode_gif_delta_device(q, [ptrs[i] for i in pick], 3, 1, pal, delays, 0, 0, return_rects=True)
    finally:
        q.close()
    assert [tuple(r) for r in rects.tolist()] == want_rects
    assert got == want, (len(got), len(want))
    own = gif_delta_ref.compose(got)
    assert len(own) == n and all((c == f).all() for c, f in zip(own, frames))
    assert (buf.cpu().numpy().view(np.uint16) == host).all()


# ---- the pipeline: a sprite over a static background ----
W, H, SPRITE = 128, 96, 16


def _sprite_at(i):
    return 9 + 23 * i, 13 + 17 * i


def _animation():
    back = synth.gradient_noise(W, H, 31)
    rng = np.random.default_rng(8)
    sprite = (0xFF000000 | rng.integers(0, 1 << 24, (SPRITE, SPRITE))).astype(np.int64).astype(np.uint32).view(np.int32)
    frames = []
    for i in range(4):
        f = back.copy()
        x, y = _sprite_at(i)
        f[y:y + SPRITE, x:x + SPRITE] = sprite
        frames.append(f)
    return frames


@pytest.mark.parametrize("tile", [(4, 4), (8, 8)])
@pytest.mark.parametrize("K", [255, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_sprite_animation_stores_only_the_tiles_it_touched(nq, kind, K, tile, tmp_path):
    frames = _animation()
    seeds = [5] * len(frames)
    delays = [4] * len(frames)
    pal, outs = nq.convert_frames(kind, frames, K, True, seeds=seeds, tile=tile)
    data, pal2 = nq.convert_frames_to_gif(kind, frames, K, True, delays_cs=delays, seeds=seeds, tile=tile, delta=True)
    full, _ = nq.convert_frames_to_gif(kind, frames, K, True, delays_cs=delays, seeds=seeds, tile=tile)
    assert (np.asarray(pal2) == np.asarray(pal)).all()
    maps = [o.index for o in outs]
    assert data == gif_delta_ref.encode(maps, pal, delays_cs=delays)
    _, _, parsed = gif_delta_ref.parse(data)
    tw, th = tile
    for i in range(1, len(frames)):
        inside = np.zeros((H, W), bool)                      # the sprite's old and new place, each expanded to tile boundaries
        for x, y in (_sprite_at(i - 1), _sprite_at(i)):
            inside[y // th * th:-(-(y + SPRITE) // th) * th, x // tw * tw:-(-(x + SPRITE) // tw) * tw] = True
        assert not ((maps[i] != maps[i - 1]) & ~inside).any(), (kind, K, tile, i)
        ys, xs = np.nonzero(inside)
        p = parsed[i]
        assert xs.min() <= p["x"] and p["x"] + p["w"] <= xs.max() + 1 and ys.min() <= p["y"] and p["y"] + p["h"] <= ys.max() + 1, (i, p["x"], p["y"])
    print("delta / full bytes: %d / %d = %.3f (kind %d, K %d, tile %s)" % (len(data), len(full), len(data) / len(full), kind, K, tile))
    assert len(data) < 0.5 * len(full), (len(data), len(full))
    for i, (g, c, o) in enumerate(zip(pillow_canvases(data), gif_delta_ref.compose(data), outs)):
        assert (c == o.index).all(), i
        argb = np.asarray(o.argb).view(np.uint32)
        assert (g == np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255], -1)).all(), i
    path = tmp_path / "a.gif"
    assert nq.write_gif(str(path), maps, pal, delays, delta=True) == len(data) and path.read_bytes() == data


def test_invalid_inputs_then_a_valid_call(nq, hd):
    L = hd._L
    a = np.zeros((4, 6), np.uint16)
    a[1, 2] = 2
    b = a.copy()
    b[2, 3] = 1
    pal = np.array([0xFF000000, 0xFFFFFFFF, 0xFF808080], np.uint32)

    def call(n=2, w=6, h=4, K=3, pal=pal, delays=None, loop=0, S=0, maps=None, cap=1 << 16, out=None, entry="nq_encode_gif_delta", src=0):
        maps = [a, b] if maps is None else maps
        if src == 0:
            src = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in (maps * max(n, 1))[:max(n, 1)]])
        d = None if delays is None else np.array(delays, np.int32)
        buf = np.zeros(max(cap, 1), np.uint8) if out is None else out
        size = C.c_int64(-7)
        rects = np.full((max(n, 1), 4), -9, np.int32)
        rc = getattr(L, entry)(hd._h, n, src, w, h, pal.ctypes.data, K, None if d is None else d.ctypes.data, loop, S, buf.ctypes.data, cap,
                               C.byref(size), rects.ctypes.data)
        return rc, size.value, buf, rects

    def valid():
        rc, size, buf, rects = call()
        assert rc == 0 and bytes(buf[:size]) == want and rects.tolist() == [[0, 0, 6, 4], [3, 2, 1, 1]]

    want = gif_delta_ref.encode([a, b], pal)
    valid()
    clear = pal.copy()
    clear[1] &= 0x00FFFFFF
    for kw in ({"pal": clear}, {"K": 0}, {"K": 257}, {"n": 0}, {"n": -3}, {"w": 0}, {"h": 65536}, {"S": -1}, {"loop": -2}, {"loop": 65536},
               {"delays": [0, -1]}, {"delays": [65536, 0]}, {"src": None}):
        rc, size, _, rects = call(**kw)
        assert rc == -1, kw
        assert size == -7 and (rects == -9).all(), kw        # rejected before any work
        if "pal" in kw:
            assert "nq_encode_gif" in (L.nq_last_error(hd._h) or b"").decode()
        valid()
    # one frame: an alpha-0 entry is still accepted, and the file is nq_encode_gif's
    rc, size, buf, rects = call(n=1, pal=clear)
    assert rc == 0 and bytes(buf[:size]) == gif_ref.encode(a, clear) and rects.tolist() == [[0, 0, 6, 4]]
    valid()
    # an index >= K, in the first frame, in a later one, inside and outside the changed rectangle
    for which, at in ((0, (3, 5)), (1, (3, 5)), (1, (0, 0)), (0, (2, 3))):
        maps = [a.copy(), b.copy()]
        maps[which][at] = 3
        assert call(maps=maps)[0] == -1, (which, at)
        assert "index" in (L.nq_last_error(hd._h) or b"").decode()
        valid()
    both = [a.copy(), b.copy()]
    both[0][0, 0] = both[1][0, 0] = 3                        # the same bad index in both frames: unchanged, still reported
    assert call(maps=both)[0] == -1
    valid()
    # cap smaller than the file: the size is reported, out is untouched
    small = np.full(len(want) - 1, 0xAB, np.uint8)
    rc, size, _, _ = call(cap=len(want) - 1, out=small)
    assert rc == -1 and size == len(want) and (small == 0xAB).all()
    rc, size, buf, _ = call(cap=len(want))
    assert rc == 0 and bytes(buf[:size]) == want
    # odd index pointers
    raw = np.zeros(a.size + 1, np.uint16)
    odd = np.frombuffer(raw.data, np.uint8)[1:1 + 2 * a.size]
    assert odd.ctypes.data % 2 == 1
    assert call(maps=[a, odd])[0] == -1
    valid()
    # a NULL frame pointer
    src = (C.c_void_p * 2)(a.ctypes.data, None)
    assert call(src=src)[0] == -1
    valid()
    # and the full-frame entry point is what it was
    w2, h2 = np.full(2, 6, np.int32), np.full(2, 4, np.int32)
    assert G._encode(L, hd._h, "nq_encode_gif", [a.ctypes.data, b.ctypes.data], w2, h2, pal, None, 0, 0, hd._check) == gif_ref.encode([a, b], pal)
