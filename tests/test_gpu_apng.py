"""APNG encoding on the GPU (nq_encode_apng / nq_encode_apng_device): the bytes and the rectangles equal the restatement in apng_ref.py
for every K, segment length, shape, palette kind and kind of change tried; every file composes back to the RGBA frames through
apng_ref.compose and through Pillow; a sprite over a transparent region un-paints its old place (crop mode); rectangles that start in
mid-word of the source at depths 1, 2 and 4; frames larger than one grid stride of the difference pass; frames at odd 2-byte offsets in device memory, never written; convert_frames_to_apng on
a sprite animation, also over a transparent background (which delta GIF refuses); every invalid input, each followed by a valid call
on the same handle.  The limit cases of png_cases.py as frame 1 of a two-frame file, whole (crop mode) and with unchanged pixels packed
as u (mark mode): png_deflate_kernel<true> at its limiters, its bit writer's third word and its window's edges."""
import ctypes as C

import numpy as np
import pytest

import apng_ref
import gif_delta_ref
import png_cases
import png_ref
from nquant.android_amd import apng as A
from nquant.android_amd import gif as G
from nquant.android_amd import png as P
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL")

from gif_delta_cases import BIG_H, BIG_RECTS, BIG_W, KS, device_pool, palette_of, past_one_grid_stride, sequence  # noqa: E402
from test_apng_cpu import alpha_palette, composes_back  # noqa: E402

SHAPES = ((1, 1), (1, 777), (37, 91), (256, 256))
SEGMENTS = (1, 7, 4096, 0, 65535)


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _enc(hd, maps, pal, delays=None, loop=0, S=0):
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    h, w = maps[0].shape
    return A._encode(hd._L, hd._h, "nq_encode_apng", [a.ctypes.data for a in maps], w, h, pal, delays, loop, S, hd._check)


def _rects(frames):
    return [list(r) for r in gif_delta_ref.rectangles(frames)]


@pytest.mark.parametrize("kind", ["opaque", "alpha"])
@pytest.mark.parametrize("K", KS)
def test_bytes_and_rectangles_equal_the_restatement(nq, hd, K, kind):
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng) if kind == "opaque" else alpha_palette(K, rng)
    for h, w in SHAPES:
        frames = sequence(h, w, K, rng)
        delays = [(7 * i) % 11 for i in range(len(frames))]
        for S in SEGMENTS:
            got, rects = _enc(hd, frames, pal, delays, 2, S)
            want = apng_ref.encode(frames, pal, delays_cs=delays, loop=2, segment_bytes=S)
            assert rects.tolist() == _rects(frames), (K, kind, h, w, S)
            assert got == want, (K, kind, h, w, S, len(got), len(want))
            assert _enc(hd, frames, pal, delays, 2, S)[0] == got          # two calls, identical bytes
            assert len(got) <= nq.apng_max_bytes(len(frames), w, h, S)
            composes_back(got, frames, pal, (K, kind, h, w, S))


def test_sprite_over_a_transparent_region_unpaints_its_old_place(hd):
    """Crop mode: index 0 is alpha 0.  The sprite moves; where it was, the frame holds index 0 again, and blend SOURCE makes the canvas
    transparent there (blend OVER would leave the sprite standing)."""
    rng = np.random.default_rng(3)
    K = 16
    pal = palette_of(K, rng)
    pal[0] = 0x00123456
    pal[5] = (pal[5] & 0x00FFFFFF) | 0x80000000
    frames = []
    for i in range(4):
        f = np.zeros((48, 64), np.int64)
        f[40:, :] = 7                                                       # an opaque floor that never changes
        f[5 + 9 * i:17 + 9 * i, 3 + 13 * i:15 + 13 * i] = rng.integers(1, K, (12, 12))
        frames.append(f)
    got, rects = _enc(hd, frames, pal, [5] * 4)
    assert got == apng_ref.encode(frames, pal, delays_cs=[5] * 4)
    assert rects.tolist() == _rects(frames) and rects.tolist()[1] == [3, 5, 25, 21]
    _, parsed = apng_ref.parse(got)
    assert [p["blend"] for p in parsed] == [0] * 4
    canvases = apng_ref.compose(got)
    assert (canvases[1][5:14, 3:15, 3] == 0).all()                           # the old place, transparent again
    composes_back(got, frames, pal, "sprite over alpha 0")


def test_noise_that_changes_everywhere_in_long_chains(hd):
    rng = np.random.default_rng(2)
    for K in (255, 256):
        frames = [rng.integers(0, K, (300, 500)) for _ in range(3)]
        pal = 0xFF000000 | np.arange(K)
        for S in (65535, 0):
            got, rects = _enc(hd, frames, pal, S=S)
            assert rects.tolist() == [[0, 0, 500, 300]] * 3
            assert got == apng_ref.encode(frames, pal, segment_bytes=S), (K, S)
            composes_back(got, frames, pal, (K, S))


def test_rectangles_past_one_grid_stride_of_the_difference_pass(nq):
    """The cap: APNG takes its rectangles from gif_diff_kernel, whose gridDim.x is at most 1024 workgroups of 256 threads of 8 pixels,
    2 097 152 pixels.  The 1449 x 1450 sequence of test_gpu_gif_delta.py (2 101 050 pixels; gif_delta_cases.past_one_grid_stride) in
    mark mode, device form at odd 2-byte offsets: the rectangles, and the canvases apng_ref composes from the file."""
    K = 17
    rng = np.random.default_rng(K)
    pal = palette_of(K, rng)
    frames = past_one_grid_stride(K, rng)
    buf, host, ptrs = device_pool(frames)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        got, rects = nq.encode_apng_device(q, ptrs, BIG_W, BIG_H, pal, None, 0, 0, return_rects=True)
    finally:
        q.close()
    assert rects.tolist() == [list(r) for r in BIG_RECTS] == _rects(frames)
    assert len(got) <= nq.apng_max_bytes(len(frames), BIG_W, BIG_H, 0)
    own = apng_ref.compose(got)
    assert len(own) == len(frames)
    for i, (c, f) in enumerate(zip(own, frames)):
        assert (c == apng_ref.rgba_of(f, pal)).all(), i
    assert (buf.cpu().numpy().view(np.uint16) == host).all()


@pytest.mark.parametrize("K", [2, 3, 15])
def test_rectangles_that_start_in_mid_word_of_the_source(hd, K):
    """Mark mode (u = K) at depths 2, 2 and 4, and crop mode at depths 1, 2 and 4: the rectangle's x offset and width are odd, so its
    rows start at odd elements of the maps and end inside a packed byte."""
    rng = np.random.default_rng(40 + K)
    for pal in (palette_of(K, rng), alpha_palette(K, rng)):
        for (h, w), (x, y, rw, rh) in (((20, 40), (5, 3, 13, 9)), ((9, 33), (1, 0, 31, 9)), ((6, 11), (7, 5, 3, 1)), ((64, 100), (33, 7, 51, 40))):
            a = rng.integers(0, K, (h, w))
            b = a.copy()
            b[y:y + rh, x:x + rw] = rng.integers(0, K, (rh, rw))
            b[y, x] = (a[y, x] + 1) % K                                      # the corners change for certain
            b[y + rh - 1, x + rw - 1] = (a[y + rh - 1, x + rw - 1] + 1) % K
            c = b.copy()
            c[y:y + rh, x] = (b[y:y + rh, x] + 1) % K                         # one odd column
            frames = [a, b, c]
            for S in (0, 5):
                got, rects = _enc(hd, frames, pal, S=S)
                assert rects.tolist() == [[0, 0, w, h], [x, y, rw, rh], [x, y, 1, rh]], (K, h, w)
                assert x % 2 == 1 and rw % 2 == 1
                assert got == apng_ref.encode(frames, pal, segment_bytes=S), (K, h, w, S)
                composes_back(got, frames, pal, (K, h, w, S))


def test_device_form_at_odd_offsets_leaves_the_frames_alone(nq, hd):
    import torch
    rng = np.random.default_rng(4)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    for (h, w), K, opaque in (((37, 91), 17, True), ((1, 777), 255, True), ((64, 63), 256, True), ((1, 1), 3, False), ((40, 31), 4, False)):
        frames = sequence(h, w, K, rng)
        pal = palette_of(K, rng) if opaque else alpha_palette(K, rng)
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
            got, rects = nq.encode_apng_device(q, ptrs, w, h, pal, delays, 0, S, return_rects=True)
            assert got == apng_ref.encode(frames, pal, delays_cs=delays, loop=0, segment_bytes=S), (h, w, K, S)
            assert rects.tolist() == _rects(frames)
            composes_back(got, frames, pal, (h, w, K, S))
        assert nq.encode_apng(frames, pal, delays) == apng_ref.encode(frames, pal, delays_cs=delays)     # host and device forms agree
        assert (buf.cpu().numpy().view(np.uint16) == host).all()
    q.close()


def _other_corners(frame, K):
    """The frame with other indices in its four corners: the changed rectangle of (this, frame) is the whole frame."""
    f = np.array(frame, np.int64)
    for y in (0, -1):
        for x in (0, -1):
            f[y, x] = (frame[y, x] + 1) % K
    return f


@pytest.mark.parametrize("name", [n for n in png_cases.names() if n != "pooled"])
def test_limit_cases_as_the_second_frame(nq, hd, name):
    """Crop mode (K = 256), frame 0 differs from frame 1 in the four corners: frame 1's chains encode the limit case's whole map, read
    as a rectangle by png_deflate_kernel<true>.  Host form, and device form at odd 2-byte offsets with the frames left unchanged."""
    _, idx, pal, S = png_cases.case(name)
    assert len(pal) == 256 and apng_ref.unchanged_index(pal) is None
    h, w = idx.shape
    frames = [_other_corners(idx, 256), idx]
    assert _rects(frames) == [[0, 0, w, h]] * 2
    want = apng_ref.encode(frames, pal, delays_cs=[3, 4], loop=1, segment_bytes=S)
    assert apng_ref.zlib_stream(idx, 256, S) in want                         # frame 1's stream is the still image's
    got, rects = _enc(hd, frames, pal, [3, 4], 1, S)
    assert rects.tolist() == [[0, 0, w, h]] * 2
    assert got == want, (name, len(got), len(want))
    buf, host, ptrs = png_cases.device_maps(frames)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        got = nq.encode_apng_device(q, ptrs, w, h, pal, [3, 4], 1, S)
    finally:
        q.close()
    assert got == want, (name, "device form")
    assert (buf.cpu().numpy().view(np.uint16) == host).all()


def test_dist_limit_in_mark_mode_with_unchanged_pixels(hd):
    """Mark mode (K = 255, every alpha 255; u = 255): frame 0 differs from the dist_limit map in pixel 0 and in every pixel from 1000
    on, so pixels 1 .. 999 of frame 1's body are u.  What is left of the map still takes the distance code past 15."""
    _, idx, _, S = png_cases.case("dist_limit")
    K = 255
    assert idx.max() < K
    pal = palette_of(K, np.random.default_rng(18))
    prev = (idx + 1) % K
    prev[0, 1:1000] = idx[0, 1:1000]
    frames = [prev, idx]
    assert apng_ref.unchanged_index(pal) == K and _rects(frames) == [[0, 0, idx.shape[1], 1]] * 2
    body = apng_ref.bodies(frames, pal)[1]
    assert (body[0, 1:1000] == K).all() and (body[0, 1000:] == idx[0, 1000:]).all() and body[0, 0] == idx[0, 0]
    stats = []
    png_ref.deflate(png_ref.raw_stream(body, K + 1), S, stats)
    assert stats[0].dist_depth == 16 and max(stats[0].dist_lens) == 15
    got, rects = _enc(hd, frames, pal, S=S)
    assert got == apng_ref.encode(frames, pal, segment_bytes=S)
    composes_back(got, frames, pal, "dist_limit in mark mode")


def test_one_frame_and_two_frames(nq, hd):
    rng = np.random.default_rng(5)
    K = 17
    a = rng.integers(0, K, (37, 91))
    for pal in (palette_of(K, rng), alpha_palette(K, rng)):
        got, rects = _enc(hd, [a], pal, [9], 4, S=7)
        assert got == nq.encode_png(a, pal, 7) == png_ref.encode(a, pal, 7) and rects.tolist() == [[0, 0, 91, 37]]
        for loop in (0, 5, 1 << 30):
            got, rects = _enc(hd, [a, a], pal, [3, 65535], loop)
            assert got == apng_ref.encode([a, a], pal, delays_cs=[3, 65535], loop=loop)
            assert rects.tolist() == [[0, 0, 91, 37], [0, 0, 1, 1]]
            composes_back(got, [a, a], pal, loop)
        b = a.copy()
        b[20:30, 40:80] = (b[20:30, 40:80] + 1) % K
        got, rects = _enc(hd, [a, b], pal, S=7)
        assert got == apng_ref.encode([a, b], pal, segment_bytes=7) and rects.tolist() == [[0, 0, 91, 37], [40, 20, 40, 10]]
        composes_back(got, [a, b], pal, "two frames")


# ---- the pipeline: a sprite over a static background ----
W, H, SPRITE = 128, 96, 16


def _sprite_at(i):
    return 9 + 23 * i, 13 + 17 * i


def _animation(transparent_back=False):
    back = synth.gradient_noise(W, H, 31)
    if transparent_back:
        back = np.zeros_like(back)                                          # ARGB 0: fully transparent
    rng = np.random.default_rng(8)
    sprite = (0xFF000000 | rng.integers(0, 1 << 24, (SPRITE, SPRITE))).astype(np.int64).astype(np.uint32).view(np.int32)
    frames = []
    for i in range(4):
        f = back.copy()
        x, y = _sprite_at(i)
        f[y:y + SPRITE, x:x + SPRITE] = sprite
        frames.append(f)
    return frames


def _rgba_of_argb(argb):
    v = np.asarray(argb).view(np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255, v >> 24], -1).astype(np.uint8)


def _inside_the_sprites_places(maps, rects, tile):
    tw, th = tile
    for i in range(1, len(maps)):
        inside = np.zeros((H, W), bool)                      # the sprite's old and new place, each expanded to tile boundaries
        for x, y in (_sprite_at(i - 1), _sprite_at(i)):
            inside[y // th * th:-(-(y + SPRITE) // th) * th, x // tw * tw:-(-(x + SPRITE) // tw) * tw] = True
        assert not ((maps[i] != maps[i - 1]) & ~inside).any(), (tile, i)
        ys, xs = np.nonzero(inside)
        x, y, w, h = rects[i]
        assert xs.min() <= x and x + w <= xs.max() + 1 and ys.min() <= y and y + h <= ys.max() + 1, (i, rects[i])


@pytest.mark.parametrize("tile", [(4, 4), (8, 8)])
@pytest.mark.parametrize("K", [255, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_convert_frames_to_apng_stores_only_the_tiles_the_sprite_touched(nq, kind, K, tile, tmp_path):
    frames = _animation()
    seeds = [5] * len(frames)
    delays = [4] * len(frames)
    pal, outs = nq.convert_frames(kind, frames, K, True, seeds=seeds, tile=tile)
    data, pal2, rects = nq.convert_frames_to_apng(kind, frames, K, True, delays_cs=delays, seeds=seeds, tile=tile, return_rects=True)
    assert (np.asarray(pal2) == np.asarray(pal)).all()
    maps = [o.index for o in outs]
    assert data == apng_ref.encode(maps, pal, delays_cs=delays)
    assert rects.tolist() == _rects(maps)
    _inside_the_sprites_places(maps, rects.tolist(), tile)
    _, parsed = apng_ref.parse(data)
    mark = apng_ref.unchanged_index(pal) is not None                         # the mode follows the palette the quantizer returned
    print("K = %d, alphas %s: %s mode" % (len(pal), sorted({(int(c) & 0xFFFFFFFF) >> 24 for c in pal}), "mark" if mark else "crop"))
    assert [p["blend"] for p in parsed] == [0] + [int(mark)] * 3
    stills = sum(len(f) for f in nq.encode_png(maps, [pal] * len(maps)))
    print("delta / stills bytes: %d / %d = %.3f (kind %d, K %d, tile %s)" % (len(data), stills, len(data) / stills, kind, K, tile))
    got, own = apng_ref.pillow_canvases(data), apng_ref.compose(data)
    for i, o in enumerate(outs):
        assert (got[i] == _rgba_of_argb(o.argb)).all() and (own[i] == _rgba_of_argb(o.argb)).all(), i
    path = tmp_path / "a.png"
    assert nq.write_apng(str(path), maps, pal, delays) == len(data) and path.read_bytes() == data


@pytest.mark.parametrize("K", [255, 16, 64])
def test_convert_frames_to_apng_over_a_transparent_background(nq, K):
    """LAB kind, a sprite over fully transparent pixels.  At 255 and at 16 colours the shared palette holds the transparent colour
    itself, an alpha-0 entry: the case nq_encode_gif_delta refuses, written here in crop mode.  At 64 colours the quantizer's merge
    loop has averaged the transparent bin with a neighbour and the entry comes out with alpha 2 (the CPU oracle gives the same
    palette): no alpha 0, delta GIF accepts it and flattens it, and the APNG is in crop mode all the same and keeps the alpha.  In
    all three every pixel outside the tiles the sprite touches is that one non-opaque entry in every frame, the old places too."""
    frames = _animation(transparent_back=True)
    seeds = [5] * len(frames)
    tile = (8, 8)
    pal, outs = nq.convert_frames(1, frames, K, True, seeds=seeds, tile=tile)
    alphas = sorted({(int(c) & 0xFFFFFFFF) >> 24 for c in pal})
    print("K = %d: palette of %d entries, alphas %s" % (K, len(pal), alphas))
    if K != 64:
        assert alphas[0] == 0
    assert alphas[0] < 255 and apng_ref.unchanged_index(pal) is None
    maps = [o.index for o in outs]
    if alphas[0] == 0:
        with pytest.raises(nq.NqError) as e:
            nq.encode_gif_delta(maps, pal)
        assert e.value.status == -1
    data, pal2, rects = nq.convert_frames_to_apng(1, frames, K, True, seeds=seeds, tile=tile, return_rects=True)
    assert (np.asarray(pal2) == np.asarray(pal)).all()
    assert data == apng_ref.encode(maps, pal)
    assert rects.tolist() == _rects(maps)
    _inside_the_sprites_places(maps, rects.tolist(), tile)
    _, parsed = apng_ref.parse(data)
    assert [p["blend"] for p in parsed] == [0] * 4
    got, own = apng_ref.pillow_canvases(data), apng_ref.compose(data)
    for i, (o, m) in enumerate(zip(outs, maps)):
        want = apng_ref.rgba_of(m, pal)
        assert (own[i] == want).all() and (got[i] == want).all(), i
        assert (want == _rgba_of_argb(o.argb)).all(), i                      # the canvases are what the quantizer returned
        x, y = _sprite_at(i)
        assert (want[y:y + SPRITE, x:x + SPRITE, 3] == 255).all()
        touched = np.zeros((H, W), bool)                                     # the tiles the sprite touches now
        touched[y // 8 * 8:-(-(y + SPRITE) // 8) * 8, x // 8 * 8:-(-(x + SPRITE) // 8) * 8] = True
        rest = want[~touched]
        assert (rest == rest[0]).all() and rest[0][3] == alphas[0], i         # everything else, the old places too, is clear again


def test_invalid_inputs_then_a_valid_call(nq, hd):
    L = hd._L
    a = np.zeros((4, 6), np.uint16)
    a[1, 2] = 2
    b = a.copy()
    b[2, 3] = 1
    pal = np.array([0xFF000000, 0xFFFFFFFF, 0xFF808080], np.uint32)

    def call(n=2, w=6, h=4, K=3, pal=pal, delays=None, loop=0, S=0, maps=None, cap=1 << 16, out=None, entry="nq_encode_apng", src=0, size=0):
        maps = [a, b] if maps is None else maps
        if src == 0:
            src = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in (maps * max(n, 1))[:max(n, 1)]])
        d = None if delays is None else np.array(delays, np.int32)
        buf = np.zeros(max(cap, 1), np.uint8) if out is None else out
        size = C.c_int64(-7) if size == 0 else size
        rects = np.full((max(n, 1), 4), -9, np.int32)
        rc = getattr(L, entry)(hd._h, n, src, w, h, None if pal is None else pal.ctypes.data, K, None if d is None else d.ctypes.data, loop, S,
                               buf.ctypes.data, cap, None if size is None else C.byref(size), rects.ctypes.data)
        return rc, None if size is None else size.value, buf, rects

    def valid():
        rc, size, buf, rects = call()
        assert rc == 0 and bytes(buf[:size]) == want and rects.tolist() == [[0, 0, 6, 4], [3, 2, 1, 1]]

    want = apng_ref.encode([a, b], pal)
    valid()
    for kw in ({"K": 0}, {"K": 257}, {"n": 0}, {"n": -3}, {"w": 0}, {"w": 65536}, {"h": 0}, {"h": 65536}, {"S": -1}, {"S": 65536}, {"loop": -1},
               {"delays": [0, -1]}, {"delays": [65536, 0]}, {"src": None}, {"pal": None}, {"size": None}, {"cap": -1},
               {"w": 65535, "h": 65535}):
        rc, size, _, rects = call(**kw)
        assert rc == -1, kw
        assert size in (-7, None) and (rects == -9).all(), kw     # rejected before any work
        valid()
    # an alpha-0 entry is no error here: the file switches to crop mode
    clear = pal.copy()
    clear[1] &= 0x00FFFFFF
    rc, size, buf, rects = call(pal=clear)
    assert rc == 0 and bytes(buf[:size]) == apng_ref.encode([a, b], clear) and rects.tolist() == [[0, 0, 6, 4], [3, 2, 1, 1]]
    valid()
    # an index >= K: in the first frame and in a later one (a bad index that differs from the frame before lies inside the changed
    # rectangle by definition; the case after this loop, the same bad index in both frames, is the one outside every rectangle)
    for which, at in ((0, (3, 5)), (1, (2, 3)), (1, (0, 0)), (0, (2, 3))):
        for bad in (3, 4, 300):                                   # K itself (the value of u), beyond it, beyond a byte
            maps = [a.copy(), b.copy()]
            maps[which][at] = bad
            rc, size, _, rects = call(maps=maps)
            assert rc == -1 and (rects == -9).all(), (which, at, bad)
            assert "index" in (L.nq_last_error(hd._h) or b"").decode()
            valid()
    both = [a.copy(), b.copy()]
    both[0][0, 0] = both[1][0, 0] = 3                        # the same bad index in both frames: unchanged, so outside the rectangle
                                                             # [3, 2, 1, 1], and still reported by the difference pass
    assert call(maps=both)[0] == -1
    valid()
    assert call(n=1, maps=[both[0]])[0] == -1                # and in a single frame
    valid()
    # cap smaller than the file: the size is reported, out is untouched
    for n, full in ((2, want), (1, png_ref.encode(a, pal))):
        small = np.full(len(full) - 1, 0xAB, np.uint8)
        rc, size, _, _ = call(n=n, cap=len(full) - 1, out=small)
        assert rc == -1 and size == len(full) and (small == 0xAB).all()
        rc, size, buf, _ = call(n=n, cap=len(full))
        assert rc == 0 and bytes(buf[:size]) == full
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
    # and the other encoders on this handle are what they were
    w1, h1 = np.array([6], np.int32), np.array([4], np.int32)
    assert P._encode(L, hd._h, "nq_encode_png", [a.ctypes.data], w1, h1, [pal], 0, hd._check) == [png_ref.encode(a, pal)]
    gif, rects = G._encode_delta(L, hd._h, "nq_encode_gif_delta", [a.ctypes.data, b.ctypes.data], 6, 4, pal, None, 0, 0, hd._check)
    assert gif == gif_delta_ref.encode([a, b], pal) and rects.tolist() == [[0, 0, 6, 4], [3, 2, 1, 1]]
    valid()
