"""Lossy mode of the GIF encoders on the GPU (nq_encode_gif_lossy* / nq_encode_gif_delta_lossy*): the bytes equal the restatement in
gif_lossy_ref.py for every K, shape, segment length, threshold, palette and content tried, and where a case says "substitutes" the
restatement did take the lossy branch; the table refills under it; lossy = 0 is the lossless exports byte for byte; frames at odd 2-byte
offsets in device memory, never written; delta mode with the lossless call's rectangles and a canvas within the threshold; the
convert -> hold -> lossy delta pipeline on one handle; invalid thresholds and an index >= K."""
import ctypes as C
import io

import numpy as np
import pytest

import gif_delta_ref
import gif_lossy_ref as R
import gif_ref
from gif_delta_cases import palette_of
from nquant.android_amd import gif as G
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

KS = (2, 3, 16, 17, 255, 256)
SHAPES = ((1, 1), (1, 777), (37, 91), (128, 128))
SEGMENTS = (1, 7, 4096, 0)
LOSSY = (1, 8, 40, 255)


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _enc(hd, maps, pal, delays=None, loop=0, S=0, lossy=0):
    w = np.array([a.shape[1] for a in maps], np.int32)
    h = np.array([a.shape[0] for a in maps], np.int32)
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    return G._encode(hd._L, hd._h, "nq_encode_gif", [a.ctypes.data for a in maps], w, h, pal, delays, loop, S, hd._check, lossy)


def _enc_delta(hd, maps, pal, delays=None, loop=0, S=0, lossy=0):
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    h, w = maps[0].shape
    return G._encode_delta(hd._L, hd._h, "nq_encode_gif_delta", [a.ctypes.data for a in maps], w, h, pal, delays, loop, S, hd._check, lossy)


def _duplicates(K, rng):
    """About K / 3 distinct colours, close to one another, every one at several indices."""
    base = 0xFF000000 | (0x40 + rng.integers(0, 24, max(K // 3, 1))) << 16 | (0x80 + rng.integers(0, 24, max(K // 3, 1))) << 8 | 0x20
    return base[rng.integers(0, base.size, K)].astype(np.int64)


def _palette(kind, K, rng):
    return {"random": palette_of, "ramp": lambda K, rng: R.ramp_palette(K), "duplicates": _duplicates}[kind](K, rng)


def _alternating(h, w, K):
    """Neighbouring pixels flip between two adjacent entries, and the pair moves up one entry every 8 pixels: what a dither produces."""
    y, x = np.mgrid[0:h, 0:w]
    return (x + y) // 8 % (K - 1) + ((x + y) & 1)


def _content(kind, h, w, K, rng):
    if kind == "noise":
        return rng.integers(0, K, (h, w))
    if kind == "gradient":
        return ((np.arange(h)[:, None] + np.arange(w)[None, :]) * K // (h + w)) % K
    if kind == "alternating":
        return _alternating(h, w, K)
    return R.dithered(h, w, K, rng)


@pytest.mark.parametrize("K", KS)
def test_bytes_equal_the_restatement(hd, K):
    """Every palette, shape and content at every segment length; the threshold goes round so that every (segment, threshold) pair is
    met for every palette (16 pairs over 4 shapes x 3 contents x 4 segments), the large shape at two segment lengths."""
    rng = np.random.default_rng(100 + K)
    substituted = 0
    for pi, pkind in enumerate(("random", "ramp", "duplicates")):
        pal = _palette(pkind, K, rng)
        turn = pi
        for h, w in SHAPES:
            for kind in ("noise", "gradient", "alternating"):
                idx = _content(kind, h, w, K, rng)
                for si, S in enumerate(SEGMENTS if h * w < 10000 else (4096, 0)):
                    lossy = LOSSY[(si + turn) % 4]
                    want, subs = R.encode(idx, pal, segment_pixels=S, lossy=lossy)
                    got = _enc(hd, [idx], pal, S=S, lossy=lossy)
                    assert got == want, (K, pkind, h, w, kind, S, lossy, len(got), len(want), subs)
                    substituted += subs
                turn += 1
    assert substituted > 0, K


@pytest.mark.parametrize("K", [16, 17, 255, 256])
@pytest.mark.parametrize("kind", ["alternating", "dithered"])
def test_ramp_palette_substitutes(hd, K, kind):
    """A grey ramp with dither-like content: every threshold from the ramp's step on finds candidates, 255 makes every entry one."""
    rng = np.random.default_rng(K)
    pal = R.ramp_palette(K)
    step = 255 // (K - 1)                                # the smallest distance between neighbouring entries
    for h, w in ((37, 91), (128, 128)):
        idx = _content(kind, h, w, K, rng)
        for S in (4096, 0):
            lossless = gif_ref.encode(idx, pal, segment_pixels=S)
            for lossy in LOSSY:
                want, subs = R.encode(idx, pal, segment_pixels=S, lossy=lossy)
                got = _enc(hd, [idx], pal, S=S, lossy=lossy)
                assert got == want, (K, kind, h, w, S, lossy, len(got), len(want), subs)
                if lossy >= step:
                    assert subs > 0 and len(want) < len(lossless), (K, kind, h, w, S, lossy)
                else:
                    assert subs == 0 and want == lossless, (K, kind, h, w, S, lossy)
                dec = gif_ref.parse(got)[2][0]["index"]
                assert R.within(dec, idx, pal, lossy).all() and int((dec != idx).sum()) == subs


def test_several_frames_with_a_transparent_entry_substitutes(hd):
    """Entries 7 and 9 have alpha 0: 7 is T, 9 an ordinary colour.  Frames of different sizes, delays, a loop count."""
    rng = np.random.default_rng(9)
    K = 16
    pal = _duplicates(K, rng)
    pal[7] &= 0x00FFFFFF
    pal[9] &= 0x00FFFFFF
    frames = []
    for h, w in ((64, 64), (37, 91), (1, 5)):
        f = rng.integers(0, K, (h, w))
        f[rng.random(f.shape) < 0.3] = 7
        frames.append(f)
    for S in (0, 100):
        for lossy in (8, 255):
            want, subs = R.encode(frames, pal, [3, 0, 9], 2, S, lossy)
            assert subs > 0
            got = _enc(hd, frames, pal, [3, 0, 9], 2, S, lossy)
            assert got == want, (S, lossy)
            for f, p in zip(frames, gif_ref.parse(got)[2]):
                assert p["transparency"] == 7 and ((p["index"] == 7) == (f == 7)).all() and R.within(p["index"], f, pal, lossy).all()


def test_table_refills_under_lossy(hd):
    """200 x 200 noise over 256 colours as ONE chain at lossy 40: the dictionary reaches 4096 and is cleared several times."""
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 256, (200, 200))
    for pkind in ("random", "ramp"):
        pal = _palette(pkind, 256, rng)
        want, subs = R.encode(idx, pal, segment_pixels=40000, lossy=40)
        assert subs > 0
        assert (len(want) - 800) * 8 // 12 > 3 * 4096, len(want)         # more codes than three full tables hold
        got = _enc(hd, [idx], pal, S=40000, lossy=40)
        assert got == want, (pkind, len(got), len(want), subs)
        assert R.within(gif_ref.parse(got)[2][0]["index"], idx, pal, 40).all()


def _raw(hd, entry, maps, pal, S, lossy, delta, cap=1 << 20, K=None, device_ptrs=None):
    """A direct call of one of the eight exports: (rc, *out_size, file buffer, rectangles); lossy None: the export has no such argument."""
    L = hd._L
    n = len(maps)
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    src = (C.c_void_p * n)(*(device_ptrs if device_ptrs is not None else [m.ctypes.data for m in maps]))
    pal = np.ascontiguousarray(np.asarray(pal).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    buf = np.zeros(cap, np.uint8)
    size = C.c_int64(-7)
    rects = np.full((n, 4), -9, np.int32)
    tail = (S,) if lossy is None else (S, lossy)
    if delta:
        h, w = maps[0].shape
        rc = getattr(L, entry)(hd._h, n, src, w, h, pal.ctypes.data, len(pal) if K is None else K, None, 0, *tail, buf.ctypes.data, cap,
                               C.byref(size), rects.ctypes.data)
    else:
        ws = np.array([m.shape[1] for m in maps], np.int32)
        hs = np.array([m.shape[0] for m in maps], np.int32)
        rc = getattr(L, entry)(hd._h, n, src, ws.ctypes.data, hs.ctypes.data, pal.ctypes.data, len(pal) if K is None else K, None, 0, *tail,
                               buf.ctypes.data, cap, C.byref(size))
    return rc, size.value, buf, rects


def test_lossy_zero_is_the_lossless_export(nq, hd):
    import torch
    rng = np.random.default_rng(3)
    K = 17
    pal = R.ramp_palette(K)
    frames = [R.dithered(48, 64, K, rng)]
    for i in range(2):
        f = frames[-1].copy()
        f[5 + 7 * i:25 + 7 * i, 9 + 11 * i:41 + 11 * i] = R.dithered(20, 32, K, rng)
        frames.append(f)
    dev = [torch.from_numpy(np.ascontiguousarray(f, np.uint16).view(np.int16).reshape(-1).copy()).cuda() for f in frames]
    ptrs = [d.data_ptr() for d in dev]
    for old, new, delta, p in (("nq_encode_gif", "nq_encode_gif_lossy", False, None),
                               ("nq_encode_gif_device", "nq_encode_gif_lossy_device", False, ptrs),
                               ("nq_encode_gif_delta", "nq_encode_gif_delta_lossy", True, None),
                               ("nq_encode_gif_delta_device", "nq_encode_gif_delta_lossy_device", True, ptrs)):
        for S in (0, 100):
            rc0, n0, b0, r0 = _raw(hd, old, frames, pal, S, None, delta, device_ptrs=p)
            rc1, n1, b1, r1 = _raw(hd, new, frames, pal, S, 0, delta, device_ptrs=p)
            assert rc0 == 0 and rc1 == 0 and n0 == n1 and bytes(b0[:n0]) == bytes(b1[:n1]), (new, S)
            assert (r0 == r1).all(), new
            want = gif_delta_ref.encode(frames, pal, segment_pixels=S) if delta else gif_ref.encode(frames, pal, loop=0, segment_pixels=S)
            assert bytes(b1[:n1]) == want, (new, S)
            # and the new export does encode lossily when asked to
            rc2, n2, b2, r2 = _raw(hd, new, frames, pal, S, 40, delta, device_ptrs=p)
            want2, subs = (R.encode_delta if delta else R.encode)(frames, pal, None, 0, S, 40)
            assert rc2 == 0 and subs > 0 and bytes(b2[:n2]) == want2 and (r2 == r0).all(), (new, S)


def test_device_form_at_odd_offsets_leaves_the_frames_alone(nq, hd):
    import torch
    rng = np.random.default_rng(4)
    shapes = [(37, 91), (1, 1), (128, 128), (5, 300), (64, 63)]
    K = 17
    pal = R.ramp_palette(K)
    frames = [R.dithered(h, w, K, rng) for h, w in shapes]
    delays = [3, 0, 65535, 12, 7]
    offs, off = [], 1
    for f in frames:
        offs.append(off)
        off += f.size + 3
        off += 1 - off % 2
    host = np.full(off, 0xFFFF, np.uint16)
    for f, o in zip(frames, offs):
        host[o:o + f.size] = f.reshape(-1)
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    ptrs = [buf.data_ptr() + 2 * o for o in offs]
    assert all(p % 4 == 2 for p in ptrs)
    q = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    for S in (0, 7, 1000):
        for lossy in (16, 255):
            want, subs = R.encode(frames, pal, delays, 5, S, lossy)
            assert subs > 0
            got = nq.encode_gif_device(q, ptrs, [s[1] for s in shapes], [s[0] for s in shapes], pal, delays, 5, S, lossy=lossy)
            assert got == want, (S, lossy)
    assert nq.encode_gif(frames, pal, delays, 5, 0, lossy=16) == R.encode(frames, pal, delays, 5, 0, 16)[0]
    # delta form: frames of one size at offsets that differ modulo 16 bytes
    same = [R.dithered(48, 64, K, rng)]
    for i in range(2):
        f = same[-1].copy()
        f[10 + 9 * i:30 + 9 * i, 8 + 13 * i:40 + 13 * i] = R.dithered(20, 32, K, rng)
        same.append(f)
    offs2, off = [], 1
    for i, f in enumerate(same):
        offs2.append(off)
        off += f.size + 2 * i + 1
        off += 1 - off % 2
    host2 = np.full(off + 8, 0xFFFF, np.uint16)
    for f, o in zip(same, offs2):
        host2[o:o + f.size] = f.reshape(-1)
    buf2 = torch.from_numpy(host2.view(np.int16)).cuda()
    ptrs2 = [buf2.data_ptr() + 2 * o for o in offs2]
    assert all(p % 4 == 2 for p in ptrs2) and len({p % 16 for p in ptrs2}) > 1
    for S in (0, 50):
        want, subs = R.encode_delta(same, pal, None, 0, S, 16)
        assert subs > 0
        got, rects = nq.encode_gif_delta_device(q, ptrs2, 64, 48, pal, None, 0, S, return_rects=True, lossy=16)
        assert got == want and [tuple(r) for r in rects.tolist()] == gif_delta_ref.rectangles(same), S
    assert (buf.cpu().numpy().view(np.uint16) == host).all() and (buf2.cpu().numpy().view(np.uint16) == host2).all()
    q.close()


@pytest.mark.parametrize("K", [17, 256])
def test_delta_mode_with_a_moving_block(hd, K):
    """Three 64 x 48 frames, a block that moves: K = 17 marks the unchanged pixels (u = 17), K = 256 crops only."""
    rng = np.random.default_rng(K)
    pal = R.ramp_palette(K)
    frames = [R.dithered(48, 64, K, rng)]
    for i in range(2):
        f = frames[-1].copy()
        f[10 + 9 * i:30 + 9 * i, 8 + 13 * i:40 + 13 * i] = _alternating(20, 32, K)
        frames.append(f)
    delays = [4, 5, 6]
    for S in (0, 50):
        _, rects0 = _enc_delta(hd, frames, pal, delays, 0, S)
        for lossy in LOSSY:
            want, subs = R.encode_delta(frames, pal, delays, 0, S, lossy)
            got, rects = _enc_delta(hd, frames, pal, delays, 0, S, lossy)
            assert got == want, (K, S, lossy, len(got), len(want), subs)
            assert (rects == rects0).all() and [tuple(r) for r in rects.tolist()] == gif_delta_ref.rectangles(frames)
            if lossy >= 255 // (K - 1) and S == 0:
                assert subs > 0, (K, lossy)
            canvases = gif_delta_ref.compose(got)
            assert len(canvases) == 3
            for i, (c, f) in enumerate(zip(canvases, frames)):
                assert (c >= 0).all() and (c < K).all() and R.within(c, f, pal, lossy).all(), (K, S, lossy, i)
            assert len(got) <= gif_ref.max_bytes([f.shape for f in frames], S)


@pytest.mark.parametrize("kind", [0, 1])
def test_convert_hold_and_lossy_delta_on_one_handle(nq, kind):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    frames = [synth.gradient_noise(60, 40, 10 + i) for i in range(3)]
    seeds = [5, 5, 5]
    data, pal = nq.convert_frames_to_gif(kind, frames, 64, True, seeds=seeds, delta=True, hold=4, lossy=16)
    pal0, outs = nq.convert_frames(kind, frames, 64, True, seeds=seeds)
    assert (np.asarray(pal0) == np.asarray(pal)).all()
    held, _ = nq.hold_frames(frames, [o.index for o in outs], 4)
    want, subs = R.encode_delta(held, pal, None, 0, 0, 16)
    assert data == want
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == 3
    for c, m in zip(gif_delta_ref.compose(data), held):
        assert R.within(c, m, pal, 16).all()
    lossless, _ = nq.convert_frames_to_gif(kind, frames, 64, True, seeds=seeds, delta=True, hold=4)
    assert lossless == gif_delta_ref.encode(held, pal)
    print("kind %d: lossy 16 / lossless bytes %d / %d, %d pixels substituted" % (kind, len(data), len(lossless), subs))
    assert len(data) <= len(lossless)


def test_invalid_thresholds_then_a_valid_call(hd):
    rng = np.random.default_rng(6)
    K = 17
    pal = R.ramp_palette(K)
    a = R.dithered(24, 30, K, rng)
    b = a.copy()
    b[3:9, 4:20] = R.dithered(6, 16, K, rng)
    for entry, delta, ref in (("nq_encode_gif_lossy", False, R.encode), ("nq_encode_gif_delta_lossy", True, R.encode_delta)):
        want = ref([a, b], pal, None, 0, 0, 40)[0]
        for bad in (-1, 256):
            rc, size, _, rects = _raw(hd, entry, [a, b], pal, 0, bad, delta)
            assert rc == -1 and size == -7 and (rects == -9).all(), (entry, bad)
            assert "lossy" in (hd._L.nq_last_error(hd._h) or b"").decode()
            rc, size, buf, _ = _raw(hd, entry, [a, b], pal, 0, 40, delta)
            assert rc == 0 and bytes(buf[:size]) == want, (entry, bad)
        # an index >= K is still reported after the encoding, and the handle goes on
        c = b.copy()
        c[20, 25] = K
        rc, _, _, _ = _raw(hd, entry, [a, c], pal, 0, 40, delta)
        assert rc == -1 and "index" in (hd._L.nq_last_error(hd._h) or b"").decode(), entry
        rc, size, buf, _ = _raw(hd, entry, [a, b], pal, 0, 40, delta)
        assert rc == 0 and bytes(buf[:size]) == want, entry
        # cap smaller than the file: the size is reported
        rc, size, _, _ = _raw(hd, entry, [a, b], pal, 0, 40, delta, cap=len(want) - 1)
        assert rc == -1 and size == len(want), entry
    with pytest.raises(G.NqError):
        _enc(hd, [a], pal, lossy=256)
    assert _enc(hd, [a], pal, lossy=255) == R.encode(a, pal, lossy=255)[0]
