"""GIF encoding on the GPU (nq_encode_gif / nq_encode_gif_device): the bytes equal the restatement in gif_ref.py for every K, segment
length, shape and content tried; mixed frame sizes at odd 2-byte offsets; convert_frames results read back by Pillow; a 4096^2 bench
image against Pillow's own encoder; every invalid input, each followed by a valid call on the same handle."""
import ctypes as C
import io

import numpy as np
import pytest

import gif_ref
from nquant.android_amd import gif as G
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL")
from PIL import GifImagePlugin, Image  # noqa: E402


@pytest.fixture(scope="module")
def hd(nq):
    h = G._Handle()
    yield h
    h.close()


def _enc(hd, maps, pal, delays=None, loop=0, S=0):
    w = np.array([a.shape[1] for a in maps], np.int32)
    h = np.array([a.shape[0] for a in maps], np.int32)
    maps = [np.ascontiguousarray(a, np.uint16) for a in maps]
    return G._encode(hd._L, hd._h, "nq_encode_gif", [a.ctypes.data for a in maps], w, h, pal, delays, loop, S, hd._check)


def _content(kind, h, w, K, rng):
    if kind == "noise":
        return rng.integers(0, K, (h, w))
    if kind == "flat":
        return np.full((h, w), K - 1)
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) * K // (h + w)) % K


@pytest.mark.parametrize("K", [2, 3, 4, 5, 16, 17, 255, 256])
def test_bytes_equal_the_restatement(hd, K):
    rng = np.random.default_rng(K)
    pal = (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.int64)
    for h, w in ((1, 1), (1, 777), (37, 91), (256, 256)):
        for S in (1, 7, 4096, 0, h * w):
            for kind in ("noise", "flat", "gradient"):
                idx = _content(kind, h, w, K, rng)
                got = _enc(hd, [idx], pal, S=S)
                want = gif_ref.encode(idx, pal, segment_pixels=S)
                assert got == want, (K, h, w, S, kind, len(got), len(want))


def test_noise_refills_the_table_in_long_chains(hd):
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 256, (512, 700))
    pal = 0xFF000000 | np.arange(256)
    for S in (65536, 3839, 0, 512 * 700):
        assert _enc(hd, [idx], pal, S=S) == gif_ref.encode(idx, pal, segment_pixels=S), S


def test_mixed_frame_sizes_at_odd_offsets(nq, hd):
    import torch
    rng = np.random.default_rng(4)
    shapes = [(37, 91), (1, 1), (256, 256), (5, 300), (64, 63)]
    K = 17
    frames = [rng.integers(0, K, s) for s in shapes]
    pal = (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.int64)
    delays = [3, 0, 65535, 12, 7]
    # one device buffer, every frame at an odd uint16 offset (2-byte but not 4-byte aligned), sentinels in between
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
        for loop in (0, 5, -1):
            got = nq.encode_gif_device(q, ptrs, [s[1] for s in shapes], [s[0] for s in shapes], pal, delays, loop, S)
            assert got == gif_ref.encode(frames, pal, delays_cs=delays, loop=loop, segment_pixels=S), (S, loop)
    assert nq.encode_gif(frames, pal, delays, 0, 0) == gif_ref.encode(frames, pal, delays_cs=delays, loop=0)
    assert (buf.cpu().numpy().view(np.uint16) == host).all()


def _pillow_frames(gif):
    old = GifImagePlugin.LOADING_STRATEGY
    GifImagePlugin.LOADING_STRATEGY = GifImagePlugin.LoadingStrategy.RGB_AFTER_DIFFERENT_PALETTE_ONLY
    try:
        im = Image.open(io.BytesIO(gif))
        out = []
        for i in range(im.n_frames):
            im.seek(i)
            im.load()
            out.append({"mode": im.mode, "index": np.array(im), "duration": im.info.get("duration"), "loop": im.info.get("loop"),
                        "transparency": im.info.get("transparency"), "palette": im.getpalette()})
        return im.n_frames, out
    finally:
        GifImagePlugin.LOADING_STRATEGY = old


@pytest.mark.parametrize("kind", [0, 1])
def test_convert_frames_decodes_in_pillow(nq, kind):
    frames = [synth.gradient_noise(60, 40, 10 + i) for i in range(3)]
    data, pal = nq.convert_frames_to_gif(kind, frames, 64, True, delays_cs=[5, 7, 9], loop=0, seeds=[1, 2, 3])
    _, outs = nq.convert_frames(kind, frames, 64, True, seeds=[1, 2, 3])
    assert data == gif_ref.encode([o.index for o in outs], pal, delays_cs=[5, 7, 9], loop=0)
    n, got = _pillow_frames(data)
    assert n == 3
    K = len(pal)
    rgb = [((int(c) >> 16) & 255, (int(c) >> 8) & 255, int(c) & 255) for c in pal]
    for i, g in enumerate(got):
        assert g["mode"] == "P"
        assert g["duration"] == [50, 70, 90][i] and g["loop"] == 0 and g["transparency"] is None
        assert [tuple(g["palette"][3 * k:3 * k + 3]) for k in range(K)] == rgb
        assert (g["index"] == outs[i].index).all(), i


def test_transparent_palette_entry(nq):
    """A palette entry with alpha 0 (here entry 7 of a convert_frames palette, made transparent) is the transparent index; other
    alpha values are dropped."""
    frames = [synth.gradient_noise(60, 40, 20 + i) for i in range(2)]
    _, outs = nq.convert_frames(0, frames, 32, True)
    pal = outs[0].palette.astype(np.int64) & 0xFFFFFFFF
    pal[7] &= 0x00FFFFFF
    pal[3] = (pal[3] & 0x00FFFFFF) | 0x80000000
    pal[9] &= 0x00FFFFFF
    maps = [o.index for o in outs]
    data = nq.encode_gif(maps, pal, [4, 4], 3)
    # with a transparent entry Pillow composites later frames over earlier ones: the bytes are the check there
    assert data == gif_ref.encode(maps, pal, delays_cs=[4, 4], loop=3)
    n, got = _pillow_frames(data)
    assert n == 2 and got[0]["transparency"] == 7 and got[0]["loop"] == 3
    assert (got[0]["index"] == maps[0]).all()
    # one frame: the extension is written for the transparency alone
    one = nq.encode_gif(maps[0], pal)
    assert one == gif_ref.encode(maps[0], pal)
    im = Image.open(io.BytesIO(one))
    im.load()
    assert im.info["transparency"] == 7 and (np.array(im) == maps[0]).all()


def test_bench_image_4096_against_pillow(nq):
    img = synth.gradient_noise(4096, 4096, 3)
    q = nq.PnnLABQuantizer(img)
    out = q.convert(256, True)
    q.close()
    pal = out.palette
    data = nq.encode_gif(out.index, pal)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert (np.array(im) == out.index).all()
    ref = Image.fromarray(out.index.astype(np.uint8), "P")
    ref.putpalette([v for c in pal for v in (((int(c) >> 16) & 255), ((int(c) >> 8) & 255), int(c) & 255)])
    b = io.BytesIO()
    ref.save(b, "GIF")
    assert len(data) <= 1.05 * len(b.getvalue()), (len(data), len(b.getvalue()))


def test_invalid_inputs_then_a_valid_call(nq, hd):
    L = hd._L
    idx = np.zeros((4, 6), np.uint16)
    idx[1, 2] = 2
    pal = np.array([0xFF000000, 0xFFFFFFFF, 0xFF808080], np.uint32)

    def call(n=1, w=6, h=4, K=3, delays=None, loop=0, S=0, maps=None, cap=1 << 16, out=None, entry="nq_encode_gif"):
        maps = [idx] if maps is None else maps
        ws, hs = np.full(max(n, 1), w, np.int32), np.full(max(n, 1), h, np.int32)
        src = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in (maps * max(n, 1))[:max(n, 1)]])
        d = None if delays is None else np.array(delays, np.int32)
        buf = np.zeros(max(cap, 1), np.uint8) if out is None else out
        size = C.c_int64(-7)
        rc = getattr(L, entry)(hd._h, n, src, ws.ctypes.data, hs.ctypes.data, pal.ctypes.data, K, None if d is None else d.ctypes.data, loop,
                               S, buf.ctypes.data, cap, C.byref(size))
        return rc, size.value, buf

    want = gif_ref.encode(idx, pal)
    for kw in ({"K": 0}, {"K": 257}, {"n": 0}, {"w": 0}, {"h": 65536}, {"S": -1}, {"loop": -2}, {"loop": 65536},
               {"n": 2, "delays": [0, -1]}, {"n": 2, "delays": [65536, 0]}):
        rc, size, _ = call(**kw)
        assert rc == -1, kw
        assert size == -7, kw                      # rejected before any work
        rc, size, buf = call()
        assert rc == 0 and bytes(buf[:size]) == want, kw
    bad = idx.copy()
    bad[3, 5] = 3
    assert call(maps=[bad])[0] == -1
    assert "index" in (L.nq_last_error(hd._h) or b"").decode()
    rc, size, buf = call()
    assert rc == 0 and bytes(buf[:size]) == want
    # cap smaller than the file: the size is reported, out is untouched
    small = np.full(len(want) - 1, 0xAB, np.uint8)
    rc, size, _ = call(cap=len(want) - 1, out=small)
    assert rc == -1 and size == len(want) and (small == 0xAB).all()
    rc, size, buf = call(cap=len(want))
    assert rc == 0 and bytes(buf[:size]) == want
    # odd index pointers
    raw = np.zeros(idx.size + 1, np.uint16)
    odd = np.frombuffer(raw.data, np.uint8)[1:1 + 2 * idx.size]
    assert odd.ctypes.data % 2 == 1
    rc, size, _ = call(maps=[odd])
    assert rc == -1
    rc, size, buf = call(entry="nq_encode_gif")
    assert rc == 0 and bytes(buf[:size]) == want
