"""WebP encoding on the GPU (nq_encode_webp / nq_encode_webp_device): the bytes and the rectangles of every case of webp_cases.py equal
the restatement in webp_ref.py, through the host form and through the device form on a caller's stream, with nq_get_device_bytes the
same before and after; n = 1 ignores delta; an index >= K is reported, also outside the rectangle; a too-small cap reports the size
and leaves `out` alone; calls of different geometry do not see each other; convert_frames_to_webp composes back to the converter's
ARGB output.  The limit cases of webp_cases.py (full chains, the farthest copy, items of up to 46 bits, more chains than the grid holds,
more segments than a round of the scan, a file past the gather's one pass) run through the same test as the small ones."""
import ctypes as C

import numpy as np
import pytest

import webp_cases
import webp_ref

pytestmark = pytest.mark.gpu


def _want_rects(frames, kw):
    return [list(r) for r in webp_ref.rectangles(frames, kw.get("delta", True))]


def _device_maps(frames, torch):
    """One device buffer holding every frame at an odd uint16 offset (2-byte but not 4-byte aligned), sentinels in between."""
    offs, off = [], 1
    for f in frames:
        offs.append(off)
        off += f.size + 2
        off += 1 - off % 2
    host = np.full(off + 8, 0xFFFF, np.uint16)
    for f, o in zip(frames, offs):
        host[o:o + f.size] = np.asarray(f).reshape(-1)
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    return buf, host, [buf.data_ptr() + 2 * o for o in offs]


@pytest.fixture(scope="module")
def stream(nq):
    import torch
    return torch.cuda.Stream()


@pytest.mark.parametrize("name", webp_cases.names())
def test_bytes_and_rectangles_equal_the_restatement(nq, stream, name):
    import torch
    _, frames, pal, kw = webp_cases.case(name)
    want, _ = webp_cases.restated(name)
    h, w = np.asarray(frames[0]).shape
    args = dict(delays_cs=kw.get("delays_cs"), loop=kw.get("loop", 0), band_bits=kw.get("band_bits", 0), delta=kw.get("delta", True))
    before = nq.device_bytes()
    got, rects = nq.encode_webp(frames, pal, return_rects=True, **args)
    assert nq.device_bytes() == before
    assert rects.tolist() == _want_rects(frames, kw), name
    assert got == want, (name, len(got), len(want))
    assert len(got) <= nq.webp_max_bytes(len(frames), w, h, args["band_bits"])
    buf, host, ptrs = _device_maps(frames, torch)
    assert all(p % 4 == 2 for p in ptrs)
    torch.cuda.synchronize()
    before = nq.device_bytes()
    got, rects = nq.encode_webp_device(ptrs, w, h, pal, stream=stream.cuda_stream, return_rects=True, **args)
    assert nq.device_bytes() == before
    assert rects.tolist() == _want_rects(frames, kw), name
    assert got == want, (name, len(got), len(want))
    assert (buf.cpu().numpy().view(np.uint16) == host).all()                 # the maps are never written


def test_more_chains_than_the_grid_holds(nq):
    """The many_bands and many_frames cases are there for a workgroup's second chain: they must hold more chains than the grid of
    4 workgroups per compute unit of this device, whatever its size."""
    import torch
    grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    for name in ("many_bands_K2", "many_bands_K256", "many_frames"):
        chains = sum(len(image) for image in webp_cases.restated(name)[1])
        print(name, chains, grid)
        assert chains > grid, (name, chains, grid)


def test_a_refused_width_leaves_the_next_call_what_it_was(nq):
    """16384 wide is the limit at K = 16 and past it at K = 17: NQ_ERR_INVALID, and the same map at K = 16 encodes as before."""
    _, frames, pal, kw = webp_cases.case("full_chain_K16")
    with pytest.raises(nq.NqError) as e:
        nq.encode_webp(frames, np.concatenate([pal, pal[:1]]), **kw)
    assert e.value.status == -1 and "packed width 16384" in str(e.value)
    assert nq.encode_webp(frames, pal, **kw) == webp_cases.restated("full_chain_K16")[0]


def test_one_frame_ignores_delta(nq):
    _, frames, pal, _ = webp_cases.case("alpha_palette")
    a, ra = nq.encode_webp(frames, pal, delta=True, return_rects=True)
    b, rb = nq.encode_webp(frames, pal, delta=False, return_rects=True)
    assert a == b == webp_cases.restated("alpha_palette")[0] and ra.tolist() == rb.tolist() == [[0, 0, 33, 21]]


def _raw(nq, maps, pal, n=None, delta=1, cap=1 << 16, out=None, band_bits=0):
    L = nq.load_library()
    maps = [np.ascontiguousarray(m, np.uint16) for m in maps]
    n = len(maps) if n is None else n
    h, w = maps[0].shape
    pal = np.ascontiguousarray(pal, np.uint32)
    src = (C.c_void_p * n)(*[m.ctypes.data for m in maps])
    buf = np.full(max(cap, 1), 0xAB, np.uint8) if out is None else out
    size = C.c_int64(-7)
    rects = np.full((n, 4), -9, np.int32)
    rc = L.nq_encode_webp(0, n, src, w, h, pal.ctypes.data, int(pal.size), None, 0, band_bits, delta, buf.ctypes.data, cap, C.byref(size),
                          rects.ctypes.data)
    return rc, size.value, buf, rects, (L.nq_last_error(None) or b"").decode()


def test_an_index_past_the_palette_is_reported(nq):
    a = np.zeros((4, 6), np.uint16)
    a[1, 2] = 2
    b = a.copy()
    b[2, 3] = 1
    pal = np.array([0xFF000000, 0xFFFFFFFF, 0xFF808080], np.uint32)
    want = webp_ref.encode([a, b], pal)
    rc, size, buf, rects, _ = _raw(nq, [a, b], pal)
    assert rc == 0 and bytes(buf[:size]) == want and rects.tolist() == [[0, 0, 6, 4], [2, 2, 2, 1]]
    for delta in (1, 0):
        for which, at in ((0, (3, 5)), (1, (2, 3)), (1, (0, 0))):
            for bad in (3, 4, 300):
                maps = [a.copy(), b.copy()]
                maps[which][at] = bad
                rc, _, _, rects, text = _raw(nq, maps, pal, delta=delta)
                assert rc == -1 and (rects == -9).all() and "index" in text, (delta, which, at, bad)
        both = [a.copy(), b.copy()]
        both[0][0, 0] = both[1][0, 0] = 3              # the same bad index in both frames: unchanged, so outside the rectangle
        rc, _, _, _, text = _raw(nq, both, pal, delta=delta)
        assert rc == -1 and "index" in text
        rc, _, _, _, text = _raw(nq, [both[0]], pal, delta=delta)            # and in a single frame
        assert rc == -1 and "index" in text
        rc, size, buf, _, _ = _raw(nq, [a, b], pal, delta=delta)             # the next call is what it was
        assert rc == 0 and bytes(buf[:size]) == webp_ref.encode([a, b], pal, delta=bool(delta))


def test_a_cap_too_small_reports_the_size_and_leaves_out_alone(nq):
    for name in ("alpha_palette", "anim_45x37_K4_delta"):
        _, frames, pal, _ = webp_cases.case(name)
        full = webp_ref.encode(frames, pal, loop=0, delta=True)
        small = np.full(len(full) - 1, 0xAB, np.uint8)
        rc, size, _, _, text = _raw(nq, frames, pal, cap=len(full) - 1, out=small)
        assert rc == -1 and size == len(full) and (small == 0xAB).all() and "cap" in text
        rc, size, buf, _, _ = _raw(nq, frames, pal, cap=len(full))
        assert rc == 0 and size == len(full) and bytes(buf) == full


def test_calls_of_different_geometry_are_independent(nq):
    order = ["four_bands", "K2_w9", "anim_48x40_K17_delta", "three_bands", "four_bands", "constant", "anim_45x37_K4_whole", "K2_w9"]
    for name in order:
        _, frames, pal, kw = webp_cases.case(name)
        assert nq.encode_webp(frames, pal, **kw) == webp_cases.restated(name)[0], name


def test_write_webp(nq, tmp_path):
    _, frames, pal, kw = webp_cases.case("anim_45x37_K200_delta")
    path = tmp_path / "a.webp"
    want = webp_cases.restated("anim_45x37_K200_delta")[0]
    assert nq.write_webp(str(path), frames, pal, **kw) == len(want) and path.read_bytes() == want


# ---- the pipeline: a sprite over a static background ----
def _rgba_of_argb(argb):
    v = np.asarray(argb).view(np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255, v >> 24], -1).astype(np.uint8)


def test_convert_frames_to_webp_composes_back_to_the_converters_output(nq):
    from nquant.android_amd import synth
    W, H, S = 96, 64, 12
    back = synth.gradient_noise(W, H, 31)
    rng = np.random.default_rng(8)
    sprite = (0xFF000000 | rng.integers(0, 1 << 24, (S, S))).astype(np.int64).astype(np.uint32).view(np.int32)
    frames = []
    for i in range(4):
        f = back.copy()
        f[9 + 11 * i:9 + 11 * i + S, 13 + 17 * i:13 + 17 * i + S] = sprite
        frames.append(f)
    seeds, delays = [5] * 4, [4, 0, 9, 2]
    pal, outs = nq.convert_frames(1, frames, 64, True, seeds=seeds, tile=(8, 8))
    data, pal2, rects = nq.convert_frames_to_webp(1, frames, 64, True, delays_cs=delays, loop=2, seeds=seeds, tile=(8, 8), return_rects=True)
    assert (np.asarray(pal2) == np.asarray(pal)).all()
    maps = [o.index for o in outs]
    assert data == webp_ref.encode(maps, pal, delays_cs=delays, loop=2)
    assert rects.tolist() == [list(r) for r in webp_ref.rectangles(maps)]
    assert all(r[2] * r[3] < W * H // 2 for r in rects.tolist()[1:])          # the later frames store the sprite's places only
    own = webp_ref.compose(data)
    for i, o in enumerate(outs):
        assert (own[i] == _rgba_of_argb(o.argb)).all(), i
    still, pal3 = nq.convert_to_webp(1, frames[0], 64, True, seed=5, tile=(8, 8))
    assert (webp_ref.compose(still)[0] == webp_ref.rgba_of(webp_ref.read(still)["frames"][0]["index"], pal3)).all()
    whole, _ = nq.convert_frames_to_webp(1, frames, 64, True, seeds=seeds, tile=(8, 8), delta=False)
    assert whole == webp_ref.encode(maps, pal, delta=False) and len(whole) > len(data)
