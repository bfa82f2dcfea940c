"""The op table of tests/test_gpu_handle_lifecycle.py (tests/test_lifecycle_cpu.py checks it without a GPU).  A helper, not a test
module and not a conftest.

An OP is one library call -- or the fixed short chain that makes one result (pnnquan_device + dither_device) -- run on a handle it is
GIVEN, at one of three size variants, with its results in a canonical form next to what they have to be:

    got, want = OPS[name].run(env, q, variant)        # two dicts with the same keys; compare(got, want, what) asserts equality

Device outputs come back WHOLE, guard elements included, as stream_gate.make_buffer / make_output lay them out, and `want` holds the
sentinel around the reference; the device inputs come back too ("in:..." keys) and have to be untouched.  Expected values are the
restatements of tests/*_ref.py and the CPU oracle, never the library; they are computed once per op, variant (and, for the quantizer,
handle kind and tile) and kept for the process.

The frame and encoder ops are the cases of stream_gate.py (dispatch: test_gpu_streams._call) at WIDE 48 x 40, NARROW 45 x 37 one element
off alignment (3 frames) and LARGE 181 x 187 (5 frames, K = 256, one element off): LARGE makes every buffer and table of a handle
larger than the next small call needs -- three LZW chains and two deflate chains per frame, 3 x 3 partly filled orient tiles.  Every
`_device` op has its host form on the same handle (through the private helpers of the package, which take a handle), and the lossy and
local-table GIF encoders, which stream_gate.py does not have, are added in both forms.  The quantizer ops run on the kind of the handle
they are given (q.KIND), so every op is valid on both handle kinds.
  Every export that takes a handle is called by an op or is a getter or setter that
tests/test_lifecycle_cpu.py lists by name."""
import ctypes as C

import numpy as np

import stream_gate as G

VARIANTS = ("WIDE", "NARROW", "LARGE")
SMALL = ("WIDE", "NARROW")
SHAPE = {"WIDE": G.WIDE, "NARROW": G.NARROW, "LARGE": G.LARGE}
FRAMES = {"WIDE": 3, "NARROW": 3, "LARGE": G.LARGE_FRAMES}
TILES = ((16, 16), (8, 8))
SEQ, TILED, LOOKUP = 0, 1, 2
OPT_CELL_LISTS, OPT_FAST_DITHER, OPT_DITHER_CHAIN = 1, 2, 4
LOSSY = 12


class Env:
    """What an op needs besides the handle: the package, and the tile the handle is set to (the oracle's results are kept per tile)."""

    def __init__(self, nq, tile=TILES[0]):
        self.nq, self.tile = nq, tile


class Op:
    """name; the exports of include/nquant_abi.h it calls; run(env, q, variant) -> (got, want); dithers: True when it ends with a pass of
    the error-diffusion dither on the handle (nq_get_dither_path speaks of it), False when it runs none, None when that is not stated."""

    def __init__(self, name, symbols, run, dithers=False):
        self.name, self.symbols, self.run, self.dithers = name, tuple(symbols), run, dithers


_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def new_handle(nq, kind, tile=TILES[0]):
    cls = nq.PnnLABQuantizer if kind else nq.PnnQuantizer
    return cls(np.zeros((1, 1), np.int32), mode=TILED, seed=0, tile=tile)


def _u(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.int32 else a


def compare(got, want, what):
    """got == want, key by key: bytes, ints and lists of them literally, arrays by shape and bits."""
    assert sorted(got) == sorted(want), "%s: results %s, expected %s" % (what, sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        if isinstance(w, (bytes, int)):
            assert g == w, "%s: %s differs%s" % (what, key, "" if isinstance(w, int) else " (%d bytes, expected %d)" % (len(g), len(w)))
        elif isinstance(w, list) and w and isinstance(w[0], bytes):
            bad = [i for i, (a, b) in enumerate(zip(g, w)) if a != b]
            assert len(g) == len(w) and not bad, "%s: %s differ in files %s" % (what, key, bad)
        elif isinstance(w, list) and w and isinstance(w[0], np.ndarray):
            assert len(g) == len(w), "%s: %s has %d arrays, expected %d" % (what, key, len(g), len(w))
            for i, (a, b) in enumerate(zip(g, w)):
                assert np.asarray(a).shape == b.shape, "%s: %s[%d] has shape %s, expected %s" % (what, key, i, np.asarray(a).shape, b.shape)
                bad = int((_u(a) != _u(b)).sum())
                assert bad == 0, "%s: %s[%d] differs in %d of %d elements" % (what, key, i, bad, b.size)
        elif isinstance(w, list):
            g = [tuple(int(v) for v in r) if isinstance(r, (tuple, list, np.ndarray)) else int(r) for r in (g.tolist() if isinstance(g, np.ndarray) else g)]
            w = [tuple(int(v) for v in r) if isinstance(r, (tuple, list, np.ndarray)) else int(r) for r in w]
            assert g == w, "%s: %s is %s, expected %s" % (what, key, g, w)
        else:
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape, "%s: %s has shape %s, expected %s" % (what, key, g.shape, w.shape)
            bad = int((_u(g) != _u(w)).sum())
            assert bad == 0, "%s: %s differs in %d of %d elements (guards included)" % (what, key, bad, w.size)


# ---------------------------------------------------------------------------------------------------------------------------------
# the frame and encoder cases of stream_gate.py, by (kind of call, variant)
# ---------------------------------------------------------------------------------------------------------------------------------
_FRAME_CASES = {}


def _family(case):
    name = case.name.split("-")[0]
    if name.startswith("orient"):
        return "orient_turn" if case.args["code"] >= 5 else "orient_flip"
    return name


def frame_cases():
    """{(family, variant): stream_gate.Case}."""
    if not _FRAME_CASES:
        for variant in VARIANTS:
            for c in G._frame_cases((SHAPE[variant],), FRAMES[variant]):
                assert (_family(c), variant) not in _FRAME_CASES
                _FRAME_CASES[(_family(c), variant)] = c
    return _FRAME_CASES


def frame_families():
    return sorted({f for f, _ in frame_cases()})


def _device_results(b, ref, host, inputs):
    """(got, want) of a device call: the whole output and in-place buffers against sentinel + reference, the host results, the inputs."""
    got, want = {}, {}
    for name, value in ref.items():
        if name.startswith(("out_", "io_")):
            buf = b[name]
            expect = buf.host.copy()
            buf.fill(expect, [np.ascontiguousarray(a).view(expect.dtype) for a in value])
            got[name], want[name] = buf.read(), expect
        else:
            got[name], want[name] = host[name], value
    for group in inputs:
        if not group.startswith("io_"):
            got["in:" + group], want["in:" + group] = b[group].read(), b[group].host
    return got, want


def _frame_device(family):
    def run(env, q, variant):
        import torch
        from test_gpu_streams import _call
        case = frame_cases()[(family, variant)]
        ref = G.want(case)
        b = {group: G.make_buffer(group, arrays, case.shift) for group, arrays in case.true.items()}
        for name, arrays in ref.items():
            if name.startswith("out_"):
                b[name] = G.make_output(name, arrays, case.shift)
        host = _call(env.nq, q, case, b)
        torch.cuda.synchronize()
        return _device_results(b, ref, host, case.true)
    return run


def _frame_host(family):
    """The host form of the same call on the same handle, on copies of the case's true inputs."""
    def run(env, q, variant):
        from nquant.android_amd import apng, gif, hold, ordered, orient, png, refine, resample, shots, yuv
        case = frame_cases()[(family, variant)]
        ref, a = G.want(case), case.args
        L, h, chk = q._L, q._h, q._check
        n = FRAMES[variant]
        w, hgt = a["w"], a["h"]
        ws, hs = np.full(n, w, np.int32), np.full(n, hgt, np.int32)
        frames = [np.ascontiguousarray(f).copy() for f in case.true.get("argb", [])]
        planes = [tuple(np.ascontiguousarray(p).copy() for p in f) for f in case.true.get("yuv", [])]
        maps = [np.ascontiguousarray(m).copy() for m in case.true.get("index", [])]
        got = {}
        if family == "hold_counts":
            io_index = [np.ascontiguousarray(m).copy() for m in case.true["io_index"]]
            io_argb = [np.ascontiguousarray(o).copy() for o in case.true["io_argb"]]
            got = {"held": hold._hold_host(L, h, chk, frames, io_index, io_argb, 4), "io_index": io_index, "io_argb": io_argb}
        elif family == "resample":
            got = {"out_argb": resample._resample_host(L, h, chk, frames, a["size"], a["crop"], True)}
        elif family == "resample_oriented":
            got = {"out_argb": resample._resample_host(L, h, chk, frames, a["size"], a["crop"], True, a["code"])}
        elif family in ("orient_turn", "orient_flip"):
            got = {"out_argb": orient._orient_host(L, h, chk, frames, a["code"])}
        elif family in ("yuv", "yuv_oriented", "resample_yuv", "resample_yuv_oriented"):
            got = {"out_argb": yuv._yuv_host(L, h, chk, planes, a.get("size"), a.get("crop"), True, yuv.YUV_BT709, a.get("code", 1))}
        elif family == "ordered_stats":
            idx, out = [np.empty(f.shape, np.uint16) for f in frames], [np.empty(f.shape, np.int32) for f in frames]
            stats = ordered._dither(L, h, chk, "nq_dither_ordered", [f.ctypes.data for f in frames], ws, hs, a["palette"], a["limit"],
                                    [i.ctypes.data for i in idx], [o.ctypes.data for o in out], True)
            got = {"out_index": idx, "out_argb": out, "stats": stats}
        elif family == "refine":
            pal, sse, counts, passes = refine._refine(L, h, chk, "nq_refine_palette", [f.ctypes.data for f in frames], ws, hs, a["palette"], 3)
            got = {"palette": pal, "sse": sse, "counts": counts, "passes": passes}
        elif family == "signatures":
            got = {"sig": shots._signatures(L, h, chk, "nq_frame_signatures", [f.ctypes.data for f in frames], w, hgt)}
        elif family == "detect_shots":
            starts, scores = shots._detect_host(L, h, chk, frames, 0, 1)
            got = {"starts": starts, "scores": scores}
        elif family == "gif":
            got = {"file": gif._encode(L, h, "nq_encode_gif", [m.ctypes.data for m in maps], ws, hs, a["palette"], a["delays"], 0, 0, chk)}
        elif family == "gif_delta":
            data, rects = gif._encode_delta(L, h, "nq_encode_gif_delta", [m.ctypes.data for m in maps], w, hgt, a["palette"], a["delays"], 0, 0, chk)
            got = {"file": data, "rects": rects}
        elif family == "png":
            got = {"files": png._encode(L, h, "nq_encode_png", [m.ctypes.data for m in maps], ws, hs, [a["palette"]] * n, 0, chk)}
        elif family == "apng":
            got = {"file": apng._encode(L, h, "nq_encode_apng", [m.ctypes.data for m in maps], w, hgt, a["palette"], a["delays"], 0, 0, chk)[0]}
        else:
            raise KeyError(family)
        want = {k: (list(v) if k.startswith(("out_", "io_")) else v) for k, v in ref.items()}
        # the caller's arrays are read, never written
        for group, mine in (("argb", frames), ("index", maps)):
            if mine:
                got["in:" + group], want["in:" + group] = mine, [np.asarray(x) for x in case.true[group]]
        if planes:
            got["in:yuv"], want["in:yuv"] = [p for f in planes for p in f], [np.asarray(p) for f in case.true["yuv"] for p in f]
        return got, want
    return run


_DEVICE_SYMBOLS = {
    "hold": ["nq_hold_frames_device"], "hold_counts": ["nq_hold_frames_device"], "resample": ["nq_resample_frames_device"],
    "yuv": ["nq_frames_from_yuv_device"], "resample_yuv": ["nq_resample_frames_yuv_device"], "orient_turn": ["nq_orient_frames_device"],
    "orient_flip": ["nq_orient_frames_device"], "yuv_oriented": ["nq_frames_from_yuv_oriented_device"],
    "resample_oriented": ["nq_resample_frames_oriented_device"], "resample_yuv_oriented": ["nq_resample_frames_yuv_oriented_device"],
    "ordered": ["nq_dither_ordered_device"], "ordered_stats": ["nq_dither_ordered_device"], "refine": ["nq_refine_palette_device"],
    "signatures": ["nq_frame_signatures_device"], "detect_shots": ["nq_detect_shots_device"], "gif": ["nq_encode_gif_device"],
    "gif_delta": ["nq_encode_gif_delta_device"], "png": ["nq_encode_png_device"], "apng": ["nq_encode_apng_device"],
}
_NO_HOST_FORM = ("hold", "ordered")          # (the host forms always fetch the counts / statistics: hold_counts, ordered_stats)


# ---------------------------------------------------------------------------------------------------------------------------------
# the lossy and the local-table GIF encoders (tests/gif_lossy_ref.py, tests/gif_local_ref.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _gif_inputs(variant):
    """(index maps with still regions, their K, the global palette, one palette per frame -- two shots --, delays)."""
    def make():
        import gif_lossy_ref
        w, h, shift = SHAPE[variant][:3]
        n = FRAMES[variant]
        K = SHAPE[variant][3] if len(SHAPE[variant]) > 3 else 256 if shift == 0 else 16
        maps = G.index_maps(w, h, n, K, 9100 + w, still=True)
        # a grey ramp (neighbours a few levels apart: the lossy chains find candidates) and a random palette for the second shot
        ramp = np.asarray(gif_lossy_ref.ramp_palette(K)).astype(np.uint32).view(np.int32)
        other = G.palette(K, 9200 + w)
        locals_ = [ramp if i < (n + 1) // 2 else other for i in range(n)]
        return maps, K, ramp, locals_, ([4, 0, 65535] * n)[:n]
    return cached(("gif inputs", variant), make)


def _gif_extra(which, device):
    """which: lossy, delta_lossy, local, local_delta; the device form reads the maps from a guarded device buffer."""
    def reference(variant):
        import gif_local_ref
        import gif_lossy_ref
        maps, K, pal, locals_, delays = _gif_inputs(variant)
        if which == "lossy":
            return {"file": gif_lossy_ref.encode(maps, pal, delays_cs=delays, loop=0, lossy=LOSSY)[0]}
        if which == "delta_lossy":
            import gif_delta_ref
            return {"file": gif_lossy_ref.encode_delta(maps, pal, delays_cs=delays, loop=0, lossy=LOSSY)[0], "rects": gif_delta_ref.rectangles(maps)}
        if which == "local":
            return {"file": gif_local_ref.encode(maps, locals_, delays_cs=delays, loop=0, lossy=LOSSY)[0]}
        return {"file": gif_local_ref.encode_delta(maps, locals_, delays_cs=delays, loop=0, lossy=0)[0],
                "rects": gif_local_ref.rectangles(maps, locals_)}

    def run(env, q, variant):
        from nquant.android_amd import gif
        maps, K, pal, locals_, delays = _gif_inputs(variant)
        want = dict(cached(("gif extra", which, variant), lambda: reference(variant)))
        w, h, shift = SHAPE[variant][:3]
        n = len(maps)
        ws, hs = np.full(n, w, np.int32), np.full(n, h, np.int32)
        L, hd, chk = q._L, q._h, q._check
        sfx = "_device" if device else ""
        if device:
            buf = G.make_buffer("index", maps, shift)
            ptrs = buf.ptrs
        else:
            mine = [m.copy() for m in maps]
            ptrs = [m.ctypes.data for m in mine]
        if which == "lossy":
            got = {"file": gif._encode(L, hd, "nq_encode_gif" + sfx, ptrs, ws, hs, pal, delays, 0, 0, chk, LOSSY)}
        elif which == "delta_lossy":
            data, rects = gif._encode_delta(L, hd, "nq_encode_gif_delta" + sfx, ptrs, w, h, pal, delays, 0, 0, chk, LOSSY)
            got = {"file": data, "rects": rects}
        elif which == "local":
            got = {"file": gif._encode_local(L, hd, "nq_encode_gif_local" + sfx, ptrs, ws, hs, locals_, delays, 0, 0, LOSSY, chk, False)[0]}
        else:
            data, rects = gif._encode_local(L, hd, "nq_encode_gif_local_delta" + sfx, ptrs, w, h, locals_, delays, 0, 0, 0, chk, True)
            got = {"file": data, "rects": rects}
        if device:
            got["in:index"], want["in:index"] = buf.read(), buf.host
        else:
            got["in:index"], want["in:index"] = mine, list(maps)
        return got, want
    return run


_GIF_EXTRA = {"lossy": "nq_encode_gif_lossy", "delta_lossy": "nq_encode_gif_delta_lossy", "local": "nq_encode_gif_local",
              "local_delta": "nq_encode_gif_local_delta"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the quantizer, on the kind of the handle it is given, against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _quant_image(variant, seed, colours):
    """The small variants: stream_gate.quant_image, thousands of histogram bins.  LARGE: as many pixels drawn from `colours` colours, so
    that the merge loop, which a call spends most of its time in, starts from about as many bins as at the small variants."""
    from nquant.android_amd import synth
    w, h = SHAPE[variant][:2]
    return synth.few_colors(w, h, seed, colours) if variant == "LARGE" else G.quant_image(w, h, seed)


def _image(variant, salt):
    return cached(("image", variant, salt), lambda: _quant_image(variant, 9300 + salt, 3000))


def _few_image(variant):
    """Fewer colours than nMaxColors: the early return of pnnquan (NQ/PnnLABQuantizer.java:193-206)."""
    from nquant.android_amd import synth
    w, h = SHAPE[variant][:2]
    return cached(("few", variant), lambda: synth.few_colors(w, h, 9400 + w, 40))


def _tile_of(env, img):
    h, w = img.shape
    return (min(env.tile[0], w), min(env.tile[1], h))


def _oracle_convert(kind, img, K, dither, seed, tile):
    """prescan + pnnquan + tiled dither (tile None: the oracle's own whole convert(), the REFERENCE_SEQUENTIAL result)."""
    import oracle_lib
    oq = oracle_lib.OracleQuantizer(kind, img, seed=seed)
    if tile is None:
        argb, idx, pal = oq.convert(K, dither)
    else:
        oq.prescan(K)
        pal = oq.pnnquan(K)
        oq.set_seed(seed)
        argb, idx = oq.dither(pal, dither, tile=tile)
    oq.close()
    return {"palette": np.asarray(pal, np.int32), "index": idx.astype(np.uint16), "argb": np.asarray(argb, np.int32)}


def _point(q, img):
    q.pixels, (q.height, q.width) = np.ascontiguousarray(img).reshape(-1), img.shape


def _want_convert(env, q, variant, K, dither, mode, salt):
    """(image, the oracle's convert of it): host and device forms of one configuration share image, seed and reference."""
    img = _few_image(variant) if salt == "few" else _image(variant, salt)
    tile = None if mode == SEQ else _tile_of(env, img)
    seed = 100 + K + int(dither)
    return img, seed, cached(("convert", q.KIND, K, dither, variant, tile, salt), lambda: _oracle_convert(q.KIND, img, K, dither, seed, tile))


def _convert_host(K, dither, mode, salt=1):
    def run(env, q, variant):
        img, seed, want = _want_convert(env, q, variant, K, dither, mode, salt)
        mine = img.copy()
        _point(q, mine)
        out = q.convert(K, dither, mode=mode, seed=seed)
        got = {"palette": out.palette, "index": out.index, "argb": out.argb, "in:argb": mine}
        return got, dict(want, **{"in:argb": img})
    return run


def _device_image(img, shift):
    src = G.make_buffer("argb", [img], shift)
    return src, G.make_output("out_argb", [img], shift), G.make_output("out_index", [img], shift)


def _device_want(want, src, out, idx):
    return {"palette": want["palette"], "out_argb": out.expect([want["argb"]]), "out_index": idx.expect([want["index"]]),
            "in:argb": src.host}


def _convert_device(K, dither, mode, chain):
    """nq_convert_device, or (chain) nq_pnnquan_device + nq_dither_device."""
    def run(env, q, variant):
        import torch
        img, seed, want = _want_convert(env, q, variant, K, dither, mode, 1)
        src, out, idx = _device_image(img, SHAPE[variant][2])
        _point(q, img)
        if chain:
            pal = q.pnnquan_device(src.ptrs[0], K)
            q.dither_device(src.ptrs[0], pal, dither, out.ptrs[0], idx.ptrs[0], mode=mode, seed=seed)
        else:
            pal = q.convert_device(src.ptrs[0], K, dither, out.ptrs[0], idx.ptrs[0], mode=mode, seed=seed)
        torch.cuda.synchronize()
        return {"palette": pal, "out_argb": out.read(), "out_index": idx.read(), "in:argb": src.read()}, _device_want(want, src, out, idx)
    return run


def _pnnquan_dither_host(K, dither):
    def run(env, q, variant):
        img, seed, want = _want_convert(env, q, variant, K, dither, TILED, 1)
        _point(q, img.copy())
        pal = q.pnnquan(K)
        argb, idx = q.dither(pal, dither, mode=TILED, seed=seed)
        return {"palette": pal, "index": idx, "argb": argb}, want
    return run


def _lookup(K):
    """nq_pnnquan + nq_dither in MODE_LOOKUP_ONLY: every pixel's nearestColorIndex (tests/test_gpu_parity.py: lookup_only)."""
    def reference(kind, img):
        import oracle_lib
        oq = oracle_lib.OracleQuantizer(kind, img)
        oq.prescan(K)
        pal = oq.pnnquan(K)
        idx = np.asarray(oq.nearest_index(pal, img.reshape(-1))).reshape(img.shape)
        cols = G.argb_frames(64, 33, 1, 9500 + K)[0].reshape(-1)
        r = {"palette": np.asarray(pal, np.int32), "index": idx.astype(np.uint16), "argb": np.asarray(pal, np.int32)[idx],
             "nearest": np.asarray(oq.nearest_index(pal, cols)), "closest": np.asarray(oq.closest_tuple(pal, cols))}
        oq.close()
        return r, cols

    def run(env, q, variant):
        img = _image(variant, 4)
        want, cols = cached(("lookup", q.KIND, K, variant), lambda: reference(q.KIND, img))
        _point(q, img.copy())
        pal = q.pnnquan(K)
        argb, idx = q.dither(pal, False, mode=LOOKUP)
        return {"palette": pal, "index": idx, "argb": argb, "nearest": q.nearestColorIndex(pal, cols), "closest": q.closestTuple(pal, cols)}, want
    return run


def _frames_images(variant, salt):
    return cached(("frames images", variant, salt), lambda: [_quant_image(variant, 9600 + 10 * salt + i, 800) for i in range(FRAMES[variant])])


def _frames_reference(kind, frames, K, seeds, refine, ordered_limit, tile):
    import ordered_ref
    import refine_ref
    pal, shared = G.oracle_sequence(kind, frames, K)
    if refine:
        pal = refine_ref.refine(frames, pal, refine)[0].view(np.int32)
    if ordered_limit is not None:
        idx, out, _ = ordered_ref.dither(frames, pal, ordered_limit)
        return {"palette": np.asarray(pal, np.int32), "index": [np.asarray(i, np.uint16) for i in idx], "argb": [o.view(np.int32) for o in out]}
    import oracle_lib
    idx, out = [], []
    for f, s in zip(frames, seeds):
        oq = oracle_lib.OracleQuantizer(kind, f, seed=s)
        oq.prescan(K)
        oq.set_params(shared)
        oq.set_seed(s)
        a, i = oq.dither(np.asarray(pal).view(np.int32), True, tile=tile)
        oq.close()
        idx.append(i.astype(np.uint16))
        out.append(a)
    return {"palette": np.asarray(pal, np.int32), "index": idx, "argb": out}


def _convert_frames(K, form, device):
    """form: plain, refined (2 passes) or ordered (limit 16); nq_convert_frames[_refined|_ordered][_device]."""
    refine, limit = (2 if form == "refined" else 0), (16 if form == "ordered" else None)
    salt = {"plain": 1, "refined": 2, "ordered": 3}[form]

    def run(env, q, variant):
        frames = _frames_images(variant, salt)
        n = len(frames)
        seeds = [61 + i for i in range(n)]
        tile = _tile_of(env, frames[0])
        want = cached(("frames", q.KIND, K, form, variant, tile if limit is None else None),
                      lambda: _frames_reference(q.KIND, frames, K, seeds, refine, limit, tile))
        h, w = frames[0].shape
        ws, hs = np.full(n, w, np.int32), np.full(n, h, np.int32)
        pal, got_K = np.zeros(max(K, 2), np.int32), C.c_int32(0)
        sd = np.array(seeds, np.int64)
        arr = lambda ptrs: (C.c_void_p * n)(*[int(p) for p in ptrs])
        if device:
            import torch
            shift = SHAPE[variant][2]
            src, out, idx = G.make_buffer("argb", frames, shift), G.make_output("out_argb", frames, shift), G.make_output("out_index", frames, shift)
            ptrs = (arr(src.ptrs), arr(out.ptrs), arr(idx.ptrs))
        else:
            mine = [f.copy() for f in frames]
            outs, idxs = [np.empty(f.shape, np.int32) for f in frames], [np.empty(f.shape, np.uint16) for f in frames]
            ptrs = (arr([f.ctypes.data for f in mine]), arr([o.ctypes.data for o in outs]), arr([i.ctypes.data for i in idxs]))
        sfx = "_device" if device else ""
        head = (q._h, n, ptrs[0], ws.ctypes.data, hs.ctypes.data, K)
        tail = (ptrs[1], ptrs[2], pal.ctypes.data, C.byref(got_K))
        if form == "plain":
            q._check(getattr(q._L, "nq_convert_frames" + sfx)(*head, 1, sd.ctypes.data, TILED, *tail))
        elif form == "refined":
            q._check(getattr(q._L, "nq_convert_frames_refined" + sfx)(*head, refine, 1, sd.ctypes.data, TILED, *tail))
        else:
            q._check(getattr(q._L, "nq_convert_frames_ordered" + sfx)(*head, 0, limit, *tail))
        palette = pal[:got_K.value].copy()
        if device:
            torch.cuda.synchronize()
            return ({"palette": palette, "out_argb": out.read(), "out_index": idx.read(), "in:argb": src.read()},
                    {"palette": want["palette"], "out_argb": out.expect(want["argb"]), "out_index": idx.expect(want["index"]), "in:argb": src.host})
        return {"palette": palette, "argb": outs, "index": idxs, "in:argb": mine}, dict(want, **{"in:argb": list(frames)})
    return run


def _pnnquan_frames(K):
    """nq_pnnquan_frames_device, then nq_dither_device per frame with the palette and the params it left in the handle ("palettegen /
    paletteuse"): the results of nq_convert_frames_device on the same frames."""
    def run(env, q, variant):
        import torch
        frames = _frames_images(variant, 1)
        n = len(frames)
        seeds = [61 + i for i in range(n)]
        tile = _tile_of(env, frames[0])
        want = cached(("frames", q.KIND, K, "plain", variant, tile), lambda: _frames_reference(q.KIND, frames, K, seeds, 0, None, tile))
        h, w = frames[0].shape
        shift = SHAPE[variant][2]
        src, out, idx = G.make_buffer("argb", frames, shift), G.make_output("out_argb", frames, shift), G.make_output("out_index", frames, shift)
        pal = env.nq.pnnquan_frames_device(q, src.ptrs, [w] * n, [h] * n, K)
        q.width, q.height = w, h
        for i in range(n):
            q.dither_device(src.ptrs[i], pal, True, out.ptrs[i], idx.ptrs[i], mode=TILED, seed=seeds[i])
        torch.cuda.synchronize()
        return ({"palette": pal, "out_argb": out.read(), "out_index": idx.read(), "in:argb": src.read()},
                {"palette": want["palette"], "out_argb": out.expect(want["argb"]), "out_index": idx.expect(want["index"]), "in:argb": src.host})
    return run


def _batch(K, position, host=False):
    """nq_convert_batch_device (host: nq_convert_batch on host arrays) of three images of mixed kinds, the handle under test first or
    last; the other two handles live for the call only."""
    def run(env, q, variant):
        import torch
        kinds = [q.KIND, 1 - q.KIND, q.KIND]
        imgs = [_image(variant, 5), _image("WIDE" if variant != "WIDE" else "NARROW", 6), _image("NARROW" if variant == "LARGE" else "LARGE", 7)]
        seeds = [71, 72, 73]
        if position == "last":
            kinds, imgs, seeds = kinds[::-1], imgs[::-1], seeds[::-1]
        wants = [cached(("batch", k, K, im.shape, s, _tile_of(env, im)), lambda k=k, im=im, s=s: _oracle_convert(k, im, K, True, s, _tile_of(env, im)))
                 for k, im, s in zip(kinds, imgs, seeds)]
        others = [new_handle(env.nq, k, env.tile) for k in (kinds[1:] if position == "first" else kinds[:-1])]
        qs = [q] + others if position == "first" else others + [q]
        try:
            for quantizer, im in zip(qs, imgs):
                _point(quantizer, im)
            if host:
                mine = [im.copy() for im in imgs]
                outs, idxs = [np.empty(im.shape, np.int32) for im in imgs], [np.empty(im.shape, np.uint16) for im in imgs]
                pals = env.nq.convert_batch_host(qs, [m.ctypes.data for m in mine], K, True, [o.ctypes.data for o in outs],
                                                 [i.ctypes.data for i in idxs], mode=TILED, seeds=seeds)
                got, want = {}, {}
                for i, w in enumerate(wants):
                    for k, g in (("palette", pals[i]), ("argb", outs[i]), ("index", idxs[i])):
                        got["%d:%s" % (i, k)], want["%d:%s" % (i, k)] = g, w[k]
                    got["%d:in" % i], want["%d:in" % i] = mine[i], imgs[i]
                return got, want
            bufs = [_device_image(im, i % 2) for i, im in enumerate(imgs)]
            pals = env.nq.convert_batch_device(qs, [b[0].ptrs[0] for b in bufs], K, True, [b[1].ptrs[0] for b in bufs], [b[2].ptrs[0] for b in bufs],
                                               mode=TILED, seeds=seeds)
            torch.cuda.synchronize()
        finally:
            for o in others:
                o.close()
        got, want = {}, {}
        for i, ((src, out, idx), w) in enumerate(zip(bufs, wants)):
            g = {"palette": pals[i], "out_argb": out.read(), "out_index": idx.read(), "in:argb": src.read()}
            for k, v in _device_want(w, src, out, idx).items():
                got["%d:%s" % (i, k)], want["%d:%s" % (i, k)] = g[k], v
        return got, want
    return run


def _convert_lookup(K, dither, device):
    """nq_convert[_device] in MODE_LOOKUP_ONLY: the palette of pnnquan, then every pixel's nearestColorIndex -- no diffusion, whatever
    `dither` says (include/nquant_abi.h: nq_mode)."""
    def reference(kind, img):
        import oracle_lib
        oq = oracle_lib.OracleQuantizer(kind, img)
        oq.prescan(K)
        pal = np.asarray(oq.pnnquan(K), np.int32)
        idx = np.asarray(oq.nearest_index(pal, img.reshape(-1))).reshape(img.shape)
        oq.close()
        return {"palette": pal, "index": idx.astype(np.uint16), "argb": pal[idx]}

    def run(env, q, variant):
        img = _image(variant, 4)
        want = cached(("convert lookup", q.KIND, K, variant), lambda: reference(q.KIND, img))
        if device:
            import torch
            src, out, idx = _device_image(img, SHAPE[variant][2])
            _point(q, img)
            pal = q.convert_device(src.ptrs[0], K, dither, out.ptrs[0], idx.ptrs[0], mode=LOOKUP, seed=7)
            torch.cuda.synchronize()
            return {"palette": pal, "out_argb": out.read(), "out_index": idx.read(), "in:argb": src.read()}, _device_want(want, src, out, idx)
        mine = img.copy()
        _point(q, mine)
        o = q.convert(K, dither, mode=LOOKUP, seed=7)
        return {"palette": o.palette, "index": o.index, "argb": o.argb, "in:argb": mine}, dict(want, **{"in:argb": img})
    return run


def _saliencies(shape, seed):
    from nquant.android_amd import synth
    z = synth.splitmix64(seed, shape[0] * shape[1])
    return (0.1 + 0.9 * (z & np.uint64(0xFFFF)).astype(np.float64) / 65535.0).astype(np.float32).reshape(shape)


def _staged(K):
    """The static ditherers (tests/test_gpu_boundary.py): nq_set_params with the scalars of the image, nq_gilbert_dither with the CALLER'S
    saliencies and dither off -- palette indices out --, then nq_bluenoise_dither over them."""
    weight, blue, seed = 0.0115, 0.95, 99

    def reference(kind, img, tile):
        import oracle_lib
        oq = oracle_lib.OracleQuantizer(kind, img, seed=seed)
        oq.prescan(K)
        pal = np.asarray(oq.pnnquan(K), np.int32)
        params = oq.params
        oq.set_seed(seed)
        qpix, idx = oq.gilbert_dither_stage(pal, _saliencies(img.shape, 1000 + K), weight, False, tile=tile)
        argb, idx2 = oq.bluenoise_dither_stage(pal, qpix, blue, True)
        oq.close()
        return {"qpixels": qpix, "index": idx.astype(np.uint16), "argb": argb, "index2": idx2.astype(np.uint16)}, pal, params

    def run(env, q, variant):
        img = _image(variant, 11)
        tile = _tile_of(env, img)
        want, pal, oparams = cached(("staged", q.KIND, K, variant, tile), lambda: reference(q.KIND, img, tile))
        p = env.nq.Params()
        for f, _ in env.nq.Params._fields_:
            setattr(p, f, getattr(oparams, f))
        q.set_params(p)
        _point(q, img.copy())
        qpix, idx = q.gilbert_dither(pal, _saliencies(img.shape, 1000 + K), weight, False, mode=TILED, seed=seed)
        argb, idx2 = q.bluenoise_dither(pal, qpix, blue, mode=TILED, seed=seed)
        return {"qpixels": qpix, "index": idx, "argb": argb, "index2": idx2}, want
    return run


def split_start(variant):
    """The first row of the second band: a multiple of both tile heights of TILES."""
    return 16 if SHAPE[variant][1] < 64 else 96


def _split(K, dither, position):
    """One round of the split pipeline over two bands (tests/test_gpu_banded.py: _bands_by_hand), the handle under test as the first or as
    the last band and a handle of the same kind, open for the round only, as the other: nq_band_scan_device, nq_set_scan,
    nq_band_histogram_device, (LAB, few colours: nq_band_distinct_device, nq_set_distinct,) nq_palette_from_histograms_device, (LAB, dither
    off: nq_band_color_presence_device,) nq_set_band + nq_dither_device, and back to nq_set_band(0, 0).  At NARROW the image has fewer
    colours than nMaxColors: the early return across bands."""
    seed = 77

    def reference(kind, img, starts, tile):
        import oracle_lib
        oq = oracle_lib.OracleQuantizer(kind, img, seed=seed)
        oq.set_bands(starts)
        oq.prescan(K)
        pal = oq.pnnquan(K)
        argb, idx = oq.dither(pal, dither, tile=tile)
        oq.close()
        return {"palette": np.asarray(pal, np.int32), "index": idx.astype(np.uint16), "argb": argb}

    def run(env, q, variant):
        from test_gpu_banded import _bands_by_hand
        img = _few_image(variant) if variant == "NARROW" else _image(variant, 10)
        starts, tile = [0, split_start(variant)], _tile_of(env, img)
        want = cached(("split", q.KIND, K, dither, variant, tile), lambda: reference(q.KIND, img, starts, tile))
        other = new_handle(env.nq, q.KIND, env.tile)
        saved = (q.mode, q.seed)
        try:
            pal, argb, idx, _ = _bands_by_hand(env.nq, img, q.KIND, K, dither, starts, seed, env.tile, [q, other] if position == "first" else [other, q])
        finally:
            q.set_band(0, 0)
            q.mode, q.seed = saved
            other.close()
        return {"palette": pal, "index": idx, "argb": argb}, want
    return run


_SPLIT_SYMBOLS = ["nq_band_scan_device", "nq_set_scan", "nq_band_histogram_device", "nq_band_distinct_device", "nq_set_distinct",
                  "nq_palette_from_histograms_device", "nq_band_color_presence_device", "nq_dither_device"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
def _build():
    ops = []
    for family, symbols in sorted(_DEVICE_SYMBOLS.items()):
        ops.append(Op(family + "_device", symbols, _frame_device(family)))
        if family not in _NO_HOST_FORM:
            ops.append(Op(family + "_host", [s[:-len("_device")] for s in symbols], _frame_host(family)))
    for which, symbol in sorted(_GIF_EXTRA.items()):
        ops.append(Op("gif_%s_device" % which, [symbol + "_device"], _gif_extra(which, True)))
        ops.append(Op("gif_%s_host" % which, [symbol], _gif_extra(which, False)))
    ops += [
        Op("convert_tiled_dither_host", ["nq_convert"], _convert_host(256, True, TILED), True),
        Op("convert_tiled_plain_host", ["nq_convert"], _convert_host(256, False, TILED), True),
        Op("convert_tiled_16_host", ["nq_convert"], _convert_host(16, True, TILED), True),
        Op("convert_sequential_dither_host", ["nq_convert"], _convert_host(256, True, SEQ), True),
        Op("convert_sequential_64_host", ["nq_convert"], _convert_host(64, True, SEQ), True),
        Op("convert_sequential_plain_host", ["nq_convert"], _convert_host(64, False, SEQ), True),
        Op("convert_sequential_plain_device", ["nq_convert_device"], _convert_device(64, False, SEQ, False), True),
        Op("convert_lookup_dither_host", ["nq_convert"], _convert_lookup(256, True, False), None),
        Op("convert_lookup_plain_host", ["nq_convert"], _convert_lookup(256, False, False), None),
        Op("convert_lookup_dither_device", ["nq_convert_device"], _convert_lookup(256, True, True), None),
        Op("convert_lookup_plain_device", ["nq_convert_device"], _convert_lookup(256, False, True), None),
        Op("gilbert_saliencies_bluenoise_host", ["nq_gilbert_dither", "nq_bluenoise_dither"], _staged(256), None),
        Op("split_first_device", _SPLIT_SYMBOLS, _split(256, True, "first"), True),
        Op("split_last_device", _SPLIT_SYMBOLS, _split(256, False, "last"), True),
        Op("convert_few_colours_host", ["nq_convert"], _convert_host(256, True, TILED, salt="few"), True),
        Op("convert_two_colours_host", ["nq_convert"], _convert_host(2, True, SEQ), None),
        Op("convert_tiled_dither_device", ["nq_convert_device"], _convert_device(256, True, TILED, False), True),
        Op("convert_tiled_plain_device", ["nq_convert_device"], _convert_device(256, False, TILED, False), True),
        Op("convert_sequential_64_device", ["nq_convert_device"], _convert_device(64, True, SEQ, False), True),
        Op("pnnquan_dither_device", ["nq_pnnquan_device", "nq_dither_device"], _convert_device(16, True, TILED, True), True),
        Op("pnnquan_dither_host", ["nq_pnnquan", "nq_dither"], _pnnquan_dither_host(16, True), True),
        Op("lookup_nearest_closest_host", ["nq_pnnquan", "nq_dither", "nq_nearest_index", "nq_closest_tuple"], _lookup(256), None),
        Op("convert_frames_device", ["nq_convert_frames_device"], _convert_frames(256, "plain", True), True),
        Op("convert_frames_host", ["nq_convert_frames"], _convert_frames(256, "plain", False), True),
        Op("convert_frames_refined_device", ["nq_convert_frames_refined_device"], _convert_frames(16, "refined", True), True),
        Op("convert_frames_refined_host", ["nq_convert_frames_refined"], _convert_frames(16, "refined", False), True),
        Op("convert_frames_ordered_device", ["nq_convert_frames_ordered_device"], _convert_frames(256, "ordered", True), None),
        Op("convert_frames_ordered_host", ["nq_convert_frames_ordered"], _convert_frames(256, "ordered", False), None),
        Op("batch_first_device", ["nq_convert_batch_device"], _batch(256, "first"), None),
        Op("batch_last_device", ["nq_convert_batch_device"], _batch(256, "last"), None),
        Op("batch_first_host", ["nq_convert_batch"], _batch(256, "first", True), None),
        Op("pnnquan_frames_dither_device", ["nq_pnnquan_frames_device", "nq_dither_device"], _pnnquan_frames(256), True),
    ]
    table = {}
    for op in ops:
        assert op.name not in table
        table[op.name] = op
    return table


OPS = _build()
NAMES = sorted(OPS)


# ---------------------------------------------------------------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------------------------------------------------------------
def centre_schedule(centre):
    """Part A: A, B1, A, B2, ... over every other op: [(op name, variant)].  The variants alternate so that both a LARGE centre before a
    small neighbour and a small centre before a LARGE neighbour occur -- and, with them, a LARGE neighbour before a LARGE centre and a
    small one before a small one."""
    steps = []
    for i, other in enumerate(n for n in NAMES if n != centre):
        small = SMALL[(i // 2) % 2]
        if i % 2 == 0:
            steps += [(centre, "LARGE"), (other, small)]
        else:
            steps += [(centre, small), (other, "LARGE")]
    steps.append((centre, "NARROW"))
    return steps


SETTERS = ("option", "tile", "stream", "params")


def walk(seed, steps=150):
    """Part B: [("op", name, variant) | ("option", which, value) | ("tile", tile) | ("stream", 0 | 1 | None) | ("params",)], the same for
    the same seed."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        if rng.random() < 0.25:
            what = SETTERS[int(rng.integers(len(SETTERS)))]
            if what == "option":
                out.append(("option", (OPT_CELL_LISTS, OPT_FAST_DITHER, OPT_DITHER_CHAIN)[int(rng.integers(3))], int(rng.integers(2))))
            elif what == "tile":
                out.append(("tile", TILES[int(rng.integers(2))]))
            elif what == "stream":
                out.append(("stream", (0, 1, None)[int(rng.integers(3))]))
            else:
                out.append(("params",))
        else:
            out.append(("op", NAMES[int(rng.integers(len(NAMES)))], VARIANTS[int(rng.integers(3))]))
    return out


class Walker:
    """Runs the steps of walk() on one handle; the streams are made on first use."""

    def __init__(self, env, q):
        self.env, self.q, self.streams, self.current = env, q, None, None

    def step(self, s, what):
        import torch
        q = self.q
        if s[0] == "op":
            got, want = OPS[s[1]].run(self.env, q, s[2])
            compare(got, want, what)
        elif s[0] == "option":
            q.set_option(s[1], s[2])
        elif s[0] == "tile":
            q.set_tile(*s[1])
            self.env.tile = s[1]
        elif s[0] == "stream":
            if self.streams is None:
                self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            torch.cuda.synchronize()                  # (the header's precondition: the handle's earlier work has completed)
            self.current = None if s[1] is None else self.streams[s[1]]
            q.set_stream(None if self.current is None else self.current.cuda_stream)
        else:
            p = q.params
            q.set_params(p)

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.q.set_stream(None)
