"""One handle, every entry point after every other (include/nquant_abi.h: "a handle mirrors ONE reference quantizer object"; it lives as
long as the Java object behind it).  The handle's grow-only buffers, partly rewritten tables, caches with validity flags and sticky
setters are shared by the quantizer, the frame calls and the file encoders; every stale-state bug this project has recorded belongs
here.  The ops, their size variants and their references are in lifecycle_ops.py (tests/test_lifecycle_cpu.py checks the table and
the schedules without a GPU).

  A  every op as the centre of the schedule A, B1, A, B2, ... over all other ops, on a fresh handle per test, LARGE before small and
     small before LARGE in both directions; every call's results are checked; nq_get_dither_path asked after unrelated ops
  B  seeded walks of 150 steps with nq_set_option / nq_set_tile / nq_set_stream / nq_set_params in between, one handle per kind
  C  after a call that was rejected or failed (the statuses the header documents, nothing that could fault): every op at NARROW and
     at LARGE
  D  what a handle holds (nq_get_device_bytes): a repeated walk allocates nothing, small calls after LARGE ones allocate nothing but
     curve tables of new tile shapes, REFERENCE_SEQUENTIAL keeps one whole-image curve table and not one per image size, and
     nq_destroy gives everything back

At most one handle of the test's own is alive at a time (the batch ops open two more for the length of their call).  Nothing here can
fault: every rejected call is one the header documents, with valid memory behind every pointer."""
import ctypes as C

import numpy as np
import pytest

import lifecycle_ops as O
import stream_gate as G

pytestmark = pytest.mark.gpu

KIND_NAME = {0: "rgb", 1: "lab"}
QUANTIZER_OPS = [n for n in O.NAMES if O.OPS[n].dithers is not False]           # (ops whose work depends on the handle's kind)
CENTRES = [(n, 1) for n in O.NAMES] + [(n, 0) for n in QUANTIZER_OPS]


def _told(centre, step, history):
    return "centre %s, step %d, last ops %s" % (centre, step, " > ".join("%s@%s" % h for h in history[-8:]))


class _Run:
    """Runs ops on one handle, checks every result, and keeps what nq_get_dither_path said straight after the last dither pass: asked
    again after ops that run no dither pass it has to say the same (the hand-back count is read lazily)."""

    def __init__(self, nq, kind, centre="-"):
        self.env = O.Env(nq)
        self.q = O.new_handle(nq, kind)
        self.centre, self.history, self.path = centre, [], None

    def op(self, name, variant):
        self.history.append((name, variant))
        what = _told(self.centre, len(self.history) - 1, self.history)
        got, want = O.OPS[name].run(self.env, self.q, variant)
        O.compare(got, want, what)
        dithers = O.OPS[name].dithers
        if dithers:
            self.path = self.q.dither_path()
        elif dithers is None:
            self.path = None
        elif self.path is not None:
            assert self.q.dither_path() == self.path, "%s: nq_get_dither_path changed without a dither pass" % what

    def close(self):
        self.q.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# A. every op between all others
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre,kind", CENTRES, ids=["%s-%s" % (n, KIND_NAME[k]) for n, k in CENTRES])
def test_every_op_between_all_others(nq, oracle, centre, kind):
    run = _Run(nq, kind, centre)
    try:
        for name, variant in O.centre_schedule(centre):
            run.op(name, variant)
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# B. seeded walks with the setters in between
# ---------------------------------------------------------------------------------------------------------------------------------
WALK_SEEDS = (11, 12, 13, 14)
WALK_STEPS = 150


def run_walk(nq, kind, seed, steps=WALK_STEPS, q=None, report=None):
    """The walk of `seed` on a handle of `kind` (q: an open one, else a fresh one that is closed again).  report(i, step) is called
    before every step (tests/lifecycle_replay.py)."""
    own = q is None
    q = O.new_handle(nq, kind) if own else q
    walker = O.Walker(O.Env(nq), q)
    history = []
    try:
        if not own:
            q.set_tile(*O.TILES[0])
        for i, s in enumerate(O.walk(seed, steps)):
            history.append((s[0] if s[0] != "op" else s[1], s[-1] if s[0] == "op" else s[1:]))
            if report:
                report(i, s)
            walker.step(s, "walk %d on %s, step %d, last steps %s" % (seed, KIND_NAME[kind], i, " > ".join("%s@%s" % h for h in history[-8:])))
    finally:
        walker.close()
        # (the sticky setters back to their defaults, for a handle that goes on)
        q.set_option(O.OPT_CELL_LISTS, 1), q.set_option(O.OPT_FAST_DITHER, 1), q.set_option(O.OPT_DITHER_CHAIN, 0)
        if own:
            q.close()


@pytest.mark.parametrize("kind", [1, 0], ids=["lab", "rgb"])
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_seeded_walk_with_setters(nq, oracle, seed, kind):
    run_walk(nq, kind, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. after a call that failed or was rejected
# ---------------------------------------------------------------------------------------------------------------------------------
def _status(q, rc, status, text=None):
    assert rc == status, "status %d, expected %d (%s)" % (rc, status, (q._L.nq_last_error(q._h) or b"").decode())
    if text:
        assert text in (q._L.nq_last_error(q._h) or b"").decode()


def _large_maps():
    """(index maps, K, global palette, palette per frame, delays) of the LARGE encoder ops."""
    return O._gif_inputs("LARGE")


def _fail_bad_index(entry):
    """An index >= K in the last frame of the LARGE maps (K = 16 here, so that 16 is one): found on the device, NQ_ERR_INVALID."""
    def fail(nq, q):
        from nquant.android_amd import apng, gif, png
        w, h = O.SHAPE["LARGE"][:2]
        maps = [(m % 16).astype(np.uint16) for m in _large_maps()[0]]
        maps[-1][h - 2, w - 3] = 16
        pal = G.palette(16, 1)
        n = len(maps)
        ws, hs = np.full(n, w, np.int32), np.full(n, h, np.int32)
        ptrs = [m.ctypes.data for m in maps]
        with pytest.raises(nq.NqError) as ei:
            if entry == "nq_encode_gif":
                gif._encode(q._L, q._h, entry, ptrs, ws, hs, pal, None, 0, 0, q._check)
            elif entry == "nq_encode_gif_delta_lossy":             # (gif._entry maps the base name to the _lossy export when lossy != 0)
                gif._encode_delta(q._L, q._h, "nq_encode_gif_delta", ptrs, w, h, pal, None, 0, 0, q._check, 9)
            elif entry == "nq_encode_gif_local":
                gif._encode_local(q._L, q._h, entry, ptrs, ws, hs, [pal] * n, None, 0, 0, 0, q._check, False)
            elif entry == "nq_encode_png":
                png._encode(q._L, q._h, entry, ptrs, ws, hs, [pal] * n, 0, q._check)
            else:
                apng._encode(q._L, q._h, entry, ptrs, w, h, pal, None, 0, 0, q._check)
        assert ei.value.status == -1 and "index" in str(ei.value)
    return fail


def _fail_short_capacity(kind):
    """The output one byte short: NQ_ERR_INVALID, the needed size reported, nothing written."""
    def fail(nq, q):
        case = O.frame_cases()[(kind, "LARGE")]
        want = G.want(case)
        maps = [np.ascontiguousarray(m) for m in case.true["index"]]
        n, (h, w) = len(maps), maps[0].shape
        ws, hs = np.full(n, w, np.int32), np.full(n, h, np.int32)
        src = (C.c_void_p * n)(*[m.ctypes.data for m in maps])
        pal = np.ascontiguousarray(case.args["palette"], np.int32)
        if kind == "gif":
            need = len(want["file"])
            out, size = np.full(need - 1, 0xAB, np.uint8), C.c_int64(-7)
            rc = q._L.nq_encode_gif(q._h, n, src, ws.ctypes.data, hs.ctypes.data, pal.ctypes.data, pal.size, None, 0, 0, out.ctypes.data, need - 1,
                                    C.byref(size))
            _status(q, rc, -1)
            assert size.value == need and (out == 0xAB).all()
        else:
            need = sum(len(f) for f in want["files"])
            table, Ks = np.ascontiguousarray(np.stack([pal] * n)), np.full(n, pal.size, np.int32)
            out, offs = np.full(need - 1, 0xAB, np.uint8), np.zeros(n + 1, np.int64)
            rc = q._L.nq_encode_png(q._h, n, src, ws.ctypes.data, hs.ctypes.data, table.ctypes.data, pal.size, Ks.ctypes.data, 0, out.ctypes.data,
                                    need - 1, offs.ctypes.data)
            _status(q, rc, -1)
            assert (out == 0xAB).all()
    return fail


def _fail_invalid(which):
    def fail(nq, q):
        L = q._L
        img = O._image("LARGE", 1).copy()
        h, w = img.shape
        out, idx, pal, K = np.zeros(img.size, np.int32), np.zeros(img.size, np.uint16), np.zeros(256, np.int32), C.c_int32(0)
        if which == "convert":                          # (width 0)
            rc = L.nq_convert(q._h, img.ctypes.data, 0, h, 256, 1, 1, O.TILED, out.ctypes.data, idx.ctypes.data, pal.ctypes.data, C.byref(K))
        elif which == "orient":                         # (orientation code 9)
            src, dst = (C.c_void_p * 1)(img.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
            rc = L.nq_orient_frames(q._h, 1, src, w, h, 9, dst)
        elif which == "lossy":                          # (threshold 256)
            maps = _large_maps()[0]
            n = len(maps)
            src = (C.c_void_p * n)(*[m.ctypes.data for m in maps])
            ws, hs = np.full(n, w, np.int32), np.full(n, h, np.int32)
            p = np.ascontiguousarray(_large_maps()[2], np.int32)
            buf, size = np.zeros(16, np.uint8), C.c_int64(0)
            rc = L.nq_encode_gif_lossy(q._h, n, src, ws.ctypes.data, hs.ctypes.data, p.ctypes.data, p.size, None, 0, 0, 256, buf.ctypes.data, 16, C.byref(size))
        elif which == "frames":                         # (a frame of height 0 behind a LARGE one)
            frames = O._frames_images("LARGE", 1)[:2]
            src = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
            dst, di = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data), (C.c_void_p * 2)(idx.ctypes.data, idx.ctypes.data)
            ws, hs, sd = np.array([w, w], np.int32), np.array([h, 0], np.int32), np.zeros(2, np.int64)
            rc = L.nq_convert_frames(q._h, 2, src, ws.ctypes.data, hs.ctypes.data, 256, 1, sd.ctypes.data, O.TILED, dst, di, pal.ctypes.data, C.byref(K))
        else:
            raise KeyError(which)
        _status(q, rc, -1)
    return fail


def _fail_band(nq, q):
    """A rejected nq_set_band; then an accepted band that the next dither does not fit (NQ_ERR_INVALID), and back to (0, 0)."""
    L = q._L
    _status(q, L.nq_set_band(q._h, 64, 64), -1, "nq_set_band")
    img = O._image("WIDE", 1).copy()
    h, w = img.shape
    _status(q, L.nq_set_band(q._h, 16, 32), 0)            # a band from row 16 of an image of 32 rows; the 40 rows dithered next end at row 56
    out, idx, pal = np.zeros(img.size, np.int32), np.zeros(img.size, np.uint16), G.palette(16, 3)
    rc = L.nq_dither(q._h, img.ctypes.data, w, h, pal.ctypes.data, 16, 1, 1, O.TILED, out.ctypes.data, idx.ctypes.data)
    _status(q, rc, -1, "nq_set_band")
    _status(q, L.nq_set_band(q._h, 0, 0), 0)


def _fail_batch(nq, q):
    """A batch of three with the handle under test first and the second image of height 0: NQ_ERR_INVALID."""
    import torch
    imgs = [O._image("LARGE", 5), O._image("WIDE", 6), O._image("NARROW", 7)]
    others = [O.new_handle(nq, 1 - q.KIND), O.new_handle(nq, q.KIND)]
    try:
        bufs = [O._device_image(im, 0) for im in imgs]
        for quantizer, im in zip([q] + others, imgs):
            O._point(quantizer, im)
        others[0].height = 0
        with pytest.raises(nq.NqError) as ei:
            nq.convert_batch_device([q] + others, [b[0].ptrs[0] for b in bufs], 256, True, [b[1].ptrs[0] for b in bufs], [b[2].ptrs[0] for b in bufs],
                                    mode=O.TILED, seeds=[1, 2, 3])
        torch.cuda.synchronize()
        assert ei.value.status == -1 and "bad argument" in str(ei.value)
    finally:
        for o in others:
            o.close()


def _arr(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[int(p) for p in ptrs])


def _fail_rejected(which):
    """One documented rejection per family, host forms, valid memory behind every pointer: NQ_ERR_INVALID."""
    def fail(nq, q):
        L, h = q._L, q._h
        W, H, n = 8, 6, 2
        frames = G.argb_frames(W, H, n, 5)
        outs = [np.zeros((H, W), np.int32) for _ in range(n)]
        maps = [np.zeros((H, W), np.uint16) for _ in range(n)]
        ws, hs = np.full(n, W, np.int32), np.full(n, H, np.int32)
        src, dst, idx = _arr([f.ctypes.data for f in frames]), _arr([o.ctypes.data for o in outs]), _arr([m.ctypes.data for m in maps])
        pal = np.zeros(257, np.int32)
        pal[:] = G.palette(257, 2)
        K, size = C.c_int32(0), C.c_int64(0)
        buf = np.zeros(1 << 16, np.uint8)
        if which == "hold":                             # (threshold 256)
            rc = L.nq_hold_frames(h, n, src, idx, dst, W, H, 256, None)
        elif which == "resample":                       # (unknown flag bits)
            rc = L.nq_resample_frames(h, n, src, W, H, 0, 0, W, H, dst, 4, 3, 2)
        elif which == "yuv":                            # (unknown flag bits)
            y = [np.zeros((H, W), np.uint8) for _ in range(n)]
            c = [np.zeros((H // 2, W // 2), np.uint8) for _ in range(2 * n)]
            rc = L.nq_frames_from_yuv(h, n, _arr([a.ctypes.data for a in y]), _arr([a.ctypes.data for a in c[:n]]), _arr([a.ctypes.data for a in c[n:]]),
                                      W, H, W, W // 2, 1, 4, dst)
        elif which == "ordered":                        # (no frame)
            rc = L.nq_dither_ordered(h, 0, src, ws.ctypes.data, hs.ctypes.data, pal.ctypes.data, 16, 8, dst, idx, None)
        elif which == "refine":                         # (65 passes)
            sse, counts = np.zeros(66, np.int64), np.zeros(16, np.int64)
            rc = L.nq_refine_palette(h, n, src, ws.ctypes.data, hs.ctypes.data, pal.ctypes.data, 16, 65, sse.ctypes.data, counts.ctypes.data, C.byref(K))
        elif which == "signatures":                     # (no frame)
            sig = np.zeros((1, 4, 256), np.uint32)
            rc = L.nq_frame_signatures(h, 0, src, W, H, sig.ctypes.data)
        elif which == "png":                            # (a palette of 0 entries)
            table, Ks, offs = np.ascontiguousarray(np.stack([pal[:16]] * n)), np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
            rc = L.nq_encode_png(h, n, idx, ws.ctypes.data, hs.ctypes.data, table.ctypes.data, 16, Ks.ctypes.data, 0, buf.ctypes.data, buf.size, offs.ctypes.data)
        elif which == "apng":                           # (a palette of 257 entries)
            rects = np.zeros((n, 4), np.int32)
            rc = L.nq_encode_apng(h, n, idx, W, H, pal.ctypes.data, 257, None, 0, 0, buf.ctypes.data, buf.size, C.byref(size), rects.ctypes.data)
        elif which == "pnnquan":                        # (width 0)
            rc = L.nq_pnnquan(h, frames[0].ctypes.data, 0, H, 16, pal.ctypes.data, C.byref(K))
        elif which == "dither":                         # (width 0)
            rc = L.nq_dither(h, frames[0].ctypes.data, 0, H, pal.ctypes.data, 16, 1, 1, O.TILED, outs[0].ctypes.data, maps[0].ctypes.data)
        else:
            raise KeyError(which)
        _status(q, rc, -1)
    return fail


def _fail_batch_host(nq, q):
    """nq_convert_batch on host arrays, the handle under test first and the second image of width 0: NQ_ERR_INVALID."""
    imgs = [O._image("WIDE", 5).copy(), O._image("NARROW", 6).copy()]
    other = O.new_handle(nq, 1 - q.KIND)
    try:
        for quantizer, im in zip([q, other], imgs):
            O._point(quantizer, im)
        other.width = 0
        outs, idxs = [np.zeros(im.shape, np.int32) for im in imgs], [np.zeros(im.shape, np.uint16) for im in imgs]
        with pytest.raises(nq.NqError) as ei:
            nq.convert_batch_host([q, other], [im.ctypes.data for im in imgs], 256, True, [o.ctypes.data for o in outs], [i.ctypes.data for i in idxs],
                                  mode=O.TILED, seeds=[1, 2])
        assert ei.value.status == -1
    finally:
        other.close()


def _fail_split_without_distinct(nq, q):
    """The split pipeline on an image with fewer colours than nMaxColors, a LAB handle and no nq_set_distinct: the early return of the
    reference cannot be taken, nq_palette_from_histograms_device ends with NQ_ERR_UNSUPPORTED."""
    import torch
    assert q.KIND == 1
    img = O._few_image("NARROW")
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    s3 = torch.empty(3, dtype=torch.int64, device="cuda")
    L = q._L
    q._check(L.nq_band_scan_device(q._h, C.c_void_p(d_img.data_ptr()), d_img.numel(), 0, 256, C.c_void_p(s3.data_ptr())))
    torch.cuda.synchronize()
    scan = s3.cpu().numpy()
    q._check(L.nq_set_scan(q._h, 256, int(scan[0]), C.c_uint32(int(scan[1]) & 0xFFFFFFFF if scan[0] >= 0 else 0xFFFFFFFF), int(scan[2])))
    hist = torch.zeros(65536 * 5, dtype=torch.float64, device="cuda")
    q._check(L.nq_band_histogram_device(q._h, C.c_void_p(d_img.data_ptr()), d_img.numel(), C.c_void_p(hist.data_ptr())))
    pal, k = np.zeros(256, np.int32), C.c_int32(0)
    rc = L.nq_palette_from_histograms_device(q._h, C.c_void_p(hist.data_ptr()), 1, 256, pal.ctypes.data, C.byref(k))
    torch.cuda.synchronize()
    _status(q, rc, -3, "nq_set_distinct")


FAILURES = {
    "bad_index_gif": _fail_bad_index("nq_encode_gif"), "bad_index_gif_delta_lossy": _fail_bad_index("nq_encode_gif_delta_lossy"),
    "bad_index_gif_local": _fail_bad_index("nq_encode_gif_local"), "bad_index_png": _fail_bad_index("nq_encode_png"),
    "bad_index_apng": _fail_bad_index("nq_encode_apng"), "short_capacity_gif": _fail_short_capacity("gif"),
    "short_capacity_png": _fail_short_capacity("png"), "invalid_convert": _fail_invalid("convert"), "invalid_orient": _fail_invalid("orient"),
    "invalid_lossy": _fail_invalid("lossy"), "invalid_frames": _fail_invalid("frames"), "rejected_band": _fail_band, "invalid_batch_image": _fail_batch,
    "invalid_batch_host_image": _fail_batch_host, "unsupported_split_without_distinct": _fail_split_without_distinct,
}
FAILURES.update({"invalid_" + w: _fail_rejected(w) for w in ("hold", "resample", "yuv", "ordered", "refine", "signatures", "png", "apng", "pnnquan", "dither")})


@pytest.mark.parametrize("failure", sorted(FAILURES))
def test_every_op_after_a_failed_call(nq, oracle, failure):
    """NQ_ERR_REFERENCE_THROWS needs an image beyond 4097 x 4097 (the float count of a bin has to saturate) and stays with
    test_gpu_regressions.py / test_gpu_batch_scale.py."""
    run = _Run(nq, 1, "after " + failure)
    try:
        run.op("convert_tiled_dither_host", "NARROW")          # (a used handle: the failure is not its first call)
        FAILURES[failure](nq, run.q)
        for variant in ("NARROW", "LARGE"):
            for name in O.NAMES:
                run.op(name, variant)
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# D. what a handle holds
# ---------------------------------------------------------------------------------------------------------------------------------
def _held(nq):
    """nq_get_device_bytes once no handle of an earlier test waits for the garbage collector (the count is the process's)."""
    import gc
    gc.collect()
    return nq.device_bytes()


def test_a_repeated_walk_allocates_nothing(nq, oracle):
    """Grow-only buffers: once every call of a workload has run, the same workload allocates nothing."""
    before = _held(nq)
    q = O.new_handle(nq, 1)
    try:
        run_walk(nq, 1, WALK_SEEDS[0], q=q)
        first = nq.device_bytes()
        run_walk(nq, 1, WALK_SEEDS[0], q=q)
        assert nq.device_bytes() - first == 0, "the second walk took %d more bytes of device memory" % (nq.device_bytes() - first)
        assert first > before
    finally:
        q.close()
    assert nq.device_bytes() == before, "nq_destroy left %d bytes" % (nq.device_bytes() - before)


def test_small_calls_after_large_ones_allocate_only_curve_tables(nq, oracle):
    """Every op at LARGE, then every op at WIDE and NARROW: no buffer grows; new are at most the curve tables of new tile shapes, at most
    tile_w * tile_h shapes of at most 4 * tile_w * tile_h bytes (16 x 16 tiles: 256 KB)."""
    before = _held(nq)
    run = _Run(nq, 1, "footprint")
    try:
        for name in O.NAMES:
            run.op(name, "LARGE")
        large = nq.device_bytes()
        for variant in O.SMALL:
            for name in O.NAMES:
                run.op(name, variant)
        grown = nq.device_bytes() - large
        tw, th = O.TILES[0]
        assert 0 <= grown <= tw * th * 4 * tw * th, "the small calls took %d more bytes" % grown
    finally:
        run.close()
    assert nq.device_bytes() == before


def test_sequential_mode_keeps_one_whole_image_curve_table(nq, oracle):
    """REFERENCE_SEQUENTIAL: the tile is the whole image, and its curve table has 4 * w * h bytes.  After one 96 x 80 convert, 24 converts
    of distinct sizes, none larger in either side, leave the handle at most one such table above where it was -- a handle used to keep
    one table per size it had seen until nq_destroy (4 * w * h bytes each).  Every result is the oracle's."""
    import oracle_lib
    before = _held(nq)
    q = O.new_handle(nq, 1)
    sizes = [(96, 80)] + [(96 - 2 * i, 80 - 3 * (i % 5) - i // 5) for i in range(1, 25)]
    assert len(set(sizes)) == 25 and all(33 <= w <= 96 and 33 <= h <= 80 for w, h in sizes)
    try:
        for i, (w, h) in enumerate(sizes):
            img = G.quant_image(w, h, 9700 + i)
            oq = oracle_lib.OracleQuantizer(1, img, seed=5)
            want_argb, want_idx, want_pal = oq.convert(16, True)
            oq.close()
            O._point(q, img)
            out = q.convert(16, True, mode=O.SEQ, seed=5)
            O.compare({"palette": out.palette, "index": out.index, "argb": out.argb},
                      {"palette": want_pal, "index": want_idx.astype(np.uint16), "argb": want_argb}, "sequential convert %d, %d x %d" % (i, w, h))
            if i == 0:
                first = nq.device_bytes()
        grown = nq.device_bytes() - first
        assert grown <= 4 * 96 * 80, "24 smaller images took %d more bytes of device memory (one whole-image table: %d)" % (grown, 4 * 96 * 80)
    finally:
        q.close()
    assert nq.device_bytes() == before
