"""The `_device` entry points on a caller's stream, with no host wait between the producer of their inputs, the call and the consumer
of their outputs (include/nquant_abi.h: nq_set_stream, "asynchronous on the handle's stream").  The gate protocol and the cases are in
stream_gate.py; test_streams_cpu.py checks, without a GPU, that a call which read the poison cannot pass.

  A  every entry point behind a gate on a fresh non-blocking stream, against the restatements (frame kernels, encoders) and the CPU
     oracle (quantizer); the calls documented as asynchronous must have returned while the gate still ran
  B  nq_convert_batch_device, six images of mixed kinds, on 1, 2 and the default number of lanes, on a stream of its own and on the
     NULL stream: the lanes are streams of the library's own and have to start behind the work queued on the first handle's stream
  C  two asynchronous calls back to back on one handle behind one gate -- the second regrows the device table and rewrites the host
     table, for the ordered dither with another palette --, and the caller's pointer and palette arrays are overwritten with decoys
     as soon as each call has returned: what the comment in hold_device (csrc/nq_abi.cpp) says about staged uploads, put to the test
  D  nq_set_stream with the handle idle: the palette, the candidate lists and the cell boxes the handle keeps on the device
  E  two handles on two gated streams, driven in turns from one thread

One process, small shapes: frames of 48 x 40 (the 16-byte paths) and 45 x 37 one element off alignment (the one-element paths), n = 3;
quantizer images of 64 x 64 to 96 x 80, K = 256 and K = 16, 16 x 16 tiles.  Nothing here can fault: poison and decoys are valid
memory and valid inputs, and the gate is a bounded spin.  No case is run twice to look for a race."""
import ctypes as C

import numpy as np
import pytest

import stream_gate as G

pytestmark = pytest.mark.gpu

TILED = 1
CASES = G.cases()


def _u(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same_host(got, want, what):
    if isinstance(want, (bytes, int)) or (isinstance(want, list) and (not want or isinstance(want[0], (bytes, int, tuple)))):
        if isinstance(want, list) and want and isinstance(want[0], tuple):
            got = [tuple(int(v) for v in r) for r in np.asarray(got).tolist()]
        assert got == want, what
    else:
        assert np.asarray(got).shape == np.asarray(want).shape and np.array_equal(_u(got), _u(want)), what


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(nq):
    """Two fresh streams and the calibrated gate (cycles of the spin for G.GATE_MS)."""
    import torch
    c = _Ctx()
    c.S, c.S2 = torch.cuda.Stream(), torch.cuda.Stream()
    c.cycles, c.gate_ms = G.calibrate(c.S)
    print("gate: %d cycles, measured %.1f ms (wanted %.1f)" % (c.cycles, c.gate_ms, G.GATE_MS))
    assert 0.5 * G.GATE_MS <= c.gate_ms <= 2 * G.GATE_MS, "the spin did not calibrate: %r ms" % c.gate_ms
    c.null = torch.cuda.default_stream()
    return c


def _stream_arg(ctx, stream):
    return None if stream is ctx.null else stream.cuda_stream


@pytest.fixture(scope="module")
def q(nq):
    quantizer = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    yield quantizer
    quantizer.close()


def _quantizer(nq, kind, w, h, seed=0):
    cls = nq.PnnLABQuantizer if kind else nq.PnnQuantizer
    quantizer = cls(np.zeros((1, 1), np.int32), mode=TILED, seed=seed, tile=G.TILE)
    quantizer.width, quantizer.height = w, h
    return quantizer


# ---------------------------------------------------------------------------------------------------------------------------------
# one library call per case of part A: (case, quantizer, buffers by group / output name) -> the results that come back on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _arr(ptrs):
    return (C.c_void_p * len(ptrs))(*[int(p) for p in ptrs])


def _call(nq, q, case, b):
    a, kind = case.args, case.name.split("-")[0]
    w, h = a["w"], a["h"]
    n = len(next(iter(case.true.values())))
    ws, hs = [w] * n, [h] * n
    if kind in ("hold", "hold_counts"):
        held = nq.hold_frames_device(q, b["argb"].ptrs, b["io_index"].ptrs, w, h, 4, b["io_argb"].ptrs, counts=a["counts"])
        return {"held": held} if a["counts"] else {}
    if kind == "resample":
        nq.resample_frames_device(q, b["argb"].ptrs, w, h, b["out_argb"].ptrs, a["size"], a["crop"], True)
    elif kind == "yuv":
        p = b["yuv"]
        nq.frames_from_yuv_device(q, p.y, p.u, p.v, *p.geometry(), b["out_argb"].ptrs, bt709=True)
    elif kind == "resample_yuv":
        p = b["yuv"]
        nq.resample_frames_yuv_device(q, p.y, p.u, p.v, *p.geometry(), b["out_argb"].ptrs, a["size"], a["crop"], True, bt709=True)
    elif kind.startswith("orient"):
        nq.orient_frames_device(q, b["argb"].ptrs, w, h, b["out_argb"].ptrs, a["code"])
    elif kind == "yuv_oriented":
        p = b["yuv"]
        nq.frames_from_yuv_device(q, p.y, p.u, p.v, *p.geometry(), b["out_argb"].ptrs, bt709=True, orient=a["code"])
    elif kind == "resample_oriented":
        nq.resample_frames_device(q, b["argb"].ptrs, w, h, b["out_argb"].ptrs, a["size"], a["crop"], True, orient=a["code"])
    elif kind == "resample_yuv_oriented":
        p = b["yuv"]
        nq.resample_frames_yuv_device(q, p.y, p.u, p.v, *p.geometry(), b["out_argb"].ptrs, a["size"], a["crop"], True, bt709=True, orient=a["code"])
    elif kind in ("ordered", "ordered_stats"):
        stats = nq.dither_ordered_device(q, b["argb"].ptrs, ws, hs, a["palette"], a["limit"], b["out_index"].ptrs, b["out_argb"].ptrs, a["stats"])
        return {"stats": stats} if a["stats"] else {}
    elif kind == "refine":
        pal, sse, counts, passes = nq.refine_palette_device(q, b["argb"].ptrs, ws, hs, a["palette"], 3)
        return {"palette": pal, "sse": sse, "counts": counts, "passes": passes}
    elif kind == "signatures":
        return {"sig": nq.frame_signatures_device(q, b["argb"].ptrs, w, h)}
    elif kind == "detect_shots":
        starts, scores = nq.detect_shots_device(q, b["argb"].ptrs, w, h, 0, 1)
        return {"starts": starts, "scores": scores}
    elif kind == "gif":
        return {"file": nq.encode_gif_device(q, b["index"].ptrs, ws, hs, a["palette"], a["delays"], 0)}
    elif kind == "gif_delta":
        data, rects = nq.encode_gif_delta_device(q, b["index"].ptrs, w, h, a["palette"], a["delays"], 0, return_rects=True)
        return {"file": data, "rects": rects}
    elif kind == "png":
        return {"files": nq.encode_png_device(q, b["index"].ptrs, ws, hs, [a["palette"]] * n)}
    elif kind == "apng":
        return {"file": nq.encode_apng_device(q, b["index"].ptrs, w, h, a["palette"], a["delays"], 0)}
    elif kind == "convert_device":
        return {"palette": q.convert_device(b["argb"].ptrs[0], case.quant[1], True, b["out_argb"].ptrs[0], b["out_index"].ptrs[0])}
    elif kind == "pnnquan_dither_device":
        pal = q.pnnquan_device(b["argb"].ptrs[0], case.quant[1])
        q.dither_device(b["argb"].ptrs[0], pal, True, b["out_argb"].ptrs[0], b["out_index"].ptrs[0])
        return {"palette": pal}
    elif kind == "convert_frames_device":
        return {"palette": nq.convert_frames_device(q, b["argb"].ptrs, ws, hs, case.quant[1], True, b["out_argb"].ptrs, b["out_index"].ptrs,
                                                    seeds=a["seeds"])}
    elif kind in ("convert_frames_refined_device", "convert_frames_ordered_device"):
        K = case.quant[1]
        pal, got_K = np.zeros(max(K, 2), np.int32), C.c_int32(0)
        a_w, a_h = np.array(ws, np.int32), np.array(hs, np.int32)
        head = (q._h, n, _arr(b["argb"].ptrs), a_w.ctypes.data, a_h.ctypes.data, K)
        tail = (_arr(b["out_argb"].ptrs), _arr(b["out_index"].ptrs), pal.ctypes.data, C.byref(got_K))
        if kind == "convert_frames_refined_device":
            seeds = np.array(a["seeds"], np.int64)
            q._check(q._L.nq_convert_frames_refined_device(*head, a["refine"], 1, seeds.ctypes.data, TILED, *tail))
        else:
            q._check(q._L.nq_convert_frames_ordered_device(*head, 0, a["limit"], *tail))
        return {"palette": pal[:got_K.value].copy()}
    else:
        raise KeyError(kind)
    return {}


def _buffers(gate, case):
    """The case's inputs (holding the poison) and sentinel-filled outputs, registered with the gate."""
    true, poison, ref = case.inputs(False), case.inputs(True), G.want(case)
    b = {}
    for group in true:
        b[group] = gate.input(group, true[group], poison[group], case.shift, in_place=group.startswith("io_"))
    for name, arrays in ref.items():
        if name.startswith("out_"):
            b[name] = gate.output(name, arrays, case.shift)
    return b


def _check(gate, case, b, host, what):
    ref = G.want(case)
    for name, value in ref.items():
        if name.startswith(("out_", "io_")):
            gate.check(b[name], value, "%s: %s" % (what, name))
        else:
            _same_host(host[name], value, "%s: %s" % (what, name))
    gate.check_inputs(what)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. ordering against a producer and a consumer on the handle's stream
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_point_behind_a_gate(nq, oracle, ctx, q, name):
    case = CASES[name]
    gate = G.Gate(ctx.S, ctx.cycles)
    b = _buffers(gate, case)
    handle = q
    if case.quant:
        handle = _quantizer(nq, case.args["kind"], case.args["w"], case.args["h"], case.args.get("seed", 0))
    try:
        handle.set_stream(ctx.S.cuda_stream)
        if case.asynchronous:                           # step 6 wants a handle warmed by one call of the same shape: no allocation inside
            gate.arm(gate=False)
            _call(nq, handle, case, b)
            gate.finish(False)
        gate.arm()
        host = _call(nq, handle, case, b)
        gate.finish(case.asynchronous, name)
        _check(gate, case, b, host, name)
    finally:
        ctx.S.synchronize()
        if case.quant:
            handle.close()
        else:
            handle.set_stream(None)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. nq_convert_batch_device behind a gate
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_stream", [False, True], ids=["own_stream", "null_stream"])
@pytest.mark.parametrize("lanes", [None, "1", "2"], ids=["default_lanes", "1_lane", "2_lanes"])
def test_batch_reads_its_inputs_behind_the_first_handles_stream(nq, oracle, ctx, monkeypatch, lanes, null_stream):
    """Lanes 1.. of the prepare phase are streams of the library's own: they have to wait for what the first handle's stream holds
    when the call is made (the producer of d_argb[1..]), on a caller's stream and on the NULL stream, which a non-blocking stream
    does not follow either."""
    if lanes is None:
        monkeypatch.delenv("NQ_BATCH_LANES", raising=False)
    else:
        monkeypatch.setenv("NQ_BATCH_LANES", lanes)
    imgs, want = G.batch_images(), G.batch_want()
    stream = ctx.null if null_stream else ctx.S
    gate = G.Gate(stream, ctx.cycles)
    src = [gate.input("argb", [im], [G.invert_rgb(im)]) for im in imgs]
    out = [gate.output("out_argb", [im]) for im in imgs]
    idx = [gate.output("out_index", [im]) for im in imgs]
    qs = [_quantizer(nq, kind, w, h, seed) for (kind, w, h), seed in zip(G.BATCH, G.BATCH_SEEDS)]
    try:
        if not null_stream:
            qs[0].set_stream(stream.cuda_stream)
        gate.arm()
        pals = nq.convert_batch_device(qs, [s.ptrs[0] for s in src], G.BATCH_K, True, [o.ptrs[0] for o in out], [i.ptrs[0] for i in idx])
        gate.finish(False)
        what = "lanes %s, %s" % (lanes or "default", "NULL stream" if null_stream else "own stream")
        bad = [i for i in range(len(imgs)) if not np.array_equal(pals[i], want[i][0])]
        assert not bad, "%s: the palettes of images %s differ from the oracle's" % (what, bad)
        for i in range(len(imgs)):
            gate.check(idx[i], [want[i][1]], "%s: index map %d" % (what, i))
            gate.check(out[i], [want[i][2]], "%s: ARGB output %d" % (what, i))
        gate.check_inputs(what)
    finally:
        stream.synchronize()
        for quantizer in qs:
            quantizer.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# C. two asynchronous calls back to back on one handle behind one gate, the caller's arrays overwritten as soon as a call returns
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_call(L, h, kind, b, args, decoy_argb, decoy_index):
    """One asynchronous call through the ctypes layer; then every array of the caller's is overwritten with decoys."""
    w, hgt = G.PAIR_W, G.PAIR_H
    arrays, pal = [], None
    if kind == "yuv":
        p = b["yuv"]
        n = len(p.y)
        arrays = [_arr(p.y), _arr(p.u), _arr(p.v), _arr(b["out_argb"].ptrs)]
        rc = L.nq_frames_from_yuv_device(h, n, arrays[0], arrays[1], arrays[2], *p.geometry(), G_BT709, arrays[3])
    else:
        n = len(b["argb"].ptrs)
        if kind == "hold":
            arrays = [_arr(b["argb"].ptrs), _arr(b["io_index"].ptrs), _arr(b["io_argb"].ptrs)]
            rc = L.nq_hold_frames_device(h, n, arrays[0], arrays[1], arrays[2], w, hgt, 4, None)
        elif kind == "resample":
            arrays = [_arr(b["argb"].ptrs), _arr(b["out_argb"].ptrs)]
            rc = L.nq_resample_frames_device(h, n, arrays[0], w, hgt, 0, 0, w, hgt, arrays[1], 20, 16, 1)
        elif kind == "orient":
            arrays = [_arr(b["argb"].ptrs), _arr(b["out_argb"].ptrs)]
            rc = L.nq_orient_frames_device(h, n, arrays[0], w, hgt, 6, arrays[1])
        else:
            arrays = [_arr(b["argb"].ptrs), _arr(b["out_argb"].ptrs), _arr(b["out_index"].ptrs)]
            a_w, a_h = np.full(n, w, np.int32), np.full(n, hgt, np.int32)
            pal = (C.c_uint32 * 256)(*[int(v) & 0xFFFFFFFF for v in args["palette"]])
            rc = L.nq_dither_ordered_device(h, n, arrays[0], a_w.ctypes.data, a_h.ctypes.data, pal, 256, 24, arrays[1], arrays[2], None)
    assert rc == 0, (kind, n, L.nq_last_error(h))
    for k, arr in enumerate(arrays):
        index_array = (kind == "hold" and k == 1) or (kind == "ordered" and k == 2)
        decoys = decoy_index.ptrs if index_array else decoy_argb.ptrs
        for i in range(len(arr)):
            arr[i] = decoys[i]
    if pal is not None:
        for i in range(256):
            pal[i] = 0xFF000000 | (0x010101 * (255 - i))


G_BT709 = 1


@pytest.mark.parametrize("kind", G.PAIR_KINDS)
def test_two_asynchronous_calls_back_to_back(nq, ctx, kind):
    """Call 1 (n = 2) returns with its table upload only enqueued behind the gate; call 2 (n = 9, other buffers) rewrites the handle's
    host table and regrows the device table before the gate has ended.  Both must give their references: the runtime has staged the
    small pageable source before hipMemcpyAsync returned, and the regrowing hipFree has waited for the device."""
    gate = G.Gate(ctx.S, ctx.cycles)
    calls = []
    for n in (2, 9):
        ins, ref, args = G.pair_case(kind, n)
        poison = G.poisoned(ins)
        b = {g: gate.input(g, ins[g], poison[g], 0, in_place=g.startswith("io_")) for g in ins}
        for name, arrays in ref.items():
            if name.startswith("out_"):
                b[name] = gate.output(name, arrays)
        calls.append((n, b, ref, args))
    like = [np.zeros((G.PAIR_H, G.PAIR_W), np.int32)] * 9
    decoy_argb, decoy_index = gate.decoy("argb", like), gate.decoy("index", like)
    quantizer = nq.PnnQuantizer(np.zeros((2, 2), np.int32))
    try:
        quantizer.set_stream(ctx.S.cuda_stream)
        gate.arm()
        for n, b, ref, args in calls:
            _pair_call(quantizer._L, quantizer._h, kind, b, args, decoy_argb, decoy_index)
        gate.finish(False)
        for n, b, ref, args in calls:
            for name, value in ref.items():
                gate.check(b[name], value, "%s, call with n = %d: %s" % (kind, n, name))
        gate.check_inputs(kind)
    finally:
        ctx.S.synchronize()
        quantizer.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# D. stream switches with the handle idle
# ---------------------------------------------------------------------------------------------------------------------------------
def _gated_dither(nq, ctx, handle, stream, kind, K, img, seed, pal, shared, new_palette, what):
    """dither_device (after pnnquan_device when new_palette) of img on `stream` behind a gate, against the oracle.  Returns the palette."""
    gate = G.Gate(stream, ctx.cycles)
    src = gate.input("argb", [img], [G.invert_rgb(img)])
    out, idx = gate.output("out_argb", [img]), gate.output("out_index", [img])
    handle.set_stream(_stream_arg(ctx, stream))
    gate.arm()
    if new_palette:
        pal = handle.pnnquan_device(src.ptrs[0], K)
    handle.dither_device(src.ptrs[0], pal, True, out.ptrs[0], idx.ptrs[0], seed=seed)
    gate.finish(False)
    if new_palette:
        want_pal, want_idx, want_argb, _ = G.oracle_convert(kind, img, K, seed)
        assert np.array_equal(pal, want_pal), what
    else:
        want_idx, want_argb = G.oracle_dither(kind, img, K, seed, pal, shared)
    gate.check(idx, [want_idx], what + ": index map")
    gate.check(out, [want_argb], what + ": ARGB output")
    gate.check_inputs(what)
    stream.synchronize()
    return pal


def test_stream_switches_of_an_idle_handle_dither(nq, oracle, ctx):
    """pnnquan_device + dither_device, LAB, K = 256 (candidate lists, cell boxes, the palette kept on the device): on S1, then -- the
    handle idle -- on S2 behind a gate with the SAME palette on a new image (the upload must be repeated there: an earlier one is
    ordered only against S1), then with another palette, then on the NULL stream."""
    kind, K, w, h = 1, 256, 96, 80
    imgs = [G.quant_image(w, h, 8100 + i) for i in range(3)]
    handle = _quantizer(nq, kind, w, h)
    try:
        pal_a = _gated_dither(nq, ctx, handle, ctx.S, kind, K, imgs[0], 81, None, None, True, "first stream")
        shared = G.oracle_convert(kind, imgs[0], K, 81)[3]
        _gated_dither(nq, ctx, handle, ctx.S2, kind, K, imgs[1], 82, pal_a, shared, False, "second stream, same palette")
        pal_b = _gated_dither(nq, ctx, handle, ctx.S2, kind, K, imgs[2], 83, None, None, True, "second stream, new palette")
        assert not np.array_equal(pal_a, pal_b)
        shared = G.oracle_convert(kind, imgs[2], K, 83)[3]
        _gated_dither(nq, ctx, handle, ctx.null, kind, K, imgs[1], 84, pal_b, shared, False, "NULL stream, same palette")
    finally:
        handle.close()


def test_stream_switches_of_an_idle_handle_frames(nq, oracle, ctx):
    """convert_frames_device keeps the candidate lists of its first frame for the others (reuse_lists): three sequences on one handle,
    on S1, on S2 and on the NULL stream, each behind a gate."""
    kind, K, w, h, seeds = 1, 256, 72, 64, [91, 92, 93]
    handle = _quantizer(nq, kind, w, h)
    try:
        for k, stream in enumerate((ctx.S, ctx.S2, ctx.null)):
            frames = [G.quant_image(w, h, 8200 + 10 * k + i) for i in range(3)]
            gate = G.Gate(stream, ctx.cycles)
            src = gate.input("argb", frames, [G.invert_rgb(f) for f in frames])
            out, idx = gate.output("out_argb", frames), gate.output("out_index", frames)
            handle.set_stream(_stream_arg(ctx, stream))
            gate.arm()
            pal = nq.convert_frames_device(handle, src.ptrs, [w] * 3, [h] * 3, K, True, out.ptrs, idx.ptrs, seeds=seeds)
            gate.finish(False)
            want_pal, want_idx, want_argb = G.oracle_frames(kind, frames, K, seeds)
            what = "sequence %d" % k
            assert np.array_equal(pal, want_pal), what
            gate.check(idx, want_idx, what + ": index maps")
            gate.check(out, want_argb, what + ": ARGB outputs")
            gate.check_inputs(what)
            stream.synchronize()
    finally:
        handle.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# E. two handles, two gated streams, one host thread
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_handles_on_two_gated_streams_in_turns(nq, ctx):
    """Orient and ordered dither on one handle, YUV-fused reduction and temporal hold on the other, issued in turns while both gates
    run; all four asynchronous, all four equal to their restatements."""
    plan = [(ctx.S, "orient6-48x40"), (ctx.S2, "resample_yuv-45x37"), (ctx.S, "ordered-48x40"), (ctx.S2, "hold-45x37")]
    gates = {ctx.S: G.Gate(ctx.S, ctx.cycles), ctx.S2: G.Gate(ctx.S2, ctx.cycles)}
    handles = {s: nq.PnnQuantizer(np.zeros((2, 2), np.int32)) for s in gates}
    try:
        for s, handle in handles.items():
            handle.set_stream(s.cuda_stream)
        bufs = [_buffers(gates[s], CASES[name]) for s, name in plan]
        for gated in (False, True):                     # (first the warming calls, then the gated ones)
            for gate in gates.values():
                gate.prepare()
            for gate in gates.values():
                gate.start(gate=gated)
            hosts = [_call(nq, handles[s], CASES[name], b) for (s, name), b in zip(plan, bufs)]
            busy = [gate.finish(False, wait=False) for gate in gates.values()]
            for s in gates:
                s.synchronize()
            assert not gated or all(busy), "a call waited for a gate: streams busy = %s" % busy
        for (s, name), b, host in zip(plan, bufs, hosts):
            _check(gates[s], CASES[name], b, host, name)
    finally:
        for s, handle in handles.items():
            s.synchronize()
            handle.close()
