"""The JNI shim (nquant.android_amd/jni/nquant_jni.c) EXECUTED on the CPU: compiled against the fake JNI runtime of tests/c/jni_fake and
linked to stub_abi.c, a scripted stand-in for the fourteen nq_* functions it calls -- no GPU, nothing of libnquant_hip.so.  Held here:
every argument each native method hands to the ABI is what the Java-side arguments imply; every exit, the failing ones included (a
scripted nq_* status, a JNI allocation that fails at each possible place, a null / short / non-direct argument), releases what it
acquired, leaves exactly one exception, makes no nq_* call after the failure and never exceeds the 16 local references JNI guarantees;
and the same sweeps run once more in a standalone executable under the address and undefined-behaviour sanitizers.  A real JVM is
still not involved (tests/jni_fake.py)."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import jni_fake
from jni_fake import SIGS

H = 0x5000                      # a handle: the stub never looks inside
RT_EXC = "java/lang/RuntimeException"
OOM_EXC = "java/lang/OutOfMemoryError"
PER_FRAME = ["nqConvertBatch", "nqConvertFrames", "nqEncodeGif", "nqEncodeGifDelta", "nqEncodeApng", "nqConvertFramesToGif",
             "nqConvertFramesToApng"]
ONE_SIZE = ("nqEncodeGifDelta", "nqEncodeApng", "nqConvertFramesToApng")
SENTINEL = {"nqCreate": 0, "nqConvert": None, "nqConvertBatch": None, "nqConvertFrames": None}       # every other failing method: -1


@pytest.fixture(scope="module")
def so(tmp_path_factory):
    return jni_fake.build(tmp_path_factory.mktemp("jni_cpu"))


@pytest.fixture(scope="module")
def runtime(so):
    return jni_fake.Runtime(so)


@pytest.fixture
def rt(runtime):
    runtime.reset()
    yield runtime
    runtime.reset()


def make(rt, name, n=3, w=6, h=4, nMax=16, cap=64, delays=True, delta=False, index_out=True, dither=1):
    """Valid Java-side arguments of native method `name`, by parameter name and in order, and the arrays behind them."""
    one = name in ONE_SIZE or delta
    c = SimpleNamespace(n=n, w=w, h=h, nMax=nMax, cap=cap)
    c.ws = [w] * n if one else [w + i % 3 for i in range(n)]
    c.hs = [h] * n if one else [h + i % 2 for i in range(n)]
    c.frames = [np.arange(c.ws[i] * c.hs[i], dtype=np.uint32) + np.uint32(0x01000000 * (i % 200 + 1)) for i in range(n)]
    c.outs = [np.zeros(f.size, np.uint32) for f in c.frames]
    c.maps = [((np.arange(f.size) + i) % 5).astype(np.uint16) for i, f in enumerate(c.frames)]
    c.file = np.full(cap + 8, 0xEE, np.uint8)
    c.palette = [0xFF000000 | (3 * j + 1) for j in range(5)]
    c.delays = [10 + i % 50 for i in range(n)]
    c.seeds = [100 + i for i in range(n)]
    ins = lambda: rt.objects([rt.direct(f) for f in c.frames])
    outs = lambda: rt.objects([rt.direct(o) for o in c.outs])
    maps = lambda: rt.objects([rt.direct(m) for m in c.maps])
    file = lambda: rt.direct(c.file, cap)
    dl = lambda: rt.ints(c.delays) if delays else None
    if name == "nqCreate":
        a = dict(kind=1, device=0)
    elif name in ("nqDestroy", "nqHasAlpha"):
        a = dict(h=H)
    elif name == "nqConvert":
        a = dict(h=H, argb=rt.ints(c.frames[0]), w=c.ws[0], hgt=c.hs[0], nMaxColors=nMax, dither=dither, seed=77, mode=1,
                 outArgb=rt.ints(c.outs[0]), outIndex=rt.shorts(np.zeros(c.frames[0].size)) if index_out else None)
    elif name == "nqConvertBatch":
        a = dict(handles=rt.longs([H + 16 * i for i in range(n)]), **{"in": ins()}, widths=rt.ints(c.ws), heights=rt.ints(c.hs), nMaxColors=nMax,
                 dither=dither, seeds=rt.longs(c.seeds), mode=1, out=outs())
    elif name == "nqConvertFrames":
        a = dict(h=H, **{"in": ins()}, widths=rt.ints(c.ws), heights=rt.ints(c.hs), nMaxColors=nMax, dither=dither, seeds=rt.longs(c.seeds),
                 mode=1, out=outs())
    elif name == "nqGifMaxBytes":
        a = dict(widths=rt.ints(c.ws), heights=rt.ints(c.hs))
    elif name == "nqEncodeGif":
        a = dict(h=H, index=maps(), widths=rt.ints(c.ws), heights=rt.ints(c.hs), palette=rt.ints(c.palette), delaysCs=dl(), loopCount=3,
                 out=file(), cap=cap)
    elif name in ("nqEncodeGifDelta", "nqEncodeApng"):
        a = dict(h=H, index=maps(), width=w, height=h, palette=rt.ints(c.palette), delaysCs=dl(), loopCount=3, out=file(), cap=cap)
    elif name == "nqConvertFramesToGif":
        a = dict(h=H, **{"in": ins()}, widths=rt.ints(c.ws), heights=rt.ints(c.hs), nMaxColors=nMax, dither=dither, seeds=rt.longs(c.seeds),
                 mode=1, delaysCs=dl(), loopCount=3, delta=int(delta), out=file(), cap=cap)
    elif name == "nqPngMaxBytes":
        a = dict(width=w, height=h)
    elif name == "nqEncodePng":
        a = dict(h=H, index=rt.direct(c.maps[0]), width=c.ws[0], height=c.hs[0], palette=rt.ints(c.palette), out=file(), cap=cap)
    elif name == "nqConvertToPng":
        a = dict(h=H, **{"in": rt.direct(c.frames[0])}, width=c.ws[0], height=c.hs[0], nMaxColors=nMax, dither=dither, seed=77, mode=1, out=file(),
                 cap=cap)
    elif name == "nqApngMaxBytes":
        a = dict(n=n, width=w, height=h)
    elif name == "nqConvertFramesToApng":
        a = dict(h=H, **{"in": ins()}, width=w, height=h, nMaxColors=nMax, dither=dither, seeds=rt.longs(c.seeds), mode=1, delaysCs=dl(),
                 loopCount=3, out=file(), cap=cap)
    assert len(a) == len(SIGS[name][1]), name
    return a, c


def run(rt, name, a, **kw):
    return rt.call(name, *a.values(), **kw)


def drop_result(rt, name, res):
    if SIGS[name][0] is jni_fake._vp and res:
        rt.L.fj_release(res)


def the_file(c, size=33):
    want = np.full(c.file.size, 0xEE, np.uint8)
    want[:size] = (np.arange(size) * 7 + 1) & 255
    return want


# ---- argument marshalling, per native method ----
def test_create_destroy_has_alpha_and_the_size_bounds(rt):
    h = run(rt, "nqCreate", dict(kind=1, device=2))
    (fn, rec), = rt.stub_calls()
    assert fn == "nq_create" and (rec["kind"], rec["device"]) == (1, 2) and h != 0 and not rt.clean() and rt.pending() is None
    run(rt, "nqDestroy", dict(h=h))
    assert rt.stub_calls()[1] == ("nq_destroy", {"h": h, "pending": 0})
    for alpha in (0, 1):
        rt.L.st_script(5, 33, 4096, alpha)
        assert run(rt, "nqHasAlpha", dict(h=H)) == alpha and rt.stub_calls()[-1][1]["h"] == H
    rt.L.st_reset()
    a, c = make(rt, "nqGifMaxBytes")
    assert run(rt, "nqGifMaxBytes", a) == 4096 and not rt.clean()
    rec = rt.stub_calls()[0][1]
    assert (rec["n"], rec["K"], rec["segment"]) == (3, 256, 0)
    assert (rec["w0"], rec["wl"], rec["h0_"], rec["hl_"]) == (c.ws[0], c.ws[-1], c.hs[0], c.hs[-1]) and c.ws[-1] != c.hs[-1]
    assert run(rt, "nqPngMaxBytes", dict(width=7, height=9)) == 4096
    rec = rt.stub_calls()[1][1]
    assert (rec["n"], rec["w0"], rec["h0_"], rec["K"], rec["segment"]) == (1, 7, 9, 0, 0)          # K NULL: 256 everywhere
    assert run(rt, "nqApngMaxBytes", dict(n=4, width=7, height=9)) == 4096
    rec = rt.stub_calls()[2][1]
    assert (rec["n"], rec["width"], rec["height"], rec["segment"]) == (4, 7, 9, 0)
    # a size the ABI refuses, and arrays of two lengths: -1, no exception
    assert run(rt, "nqPngMaxBytes", dict(width=-1, height=9)) == -1 and run(rt, "nqApngMaxBytes", dict(n=0, width=7, height=9)) == -1
    assert run(rt, "nqGifMaxBytes", dict(widths=rt.ints([4, -1]), heights=rt.ints([4, 4]))) == -1
    n_before = rt.L.st_ncalls()
    assert run(rt, "nqGifMaxBytes", dict(widths=rt.ints([4, 4]), heights=rt.ints([4]))) == -1 and rt.L.st_ncalls() == n_before
    assert run(rt, "nqGifMaxBytes", dict(widths=None, heights=rt.ints([4]))) == -1
    assert rt.pending() is None and not rt.clean()


@pytest.mark.parametrize("nMax,index_out,dither", [(16, True, 1), (3, False, 0), (2, True, 1), (1, True, 0)])
def test_convert_marshalling(rt, nMax, index_out, dither):
    a, c = make(rt, "nqConvert", w=7, h=5, nMax=nMax, index_out=index_out, dither=dither)
    res = run(rt, "nqConvert", a)
    assert not rt.clean() and rt.pending() is None and res
    K = min(5, max(nMax, 2))
    assert (rt.take_ints(res).view(np.uint32) == 0xFF000000 + np.arange(K)).all()
    (fn, rec), = rt.stub_calls()
    assert fn == "nq_convert"
    assert (rec["h"], rec["width"], rec["height"], rec["nMaxColors"], rec["dither"], rec["seed"], rec["mode"]) == (H, 7, 5, nMax, dither, 77, 1)
    assert (rec["in_first"], rec["in_last"]) == (int(c.frames[0][0]), int(c.frames[0][-1]))
    assert (rec["out_index"] != 0) == index_out
    assert (rt.read(a["argb"], np.uint32) == c.frames[0]).all()                            # the input array is what it was
    assert (rt.read(a["outArgb"], np.uint32) == c.frames[0] ^ 0x00FFFFFF).all()            # the output was copied back (mode 0)
    if index_out:
        assert (rt.read(a["outIndex"], np.uint16) == np.arange(35) % K).all()


def _frames_record(rec, c, mapped=False):
    srcs = c.maps if mapped else c.frames
    assert rec["n"] == c.n and (rec["src0"], rec["srcl"]) == (srcs[0].ctypes.data, srcs[-1].ctypes.data)


@pytest.mark.parametrize("nMax,dither", [(16, 1), (1, 0)])
def test_convert_batch_and_frames_marshalling(rt, nMax, dither):
    stride = max(nMax, 2)
    a, c = make(rt, "nqConvertBatch", n=4, nMax=nMax, dither=dither)
    res = run(rt, "nqConvertBatch", a)
    assert not rt.clean() and rt.pending() is None
    pals = rt.take_int_arrays(res)
    Ks = [max(1, min(5, stride) - i % 3) for i in range(4)]
    assert [len(p) for p in pals] == Ks
    for i, p in enumerate(pals):
        assert (p.view(np.uint32) == 0xFF000000 + (i << 16) + np.arange(Ks[i])).all()
        assert (c.outs[i] == c.frames[i] ^ 0x00FFFFFF).all()
    (fn, rec), = rt.stub_calls()
    assert fn == "nq_convert_batch"
    _frames_record(rec, c)
    assert (rec["nMaxColors"], rec["dither"], rec["mode"], rec["stride"], rec["out_index"]) == (nMax, dither, 1, stride, 0)
    assert (rec["h0"], rec["hl"], rec["dst0"], rec["dstl"]) == (H, H + 48, c.outs[0].ctypes.data, c.outs[-1].ctypes.data)
    assert (rec["w0"], rec["wl"], rec["h0_"], rec["hl_"], rec["seed0"], rec["seedl"]) == (c.ws[0], c.ws[-1], c.hs[0], c.hs[-1], 100, 103)
    assert c.ws[-1] != c.hs[-1] and c.ws[0] != c.hs[0]                                    # a swap would show

    rt.reset()
    a, c = make(rt, "nqConvertFrames", n=3, nMax=nMax, dither=dither)
    res = run(rt, "nqConvertFrames", a)
    assert not rt.clean() and rt.pending() is None
    assert (rt.take_ints(res).view(np.uint32) == 0xFF000000 + np.arange(min(5, stride))).all()
    (fn, rec), = rt.stub_calls()
    assert fn == "nq_convert_frames"
    _frames_record(rec, c)
    assert (rec["h"], rec["nMaxColors"], rec["dither"], rec["mode"], rec["out_index"]) == (H, nMax, dither, 1, 0)
    assert (rec["dst0"], rec["dstl"]) == (c.outs[0].ctypes.data, c.outs[-1].ctypes.data)
    assert (rec["w0"], rec["wl"], rec["h0_"], rec["hl_"], rec["seed0"], rec["seedl"]) == (c.ws[0], c.ws[-1], c.hs[0], c.hs[-1], 100, 102)
    for i in range(3):
        assert (c.outs[i] == c.frames[i] ^ 0x00FFFFFF).all()


def _encoder_record(rec, c, a, delays, one_size):
    _frames_record(rec, c, mapped=True)
    assert (rec["h"], rec["K"], rec["loop"], rec["segment"], rec["cap"], rec["out"]) == (H, 5, 3, 0, c.cap, c.file.ctypes.data)
    assert (rec["pal0"], rec["pall"]) == (c.palette[0], c.palette[-1])
    assert (rec["delays"] != 0) == delays and (rec["delay0"], rec["delayl"]) == ((c.delays[0], c.delays[-1]) if delays else (-1, -1))
    assert (rec["index_first"], rec["index_last"]) == (int(c.maps[0][0]), int(c.maps[-1][-1]))
    if one_size:
        assert (rec["width"], rec["height"], rec["rects"]) == (c.w, c.h, 0) and c.w != c.h
    else:
        assert (rec["w0"], rec["wl"], rec["h0_"], rec["hl_"]) == (c.ws[0], c.ws[-1], c.hs[0], c.hs[-1])


@pytest.mark.parametrize("delays", [True, False])
@pytest.mark.parametrize("name,fn", [("nqEncodeGif", "nq_encode_gif"), ("nqEncodeGifDelta", "nq_encode_gif_delta"), ("nqEncodeApng", "nq_encode_apng")])
def test_encoder_marshalling(rt, name, fn, delays):
    a, c = make(rt, name, delays=delays)
    assert run(rt, name, a) == 33 and not rt.clean() and rt.pending() is None
    (got, rec), = rt.stub_calls()
    assert got == fn
    _encoder_record(rec, c, a, delays, name in ONE_SIZE)
    assert (c.file == the_file(c)).all()                                                   # `out` beyond the size is untouched


def test_encode_png_and_convert_to_png_marshalling(rt):
    a, c = make(rt, "nqEncodePng", w=7, h=5)
    assert run(rt, "nqEncodePng", a) == 33 and not rt.clean() and rt.pending() is None
    (fn, rec), = rt.stub_calls()
    assert fn == "nq_encode_png"
    assert (rec["h"], rec["n"], rec["w0"], rec["h0_"], rec["K0"], rec["stride"], rec["segment"], rec["cap"]) == (H, 1, 7, 5, 5, 5, 0, 64)
    assert (rec["src0"], rec["out"], rec["pal0"], rec["pall"]) == (c.maps[0].ctypes.data, c.file.ctypes.data, c.palette[0], c.palette[-1])
    assert (c.file == the_file(c)).all()
    for nMax, K in ((16, 5), (3, 3), (1, 2)):
        rt.reset()
        a, c = make(rt, "nqConvertToPng", w=7, h=5, nMax=nMax, dither=0)
        assert run(rt, "nqConvertToPng", a) == 33 and not rt.clean() and rt.pending() is None
        (f1, r1), (f2, r2) = rt.stub_calls()
        assert (f1, f2) == ("nq_convert", "nq_encode_png")
        assert (r1["h"], r1["argb"], r1["width"], r1["height"], r1["nMaxColors"], r1["dither"], r1["seed"], r1["mode"]) == \
            (H, c.frames[0].ctypes.data, 7, 5, nMax, 0, 77, 1)
        assert r1["out_index"] == r2["src0"] != 0                                          # the index map the convert wrote is what is encoded
        assert (r2["h"], r2["w0"], r2["h0_"], r2["K0"], r2["stride"], r2["palettes"]) == (H, 7, 5, K, K, r1["out_palette"])     # K, not nMaxColors
        assert (r2["pal0"], r2["pall"], r2["index_first"], r2["index_last"]) == (0xFF000000, 0xFF000000 + K - 1, 0, 34 % K)
        assert (r2["out"], r2["cap"]) == (c.file.ctypes.data, 64) and (c.file == the_file(c)).all()


@pytest.mark.parametrize("name,delta,delays", [("nqConvertFramesToGif", False, True), ("nqConvertFramesToGif", True, False),
                                               ("nqConvertFramesToApng", False, True), ("nqConvertFramesToApng", False, False)])
def test_convert_frames_to_file_marshalling(rt, name, delta, delays):
    a, c = make(rt, name, delta=delta, delays=delays, nMax=4, dither=1)
    assert run(rt, name, a) == 33 and not rt.clean() and rt.pending() is None
    (f1, r1), (f2, r2) = rt.stub_calls()
    assert f1 == "nq_convert_frames"
    assert f2 == ("nq_encode_apng" if name.endswith("Apng") else "nq_encode_gif_delta" if delta else "nq_encode_gif")
    _frames_record(r1, c)
    assert (r1["h"], r1["nMaxColors"], r1["dither"], r1["mode"]) == (H, 4, 1, 1) and r1["out_index"] != 0 and r1["out_argb"] != 0
    assert (r1["w0"], r1["wl"], r1["h0_"], r1["hl_"], r1["seed0"], r1["seedl"]) == (c.ws[0], c.ws[-1], c.hs[0], c.hs[-1], 100, 102)
    assert (r2["h"], r2["n"], r2["K"], r2["palette"], r2["loop"], r2["segment"], r2["out"], r2["cap"]) == \
        (H, 3, 4, r1["out_palette"], 3, 0, c.file.ctypes.data, 64)                         # K is what the convert returned
    assert (r2["pal0"], r2["pall"]) == (0xFF000000, 0xFF000003)
    assert (r2["delays"] != 0) == delays and (r2["delay0"], r2["delayl"]) == ((10, 12) if delays else (-1, -1))
    if f2 == "nq_encode_gif":
        assert (r2["w0"], r2["wl"], r2["h0_"], r2["hl_"]) == (c.ws[0], c.ws[-1], c.hs[0], c.hs[-1])
    else:
        assert (r2["width"], r2["height"], r2["rects"]) == (6, 4, 0)
    assert (c.file == the_file(c)).all()


# ---- failures ----
def _fails_cleanly(rt, name, exc_class, message=None):
    assert not rt.clean(), (name, rt.clean())
    p = rt.pending()
    assert p is not None and p[0] == exc_class, (name, p)
    if message is not None:
        assert p[1] == message, (name, p)
    assert all(rec["pending"] == 0 for _, rec in rt.stub_calls()), name                   # no nq_* call once an exception is pending


COMPOSITES = [("nqConvertFramesToGif", False), ("nqConvertFramesToGif", True), ("nqConvertToPng", False), ("nqConvertFramesToApng", False)]


@pytest.mark.parametrize("name,delta", COMPOSITES)
@pytest.mark.parametrize("k", [1, 2])
def test_scripted_failure_of_the_first_and_of_the_second_call_of_a_composite(rt, name, delta, k):
    a, c = make(rt, name, delta=delta)
    level = rt.counters()["object_bytes"]
    rt.L.st_set_error(b"frame 1: scripted")
    rt.L.st_fail_call(k, -1)
    assert run(rt, name, a) == -1
    _fails_cleanly(rt, name, RT_EXC, "frame 1: scripted")
    assert rt.L.st_ncalls() == k and rt.L.st_last_error_calls() == 1                       # the second call is not made after the first failed
    assert rt.counters()["object_bytes"] == level
    assert (c.file == 0xEE).all()


@pytest.mark.parametrize("name", sorted(set(SIGS) - {"nqDestroy", "nqHasAlpha", "nqGifMaxBytes", "nqPngMaxBytes", "nqApngMaxBytes"}
                                        - {n for n, _ in COMPOSITES}))
def test_scripted_failure_of_the_one_call_of_a_plain_method(rt, name):
    a, c = make(rt, name)
    level = rt.counters()["object_bytes"]
    rt.L.st_fail_call(1, -2)
    res = run(rt, name, a)
    assert res == SENTINEL.get(name, -1)
    _fails_cleanly(rt, name, RT_EXC, "scripted error")
    assert rt.L.st_ncalls() == 1 and rt.counters()["object_bytes"] == level
    if name == "nqConvert":                                                                # nothing of a failed convert reaches the Java arrays
        assert (rt.read(a["outArgb"], np.uint32) == 0).all() and (rt.read(a["outIndex"], np.uint16) == 0).all()


@pytest.fixture(scope="module")
def sweep(runtime, so):
    """Every exported native method, with a JNI allocation failing at the 1st, 2nd, ... allocating call up to the number a successful
    call makes: {name: [what went wrong, ...]} and {name: allocating calls of the successful call}."""
    rt, problems, allocs = runtime, {}, {}
    for name in jni_fake.exported_natives(so):
        bad = problems.setdefault(name, [])
        for delta in ((False, True) if name == "nqConvertFramesToGif" else (False,)):
            rt.reset()
            a, c = make(rt, name, delta=delta)
            drop_result(rt, name, run(rt, name, a))
            if rt.clean() or rt.pending():
                bad.append("the successful call: %s %s" % (rt.clean(), rt.pending()))
            total = allocs[name] = rt.last["alloc_calls"]
            calls_ok = rt.L.st_ncalls()
            for k in range(1, total + 1):
                rt.reset()
                a, c = make(rt, name, delta=delta)
                level = rt.counters()["object_bytes"]
                res = run(rt, name, a, fail_alloc=k)
                tag = "allocation %d of %d fails: " % (k, total)
                if rt.clean():
                    bad.append(tag + rt.clean())
                if rt.pending() != (OOM_EXC, "injected allocation failure"):
                    bad.append(tag + "pending is %s" % (rt.pending(),))                    # the original, not replaced
                if any(rec["pending"] for _, rec in rt.stub_calls()) or rt.L.st_ncalls() > calls_ok:
                    bad.append(tag + "an nq_* call after the failure")
                if res != SENTINEL.get(name, -1):
                    bad.append(tag + "returned %r" % (res,))
                if rt.counters()["object_bytes"] != level:
                    bad.append(tag + "object bytes %d -> %d" % (level, rt.counters()["object_bytes"]))
    rt.reset()
    return problems, allocs


def test_the_sweep_covers_every_exported_native_method(so, sweep):
    problems, allocs = sweep
    exported = jni_fake.exported_natives(so)
    assert exported == sorted(SIGS) and len(exported) == 16
    assert sorted(problems) == exported
    # the methods that touch Java arrays or create objects have something to sweep
    assert {n for n, k in allocs.items() if k == 0} == {"nqCreate", "nqDestroy", "nqHasAlpha", "nqPngMaxBytes", "nqApngMaxBytes", "nqConvertToPng"}
    assert allocs["nqConvert"] == 4 and allocs["nqConvertBatch"] == 4 + 2 + 3              # 4 Get, FindClass, NewObjectArray, n NewIntArray


@pytest.mark.parametrize("name", sorted(SIGS))
def test_allocation_failure_sweep(sweep, name):
    assert sweep[0][name] == []


def test_a_failing_find_class_inside_the_throw_leaves_that_error_alone(rt):
    a, c = make(rt, "nqEncodePng")
    a["palette"] = None                                                                    # the shim's own exception ...
    assert run(rt, "nqEncodePng", a, fail_alloc=1) == -1                                   # ... whose FindClass fails
    _fails_cleanly(rt, "nqEncodePng", OOM_EXC)
    assert rt.L.st_ncalls() == 0


# ---- lengths and capacities: rejected before any nq_* call ----
def _bad_inputs(rt):
    """(native method, description, change of the valid arguments)"""
    def set_to(key, value):
        return lambda a, c: a.__setitem__(key, value(c) if callable(value) else value)

    def last_buffer_short(key, which):
        def change(a, c):
            arrays = getattr(c, which)
            bufs = [rt.direct(x) for x in arrays[:-1]] + [rt.direct(arrays[-1], arrays[-1].size - 1)]
            a[key] = rt.objects(bufs)
        return change

    def one_buffer_short(key, which):
        return lambda a, c: a.__setitem__(key, rt.direct(getattr(c, which)[0], getattr(c, which)[0].size - 1))

    def heap(key):
        return lambda a, c: a.__setitem__(key, rt.heap_buffer(1 << 20))

    def heap_element(key, which):
        return lambda a, c: a.__setitem__(key, rt.objects([rt.direct(x) for x in getattr(c, which)[:-1]] + [rt.heap_buffer(1 << 20)]))

    def null_element(key, which):
        return lambda a, c: a.__setitem__(key, rt.objects([rt.direct(x) for x in getattr(c, which)[:-1]] + [None]))

    short_ints = lambda key: set_to(key, lambda c: rt.ints([6] * (c.n - 1)))
    short_longs = lambda key: set_to(key, lambda c: rt.longs([6] * (c.n - 1)))
    small_file = set_to("out", lambda c: rt.direct(c.file, c.cap - 1))
    empty = lambda key: set_to(key, lambda c: rt.objects([]))
    cases = []
    for name in ("nqEncodeGif", "nqConvertBatch", "nqConvertFrames", "nqConvertFramesToGif"):
        cases += [(name, "widths shorter than the frames", short_ints("widths")), (name, "heights shorter", short_ints("heights")),
                  (name, "widths null", set_to("widths", None))]
    for name in ("nqConvertBatch", "nqConvertFrames", "nqConvertFramesToGif", "nqConvertFramesToApng"):
        cases += [(name, "seeds shorter than in[]", short_longs("seeds")), (name, "seeds null", set_to("seeds", None)),
                  (name, "an in[] buffer of w*h - 1 elements", last_buffer_short("in", "frames")),
                  (name, "a heap buffer in in[]", heap_element("in", "frames")), (name, "a null in in[]", null_element("in", "frames")),
                  (name, "n == 0", empty("in") if name != "nqConvertBatch" else set_to("handles", lambda c: rt.longs([]))),
                  (name, "in null", set_to("in", None))]
    for name in ("nqConvertBatch", "nqConvertFrames"):
        cases += [(name, "out[] shorter than in[]", set_to("out", lambda c: rt.objects([rt.direct(o) for o in c.outs[:-1]]))),
                  (name, "an out[] buffer of w*h - 1 elements", last_buffer_short("out", "outs")),
                  (name, "a heap buffer in out[]", heap_element("out", "outs"))]
    for name in ("nqEncodeGif", "nqEncodeGifDelta", "nqEncodeApng"):
        cases += [(name, "delaysCs shorter than n", short_ints("delaysCs")), (name, "an index buffer of w*h - 1 elements", last_buffer_short("index", "maps")),
                  (name, "a heap buffer in index[]", heap_element("index", "maps")), (name, "n == 0", empty("index")),
                  (name, "index null", set_to("index", None)), (name, "palette null", set_to("palette", None))]
    for name in ("nqConvertFramesToGif", "nqConvertFramesToApng"):
        cases += [(name, "delaysCs shorter than n", short_ints("delaysCs"))]
    for name in ("nqEncodeGif", "nqEncodeGifDelta", "nqEncodeApng", "nqEncodePng", "nqConvertToPng", "nqConvertFramesToGif", "nqConvertFramesToApng"):
        cases += [(name, "an out buffer smaller than cap", small_file), (name, "a heap buffer for out", heap("out")), (name, "out null", set_to("out", None))]
    cases += [("nqEncodePng", "an index buffer of w*h - 1 elements", one_buffer_short("index", "maps")), ("nqEncodePng", "a heap index buffer", heap("index")),
              ("nqEncodePng", "palette null", set_to("palette", None)), ("nqEncodePng", "index null", set_to("index", None)),
              ("nqConvertToPng", "an in buffer of w*h - 1 elements", one_buffer_short("in", "frames")), ("nqConvertToPng", "a heap in buffer", heap("in")),
              ("nqConvert", "argb shorter than w*hgt", set_to("argb", lambda c: rt.ints(c.frames[0][:-1]))),
              ("nqConvert", "outArgb shorter than w*hgt", set_to("outArgb", lambda c: rt.ints(c.outs[0][:-1]))),
              ("nqConvert", "outIndex shorter than w*hgt", set_to("outIndex", lambda c: rt.shorts(np.zeros(c.frames[0].size - 1)))),
              ("nqConvert", "argb null", set_to("argb", None)), ("nqConvert", "outArgb null", set_to("outArgb", None)),
              ("nqConvertFramesToGif", "delta frames of two sizes", set_to("delta", 1))]
    return cases


def test_short_null_and_non_direct_arguments_are_rejected_before_any_abi_call(rt):
    cases = _bad_inputs(rt)
    assert len(cases) > 80
    failures = []
    for name, what, change in cases:
        rt.reset()
        a, c = make(rt, name)
        change(a, c)
        level = rt.counters()["object_bytes"]
        res = run(rt, name, a)
        p = rt.pending()
        if res != SENTINEL.get(name, -1) or rt.clean() or p is None or p[0] != RT_EXC or not p[1] or rt.L.st_ncalls() != 0 \
                or rt.counters()["object_bytes"] != level:
            failures.append((name, what, res, rt.clean(), p, rt.L.st_ncalls()))
    assert failures == []


# ---- local references ----
@pytest.mark.parametrize("n", [1, 17, 600])
@pytest.mark.parametrize("name", PER_FRAME + ["nqConvertFramesToGif/delta"])
def test_local_references_stay_within_16_for_any_number_of_frames(rt, name, n):
    name, _, delta = name.partition("/")
    a, c = make(rt, name, n=n, w=3, h=2, delta=bool(delta))
    res = run(rt, name, a)
    assert rt.pending() is None and not rt.clean(max_locals=16), rt.last
    if name == "nqConvertBatch":
        assert len(rt.take_int_arrays(res)) == n
    elif name == "nqConvertFrames":
        assert len(rt.take_ints(res)) == 5
    else:
        assert res == 33
    assert rt.stub_calls()[0][1]["n"] == n


# ---- the same under the sanitizers ----
def _sweep_executable(tmp_path, sanitize):
    exe = str(tmp_path / ("jni_sweep_san" if sanitize else "jni_sweep"))
    cmd = ["gcc"] + jni_fake.CFLAGS + ["-o", exe, os.path.join(jni_fake.FAKE_DIR, "sweep_main.c")] + jni_fake.sources(True)
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.parametrize("sanitize", [False, True])
def test_sweeps_in_a_standalone_executable_plain_and_under_asan_ubsan(tmp_path, sanitize):
    """tests/c/jni_fake/sweep_main.c: every native method with valid arguments at n = 1, 17 and 600, with an allocation failing at every
    place, with the first and second nq_* call failing, and with every short / null / non-direct argument -- against buffers that are
    malloc'ed to the exact size.  Host code and the stub only: this process never loads the HIP library."""
    exe, r = _sweep_executable(tmp_path, sanitize)
    if sanitize and r.returncode != 0:
        pytest.skip("the sanitizer link failed: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "sweep done: 16 native methods" in r.stdout and "0 problems" in r.stdout
