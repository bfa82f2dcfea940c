"""The JNI shim (nquant.android_amd/jni/nquant_jni.c) EXECUTED against the real libnquant_hip.so on the GPU, under the fake JNI runtime
of tests/c/jni_fake (tests/jni_fake.py).  The test plays the Java host class: it makes the calls PnnQuantizer.java makes, in its order
and with its argument choices (the Java line is cited beside each call), for every one of the 16 native methods, and compares every
result, exactly, with the Python path that the rest of the suite holds to the oracle (nq.convert, nq.convert_frames,
nq.convert_batch_host, the convert_*_to_* pipelines) or with the restatements (gif_ref, gif_delta_ref, png_ref, apng_ref).  After every
native call: no violation of the JNI rules, no element pointer outstanding, at most 16 live local references, no exception pending.
The errors a real library produces each leave one RuntimeException with nq_last_error's text (or the shim's own), the documented
sentinel, everything released, and the handle good for a valid call.  Not held here: a real JVM."""
import ctypes as C

import numpy as np
import pytest

import apng_ref
import gif_delta_ref
import gif_ref
import jni_fake
import png_ref
from gif_delta_cases import palette_of, sequence
from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

SEQUENTIAL, TILED = 0, 1                     # PnnQuantizer.java:13
RT_EXC = "java/lang/RuntimeException"
COMPARED = set()                             # native methods whose result a test here has compared (read by the last test)
FILL = 0xA5


@pytest.fixture(scope="module")
def so(nq, tmp_path_factory):
    return jni_fake.build(tmp_path_factory.mktemp("jni_gpu"), nq.library_path())


@pytest.fixture(scope="module")
def runtime(nq, so):
    return jni_fake.Runtime(so)


@pytest.fixture
def rt(runtime):
    runtime.reset()
    yield runtime
    runtime.reset()


def call(rt, name, *args):
    """A native call that must succeed: the result, after the checks that follow every call."""
    res = rt.call(name, *args)
    assert rt.pending() is None, (name, rt.pending())
    assert not rt.clean(), (name, rt.clean())
    return res


def byte_buffer(rt, cap):
    """ByteBuffer.allocateDirect(cap), filled with a pattern so that what the call leaves alone can be seen."""
    mem = np.full(max(int(cap), 1), FILL, np.uint8)
    return mem, rt.direct(mem, int(cap))


def file_of(mem, size):
    """gifBytes() (PnnQuantizer.java:152-156), and: `out` beyond the size is untouched."""
    assert 0 < size <= mem.size and (mem[size:] == FILL).all()
    return mem[:size].tobytes()


def int_buffers(rt, arrays):
    return rt.objects([rt.direct(a) for a in arrays])


def maps_u16(frames):
    return [np.ascontiguousarray(f, np.uint16).reshape(-1) for f in frames]


# ---- convert() / hasAlpha() ----
def java_convert(rt, kind, img, nMax, dither, seed, mode, with_index):
    """new PnnQuantizer(fname) / PnnLABQuantizer; setSeed; setMode; convert(nMaxColors, dither); hasAlpha(); finalize()."""
    hgt, w = img.shape
    pixels = rt.ints(img)                                                       # PnnQuantizer.java:34-35
    h = call(rt, "nqCreate", kind, 0)                                           # :44
    assert h != 0
    q_pixels = rt.ints(np.zeros(img.size, np.int32))                            # :45
    out_index = rt.shorts(np.zeros(img.size, np.uint16)) if with_index else None
    pal = call(rt, "nqConvert", h, pixels, w, hgt, nMax, int(dither), seed, mode, q_pixels, out_index)      # :46 (outIndex: null there)
    assert pal
    palette = rt.take_ints(pal)
    has_alpha = bool(call(rt, "nqHasAlpha", h))                                 # :51
    call(rt, "nqDestroy", h)                                                    # :241
    assert (rt.read(pixels, np.int32) == img.reshape(-1)).all()                 # the input array is unchanged
    index = rt.read(out_index, np.uint16).reshape(img.shape) if with_index else None
    return palette, rt.read(q_pixels, np.int32).reshape(img.shape), index, has_alpha


@pytest.mark.parametrize("dither", [True, False])
@pytest.mark.parametrize("kind", [0, 1])
def test_convert_and_has_alpha_equal_the_python_path(nq, rt, kind, dither):
    cls = nq.PnnLABQuantizer if kind else nq.PnnQuantizer
    photo = synth.gradient_noise(96, 64, 400 + kind)
    cases = [(photo, 256), (photo, 64), (photo, 2), (synth.few_colors(80, 48, 410, 7), 16),
             (synth.with_alpha(photo, 420, p_transparent=0.02, p_semi=0.0), 64)]
    for i, (img, nMax) in enumerate(cases):
        for mode in ((SEQUENTIAL, TILED) if i == 0 else (SEQUENTIAL,) if i % 2 else (TILED,)):     # both modes at 256, then alternating
            with_index = (i + mode) % 2 == 0
            seed = 1000 + 7 * i
            rt.reset()
            palette, argb, index, has_alpha = java_convert(rt, kind, img, nMax, dither, seed, mode, with_index)
            q = cls(img, mode=mode, seed=seed)
            want = q.convert(nMax, dither)
            want_alpha = q.hasAlpha()
            q.close()
            assert len(palette) == len(want.palette) and (palette == want.palette).all(), (i, mode)
            assert (argb == want.argb).all(), (i, mode)
            if with_index:
                assert (index == want.index).all(), (i, mode)
            assert has_alpha == want_alpha == (i == 4), (i, mode)
    assert len(palette) <= 64
    few = java_convert(rt, kind, cases[3][0], 16, dither, 5, TILED, True)[0]
    assert len(few) < 16                                                         # the returned K is below nMaxColors
    COMPARED.update({"nqCreate", "nqDestroy", "nqConvert", "nqHasAlpha"})


# ---- convertBatch() ----
def java_convert_batch(rt, kinds, imgs, seeds, nMax, dither, mode):
    """PnnQuantizer.convertBatch (PnnQuantizer.java:57-71)."""
    handles = [call(rt, "nqCreate", k, 0) for k in kinds]                       # :64
    ins = [np.ascontiguousarray(im, np.int32).reshape(-1).copy() for im in imgs]
    outs = [np.zeros(im.size, np.int32) for im in imgs]
    res = call(rt, "nqConvertBatch", rt.longs(handles), int_buffers(rt, ins), rt.ints([im.shape[1] for im in imgs]),
               rt.ints([im.shape[0] for im in imgs]), nMax, int(dither), rt.longs(seeds), mode, int_buffers(rt, outs))      # :67
    assert res
    palettes = rt.take_int_arrays(res)
    for h in handles:
        call(rt, "nqDestroy", h)
    for a, im in zip(ins, imgs):
        assert (a == im.reshape(-1)).all()
    return palettes, outs


def python_batch(nq, kinds, imgs, seeds, nMax, dither):
    qs = []
    for kind, im, seed in zip(kinds, imgs, seeds):
        q = (nq.PnnLABQuantizer if kind else nq.PnnQuantizer)(np.zeros((1, 1), np.int32), mode=TILED, seed=seed)
        q.height, q.width = im.shape
        qs.append(q)
    ins = [np.ascontiguousarray(im, np.int32).reshape(-1).copy() for im in imgs]
    outs = [np.zeros(im.size, np.int32) for im in imgs]
    pals = nq.convert_batch_host(qs, [a.ctypes.data for a in ins], nMax, dither, [a.ctypes.data for a in outs])
    for q in qs:
        q.close()
    return pals, outs


def test_convert_batch_equals_the_python_batch_and_keeps_local_references_bounded(nq, rt):
    # five images of different sizes and mixed kinds, as tests/test_gpu_boundary.py::test_convert_batch_host_buffers_vs_oracle
    batches = [([1, 1, 1, 1, 0], [synth.gradient_noise(96 + 8 * i, 80, 320 + i) for i in range(4)] + [synth.uniform_rgb(64, 72, 330)], 256),
               ([i % 2 for i in range(40)], [synth.gradient_noise(16 + i % 5, 12 + i % 3, 500 + i) for i in range(40)], 16)]
    for kinds, imgs, nMax in batches:
        rt.reset()
        seeds = [21 + i for i in range(len(imgs))]
        got_pals, got_outs = java_convert_batch(rt, kinds, imgs, seeds, nMax, True, TILED)
        assert rt.last["peak_locals"] <= 16
        want_pals, want_outs = python_batch(nq, kinds, imgs, seeds, nMax, True)
        assert [len(p) for p in got_pals] == [len(p) for p in want_pals]                  # the int[n][] result has lengths K[i]
        for i in range(len(imgs)):
            assert (got_pals[i] == want_pals[i]).all(), i
            assert (got_outs[i] == want_outs[i]).all(), i
    COMPARED.add("nqConvertBatch")


# ---- convertFrames() ----
def test_convert_frames_equals_the_python_path(nq, rt):
    frames = [synth.gradient_noise(96, 64, 600), synth.gradient_noise(128, 96, 601), synth.gradient_noise(57, 33, 602)]
    seeds = [3, 4, 5]
    for kind, nMax, dither in ((1, 64, True), (0, 256, False)):
        rt.reset()
        ins = [np.ascontiguousarray(f, np.int32).reshape(-1).copy() for f in frames]
        outs = [np.zeros(f.size, np.int32) for f in frames]
        h = call(rt, "nqCreate", kind, 0)                                       # PnnQuantizer.java:81
        pal = call(rt, "nqConvertFrames", h, int_buffers(rt, ins), rt.ints([f.shape[1] for f in frames]), rt.ints([f.shape[0] for f in frames]),
                   nMax, int(dither), rt.longs(seeds), TILED, int_buffers(rt, outs))     # :83
        call(rt, "nqDestroy", h)                                                # :85
        palette = rt.take_ints(pal)
        want_pal, want = nq.convert_frames(kind, frames, nMax, dither, seeds=seeds)
        assert len(palette) == len(want_pal) and (palette == want_pal).all()
        for i, f in enumerate(frames):
            assert (outs[i].reshape(f.shape) == want[i].argb).all(), (kind, i)
            assert (ins[i] == f.reshape(-1)).all()
    COMPARED.add("nqConvertFrames")


# ---- the size bounds ----
def test_size_bounds_equal_the_python_path(nq, rt):
    for ws, hs in (([6], [4]), ([128, 1, 37], [96, 777, 91]), ([65535], [65535])):
        assert call(rt, "nqGifMaxBytes", rt.ints(ws), rt.ints(hs)) == nq.gif_max_bytes(ws, hs)               # PnnQuantizer.java:147
    for w, h in ((6, 4), (128, 96), (1, 777), (65535, 3)):
        assert call(rt, "nqPngMaxBytes", w, h) == nq.png_max_bytes([w], [h])                                # :189
        for n in (1, 4):
            assert call(rt, "nqApngMaxBytes", n, w, h) == nq.apng_max_bytes(n, w, h)                        # :231
    # an invalid size, arrays of two lengths: -1 (the Java side then throws IllegalArgumentException, :148), no exception from here
    assert call(rt, "nqGifMaxBytes", rt.ints([6, -1]), rt.ints([4, 4])) == -1
    assert call(rt, "nqGifMaxBytes", rt.ints([6, 6]), rt.ints([4])) == -1
    assert call(rt, "nqGifMaxBytes", rt.ints([]), rt.ints([])) == -1
    assert call(rt, "nqPngMaxBytes", -1, 4) == -1 and call(rt, "nqPngMaxBytes", 4, 65536) == -1
    assert call(rt, "nqApngMaxBytes", 2, -1, 4) == -1 and call(rt, "nqApngMaxBytes", 0, 4, 4) == -1
    COMPARED.update({"nqGifMaxBytes", "nqPngMaxBytes", "nqApngMaxBytes"})


# ---- the encoders ----
def java_encode_gif(rt, frames, pal, delays, loop):
    """PnnQuantizer.encodeGif (PnnQuantizer.java:94-102)."""
    ws, hs = [f.shape[1] for f in frames], [f.shape[0] for f in frames]
    cap = call(rt, "nqGifMaxBytes", rt.ints(ws), rt.ints(hs))                   # :95, :147
    mem, out = byte_buffer(rt, cap)                                             # :150
    h = call(rt, "nqCreate", 0, 0)                                              # :96
    size = call(rt, "nqEncodeGif", h, int_buffers(rt, maps_u16(frames)), rt.ints(ws), rt.ints(hs), rt.ints(pal),
                None if delays is None else rt.ints(delays), loop, out, cap)    # :98
    call(rt, "nqDestroy", h)                                                    # :100
    return file_of(mem, size)


def java_encode_one_size(rt, L, name, frames, pal, delays, loop):
    """PnnQuantizer.encodeGifDelta (PnnQuantizer.java:109-120) and encodeApng (:201-209)."""
    hgt, w = frames[0].shape
    if name == "nqEncodeApng":
        cap = call(rt, "nqApngMaxBytes", len(frames), w, hgt)                   # :202, :231
    else:
        cap = call(rt, "nqGifMaxBytes", rt.ints([w] * len(frames)), rt.ints([hgt] * len(frames)))            # :110-113
    mem, out = byte_buffer(rt, cap)
    h = call(rt, "nqCreate", 0, 0)                                              # :114, :203
    size = rt.call(name, h, int_buffers(rt, maps_u16(frames)), w, hgt, rt.ints(pal), None if delays is None else rt.ints(delays), loop, out,
                   cap)                                                         # :116, :205
    err = rt.pending()
    text = (L.nq_last_error(C.c_void_p(h)) or b"").decode()
    assert not rt.clean(), rt.clean()
    rt.clear()
    call(rt, "nqDestroy", h)                                                    # :118, :207
    if err is not None:
        assert size == -1 and (mem == FILL).all()
        raise jni_fake.JavaException(err[0], err[1] + ("" if err[1] == text else " != nq_last_error: " + text))
    return file_of(mem, size)


def java_encode_png(rt, index, pal):
    """PnnQuantizer.encodePng (PnnQuantizer.java:162-170)."""
    hgt, w = index.shape
    cap = call(rt, "nqPngMaxBytes", w, hgt)                                     # :163, :189
    mem, out = byte_buffer(rt, cap)
    h = call(rt, "nqCreate", 0, 0)                                              # :164
    size = call(rt, "nqEncodePng", h, rt.direct(maps_u16([index])[0]), w, hgt, rt.ints(pal), out, cap)       # :166
    call(rt, "nqDestroy", h)                                                    # :168
    return file_of(mem, size)


def _clear_entry(pal, at):
    pal = np.array(pal, np.int64) & 0xFFFFFFFF
    pal[at] &= 0x00FFFFFF
    return pal


@pytest.mark.parametrize("K", [5, 64, 256])
def test_encoders_equal_the_restatements(nq, rt, K):
    L = nq.load_library()
    rng = np.random.default_rng(700 + K)
    opaque = np.array(palette_of(K, rng), np.int64) & 0xFFFFFFFF
    clear = _clear_entry(opaque, 2)                                              # one palette with an alpha-0 entry
    same = sequence(37, 91, K, rng)[:4]                                          # frames of one size that change in places
    mixed = [rng.integers(0, K, s) for s in ((37, 91), (1, 200), (96, 128))]    # frames of three sizes
    for pal in (opaque, clear):
        for delays, loop in ((None, 0), ([3, 0, 65535, 7], 5)):
            d3 = None if delays is None else delays[:3]
            rt.reset()
            assert java_encode_gif(rt, mixed, pal, d3, loop) == gif_ref.encode(mixed, pal, delays_cs=d3, loop=loop)
            assert java_encode_one_size(rt, L, "nqEncodeApng", same, pal, delays, loop) == apng_ref.encode(same, pal, delays_cs=delays, loop=loop)
            if pal is opaque:
                assert java_encode_one_size(rt, L, "nqEncodeGifDelta", same, pal, delays, loop) == \
                    gif_delta_ref.encode(same, pal, delays_cs=delays, loop=loop)
        rt.reset()
        assert java_encode_png(rt, mixed[0], pal) == png_ref.encode(mixed[0], pal)
    # the alpha-0 entry: GIF writes it as the transparent index, APNG takes crop mode, delta GIF with two frames refuses it
    assert gif_ref.transparent_index(clear) == 2
    screen, _, gif_frames = gif_ref.parse(java_encode_gif(rt, mixed, clear, None, 0))
    assert screen["background"] == 2 and [f["transparency"] for f in gif_frames] == [2] * 3
    _, frames_parsed = apng_ref.parse(java_encode_one_size(rt, L, "nqEncodeApng", same, clear, None, 0))
    assert [p["blend"] for p in frames_parsed] == [0] * len(same)
    if K < 256:
        _, frames_parsed = apng_ref.parse(java_encode_one_size(rt, L, "nqEncodeApng", same, opaque, None, 0))
        assert [p["blend"] for p in frames_parsed] == [0] + [1] * (len(same) - 1)            # mark mode, for contrast
    with pytest.raises(jni_fake.JavaException) as e:
        java_encode_one_size(rt, L, "nqEncodeGifDelta", same[:2], clear, None, 0)
    assert e.value.cls == RT_EXC and "alpha" in e.value.message and "!=" not in e.value.message
    assert java_encode_one_size(rt, L, "nqEncodeGifDelta", same[:1], clear, None, 0) == gif_ref.encode(same[:1], clear)    # one frame: allowed
    COMPARED.update({"nqEncodeGif", "nqEncodeGifDelta", "nqEncodePng", "nqEncodeApng"})


# ---- the pipelines, on the 128 x 96 sprite animation of tests/test_gpu_apng.py ----
@pytest.mark.parametrize("kind,K", [(1, 255), (0, 64)])
def test_convert_pipelines_equal_the_python_path(nq, rt, kind, K):
    from test_gpu_apng import _animation
    frames = _animation()
    n, (hgt, w) = len(frames), frames[0].shape
    seeds, delays = [5] * n, [4] * n
    ins = [np.ascontiguousarray(f, np.int32).reshape(-1).copy() for f in frames]
    for delta in (False, True):                                                 # PnnQuantizer.convertFramesToGif (PnnQuantizer.java:126-142)
        rt.reset()
        cap = call(rt, "nqGifMaxBytes", rt.ints([w] * n), rt.ints([hgt] * n))   # :134, :147
        mem, out = byte_buffer(rt, cap)
        h = call(rt, "nqCreate", kind, 0)                                       # :135
        size = call(rt, "nqConvertFramesToGif", h, int_buffers(rt, ins), rt.ints([w] * n), rt.ints([hgt] * n), K, 1, rt.longs(seeds), TILED,
                    rt.ints(delays), 0, int(delta), out, cap)                   # :137
        call(rt, "nqDestroy", h)                                                # :140
        assert file_of(mem, size) == nq.convert_frames_to_gif(kind, frames, K, True, delays_cs=delays, loop=0, seeds=seeds, delta=delta)[0], delta
    rt.reset()                                                                  # PnnQuantizer.convertToPng (:176-184)
    cap = call(rt, "nqPngMaxBytes", w, hgt)                                     # :177, :189
    mem, out = byte_buffer(rt, cap)
    h = call(rt, "nqCreate", kind, 0)                                           # :178
    size = call(rt, "nqConvertToPng", h, rt.direct(ins[1]), w, hgt, K, 1, 5, TILED, out, cap)               # :180
    call(rt, "nqDestroy", h)                                                    # :182
    assert file_of(mem, size) == nq.convert_to_png(kind, frames[1], K, True, seed=5)[0]
    rt.reset()                                                                  # PnnQuantizer.convertFramesToApng (:216-226)
    cap = call(rt, "nqApngMaxBytes", n, w, hgt)                                 # :218, :231
    mem, out = byte_buffer(rt, cap)
    h = call(rt, "nqCreate", kind, 0)                                           # :219
    size = call(rt, "nqConvertFramesToApng", h, int_buffers(rt, ins), w, hgt, K, 1, rt.longs(seeds), TILED, rt.ints(delays), 0, out, cap)   # :221
    call(rt, "nqDestroy", h)                                                    # :224
    assert file_of(mem, size) == nq.convert_frames_to_apng(kind, frames, K, True, delays_cs=delays, loop=0, seeds=seeds)[0]
    for a, f in zip(ins, frames):
        assert (a == f.reshape(-1)).all()
    COMPARED.update({"nqConvertFramesToGif", "nqConvertToPng", "nqConvertFramesToApng"})


# ---- errors that a real library produces ----
def test_errors_leave_one_exception_the_sentinel_and_a_usable_handle(nq, rt):
    L = nq.load_library()
    rng = np.random.default_rng(9)
    K = 7
    pal = np.array(palette_of(K, rng), np.int64) & 0xFFFFFFFF
    a = rng.integers(0, K, (37, 91))
    b = a.copy()
    b[20:30, 40:80] = (b[20:30, 40:80] + 1) % K
    want_png, want_apng = png_ref.encode(a, pal), apng_ref.encode([a, b], pal)
    argb = [np.ascontiguousarray(synth.gradient_noise(32 + 8 * i, 24, 800 + i), np.int32).reshape(-1) for i in range(2)]
    h = call(rt, "nqCreate", 1, 0)

    def png(index=a, palette=pal, cap=None, out=None, index_buffer=None):
        full = call(rt, "nqPngMaxBytes", 91, 37)
        cap = full if cap is None else cap
        mem, buf = byte_buffer(rt, cap)
        res = rt.call("nqEncodePng", h, rt.direct(maps_u16([index])[0]) if index_buffer is None else index_buffer, 91, 37, rt.ints(palette),
                      buf if out is None else out, cap)
        return res, mem

    def valid():
        rt.clear()
        res, mem = png()
        assert rt.pending() is None and not rt.clean() and file_of(mem, res) == want_png

    def failed(res, own_text=None):
        """One pending RuntimeException -- nq_last_error's text of this handle, or the shim's own --, the sentinel, everything released; then
        a valid call on the same handle."""
        p = rt.pending()
        assert res == -1 and p is not None and p[0] == RT_EXC and not rt.clean(), (res, p, rt.clean())
        if own_text is None:
            assert p[1] == (L.nq_last_error(C.c_void_p(h)) or b"").decode() and p[1], p
        else:
            assert own_text in p[1], p
        valid()

    valid()
    res, mem = png(palette=[])                                                   # K = 0
    failed(res)
    assert (mem == FILL).all()
    failed(png(palette=list(pal) * 37)[0])                                       # K = 259 > 256
    failed(png(palette=np.arange(257) | 0xFF000000)[0])                          # K = 257
    bad = a.copy()
    bad[5, 5] = K                                                                # an index >= K
    failed(png(index=bad)[0])
    res, mem = png(cap=len(want_png) - 1)                                        # cap one byte short
    failed(res)
    assert (mem == FILL).all()
    failed(png(out=rt.heap_buffer(1 << 20))[0], "direct")                        # a heap buffer where a direct one is required
    failed(png(index_buffer=rt.heap_buffer(1 << 20))[0], "direct")
    # the same for the animation encoder, then its valid call
    cap = call(rt, "nqApngMaxBytes", 2, 91, 37)
    mem, out = byte_buffer(rt, cap)
    frames_ab = lambda x, y: int_buffers(rt, maps_u16([x, y]))
    failed(rt.call("nqEncodeApng", h, frames_ab(a, bad), 91, 37, rt.ints(pal), None, 0, out, cap))
    assert (mem == FILL).all()
    failed(rt.call("nqEncodeGifDelta", h, frames_ab(a, b), 91, 37, rt.ints(_clear_entry(pal, 1)), None, 0, out, cap))
    size = call(rt, "nqEncodeApng", h, frames_ab(a, b), 91, 37, rt.ints(pal), None, 0, out, cap)
    assert file_of(mem, size) == want_apng
    # the pipelines: delta frames of two sizes, seeds null, a heap buffer in in[]
    mem, out = byte_buffer(rt, 1 << 16)
    res = rt.call("nqConvertFramesToGif", h, int_buffers(rt, argb), rt.ints([32, 40]), rt.ints([24, 24]), 16, 1, rt.longs([1, 1]), TILED, None, 0, 1,
                  out, 1 << 16)
    failed(res, "one size")
    same = [argb[0], argb[0].copy()]
    failed(rt.call("nqConvertFramesToApng", h, int_buffers(rt, same), 32, 24, 16, 1, None, TILED, None, 0, out, 1 << 16), "seeds is null")
    failed(rt.call("nqConvertFramesToApng", h, rt.objects([rt.direct(argb[0]), rt.heap_buffer(768)]), 32, 24, 16, 1, rt.longs([1, 1]), TILED, None,
                   0, out, 1 << 16), "direct")
    failed(rt.call("nqConvertFramesToApng", h, int_buffers(rt, same), 32, 24, 16, 1, rt.longs([1, 1]), TILED, None, -1, out, 1 << 16))   # the second
    #                                                                          nq_* call of the pipeline fails: a loop count the encoder refuses
    assert (mem == FILL).all()
    # convert(): a size the library refuses -> NULL, a RuntimeException with its text
    res = rt.call("nqConvert", h, rt.ints(argb[0]), 0, 24, 16, 1, 1, TILED, rt.ints(np.zeros(768)), None)
    p = rt.pending()
    assert res is None and p is not None and p[0] == RT_EXC and p[1] == (L.nq_last_error(C.c_void_p(h)) or b"").decode() and not rt.clean()
    valid()
    size = call(rt, "nqConvertFramesToApng", h, int_buffers(rt, same), 32, 24, 16, 1, rt.longs([1, 1]), TILED, None, 0, out, 1 << 16)
    assert file_of(mem, size) == nq.convert_frames_to_apng(1, [x.reshape(24, 32) for x in same], 16, True, seeds=[1, 1])[0]
    call(rt, "nqDestroy", h)


def test_every_exported_native_method_was_compared(so):
    """Runs last in this file: the tests above record in COMPARED every native method whose result they compared."""
    exported = jni_fake.exported_natives(so)
    assert exported == sorted(jni_fake.SIGS) and len(exported) == 16
    assert sorted(COMPARED) == exported
    assert set(exported) <= jni_fake.Runtime.called
