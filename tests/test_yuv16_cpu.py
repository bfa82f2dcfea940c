"""CPU-side checks of the 10-bit YUV input (include/nquant_abi.h "10-bit YUV input"): the interface (the four symbols in the header and in
the built library, none of them taking a handle, and the Python entry points), the committed tables (tools/make_hdr_luts.py reproduces
include/nq_hdr_luts.inc byte for byte; the landmarks, monotonicity, the gamut rows), and the restatement in yuv16_ref.py that the GPU
tests compare against: its coefficients from the exact rationals and the header's table, grey staying grey in every mode, the SDR path
within one level of the float64 formula, the PQ / HLG path against a float64 statement of the same pipeline without tables or fixed
point, the bucketing of O against the unbucketed curve; and the Python layer's argument checks, which need no device."""
import inspect
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import yuv16_ref as Y
from conftest import HAS_GPU, ROOT

MATRICES = (0, Y.BT709, Y.BT2020)
SYMBOLS = ("nq_frames_from_yuv16_device", "nq_frames_from_yuv16", "nq_resample_frames_yuv16_device", "nq_resample_frames_yuv16")
# (flag word, its name): every matrix and range in SDR, the BT.2020 matrix in PQ and HLG
MODES = [(m | r, "sdr") for m in MATRICES for r in (0, Y.FULL_RANGE)] + [(Y.BT2020 | r | t, n) for t, n in ((Y.PQ, "pq"), (Y.HLG, "hlg"))
                                                                          for r in (0, Y.FULL_RANGE)]


def _header():
    return open(os.path.join(ROOT, "include", "nquant_abi.h")).read()


def test_symbols_are_declared_exported_and_take_no_handle(nq):
    L = nq.load_library()
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert name in nq.abi_symbols() and hasattr(L, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, name
        assert "nq_handle" not in m.group(1) and re.match(r"\s*int\s+device\b", m.group(1)), name
        assert ("void* hip_stream" in m.group(1)) == name.endswith("_device"), name
        assert m.group(1).count("const uint16_t* const*") == 3 and "uint32_t* const*" in m.group(1), name
    for flag, value in (("NQ_YUV16_BT2020", 4), ("NQ_YUV16_MSB", 8), ("NQ_YUV16_PQ", 16), ("NQ_YUV16_HLG", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), header), flag
    assert L.nq_abi_version() == 1
    for name in ("frames_from_yuv16", "frames_from_yuv16_device", "resample_frames_yuv16", "resample_frames_yuv16_device", "yuv16_planes"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    for fn in (nq.convert_frames_to_gif, nq.convert_shots_to_gif, nq.convert_clip_to_gif, nq.convert_frames_to_apng, nq.convert_frames_to_webp,
               nq.convert_frames_refined, nq.convert_frames_ordered):
        p = inspect.signature(fn).parameters
        assert p["yuv16"].default is None and p["yuv"].default is None, fn.__name__
        # the GIF converters keep `delta` last, as every keyword added before this one left it (test_gif_local_cpu, test_gif_delta_cpu,
        # test_orient_cpu and test_shots_cpu hold them to it); everywhere else the new keyword is the last one, behind all earlier ones
        last = "delta" if fn in (nq.convert_frames_to_gif, nq.convert_shots_to_gif, nq.convert_clip_to_gif) else "yuv16"
        assert list(p)[-1] == last and list(p)[-2:] in (["yuv16", "delta"], ["orient", "yuv16"], ["delta", "yuv16"]), fn.__name__
    p = inspect.signature(nq.resample_frames_yuv16).parameters
    assert [p[k].default for k in ("crop", "linear", "matrix", "full_range", "transfer", "msb", "device")] == [None, True, None, False, "sdr", True, 0]


def test_invalid_arguments_are_refused_before_any_device_is_touched(nq):
    """These hold with or without a GPU: the checks come first, and the text is the thread's handle-free one."""
    import ctypes as C
    L = nq.load_library()
    y = np.zeros(8 * 4 + 8, np.uint16)
    uv = np.zeros(8 * 2 + 8, np.uint16)
    out = np.full(8 * 4, -9, np.int32)
    arr = lambda p: (C.c_void_p * 1)(p)

    def call(device=0, n=1, w=8, h=4, ys=8, cs=8, step=2, flags=Y.MSB | Y.BT2020 | Y.PQ, yp=y.ctypes.data, up=uv.ctypes.data, vp=uv.ctypes.data + 2,
             dp=out.ctypes.data, fused=None):
        if fused is None:
            return L.nq_frames_from_yuv16(device, n, arr(yp), arr(up), arr(vp), w, h, ys, cs, step, flags, arr(dp))
        cx, cy, cw, ch, dw, dh, rflags = fused
        return L.nq_resample_frames_yuv16(device, n, arr(yp), arr(up), arr(vp), w, h, ys, cs, step, flags, cx, cy, cw, ch, arr(dp), dw, dh, rflags)

    bad = [dict(n=0), dict(n=65536), dict(w=0), dict(w=65536), dict(h=0), dict(h=65536), dict(ys=7), dict(step=0), dict(step=3), dict(cs=6),
           dict(step=1, cs=3), dict(flags=64), dict(flags=-1), dict(flags=Y.BT709 | Y.BT2020), dict(flags=Y.PQ | Y.HLG), dict(device=-1),
           dict(yp=None), dict(up=None), dict(vp=None), dict(dp=None), dict(yp=y.ctypes.data + 1), dict(up=uv.ctypes.data + 1, vp=uv.ctypes.data + 3),
           dict(dp=out.ctypes.data + 2), dict(dp=y.ctypes.data), dict(fused=(0, 0, 0, 4, 1, 1, 1)), dict(fused=(1, 0, 8, 4, 2, 2, 1)),
           dict(fused=(0, 0, 8, 4, 9, 4, 1)), dict(fused=(0, 0, 8, 4, 0, 4, 1)), dict(fused=(0, 0, 8, 4, 4, 2, 2))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert (L.nq_last_error(None) or b"") != b"", kw
        assert (out == -9).all(), kw
    assert L.nq_frames_from_yuv16(0, 1, None, None, None, 8, 4, 8, 8, 2, 0, None) == -1
    assert L.nq_frames_from_yuv16_device(0, None, 1, None, None, None, 8, 4, 8, 8, 2, 0, None) == -1
    assert L.nq_resample_frames_yuv16(0, 1, None, None, None, 8, 4, 8, 8, 2, 0, 0, 0, 8, 4, None, 4, 2, 1) == -1
    assert L.nq_resample_frames_yuv16_device(0, None, 1, None, None, None, 8, 4, 8, 8, 2, 0, 0, 0, 8, 4, None, 4, 2, 1) == -1
    if not HAS_GPU:
        assert call() == -5 and b"no HIP device" in L.nq_last_error(None)


def test_generator_reproduces_the_committed_tables_byte_for_byte(tmp_path):
    out = tmp_path / "nq_hdr_luts.inc"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_hdr_luts.py"), str(out)], check=True, capture_output=True)
    assert out.read_bytes() == open(os.path.join(ROOT, "include", "nq_hdr_luts.inc"), "rb").read()


def test_table_landmarks_monotonicity_and_gamut_rows():
    T = Y.TABLES
    assert [T[k].size for k in ("NQ_HDR_E_PQ", "NQ_HDR_E_HLG", "NQ_HDR_O_PQ", "NQ_HDR_O_HLG")] == [4096, 4096, 1280, 1280]
    for t in T.values():
        assert (np.diff(t) >= 0).all() and t[0] == 0
    epq, ehlg = T["NQ_HDR_E_PQ"], T["NQ_HDR_E_HLG"]
    assert epq[2048] == 3727 and int(np.argmax(epq == 65535)) == 3296 and (epq[3296:] == 65535).all()
    assert ehlg[2048] == 2578 and abs(int(ehlg[3071]) - 8192) <= 4 and ehlg[4095] == 30918
    white = Y.index(np.array([8192]))[0]
    grey = Y.index(np.array([int(round(0.18 * 8192))]))[0]
    assert (T["NQ_HDR_O_PQ"][white], T["NQ_HDR_O_HLG"][white]) == (189, 193)
    assert (T["NQ_HDR_O_PQ"][grey], T["NQ_HDR_O_HLG"][grey]) == (109, 110)
    assert T["NQ_HDR_O_PQ"][Y.index(np.array([65535]))[0]] == 255 and T["NQ_HDR_O_HLG"][Y.index(np.array([30918]))[0]] == 255
    assert all(sum(row) == 4096 for row in Y.GAMUT)
    # the index: the identity below 256, 128 buckets per power of two, 1279 at the top, never decreasing
    idx = Y.index(np.arange(65536))
    assert (idx[:256] == np.arange(256)).all() and idx[256] == 256 and idx[511] == 383 and idx[512] == 384 and idx[65535] == 1279
    assert (np.diff(idx) >= 0).all() and (np.diff(idx) <= 1).all()
    # the header carries the gamut rows
    assert re.search(r"r: \(6801, -2407, -298\)\s+g: \(-510, 4640, -34\)\s+b: \(-75, -412, 4583\)", _header())


def test_coefficients_are_the_rounded_rationals_and_the_headers_table():
    section = _header()
    section = section[section.index("10-bit YUV input: 10-bit"):]
    for m, mname in ((0, "601"), (Y.BT709, "709"), (Y.BT2020, "2020")):
        for full in (False, True):
            flags = m | (Y.FULL_RANGE if full else 0)
            es, yo = Y.rationals(flags)
            got, yo2 = Y.coefficients(flags)
            assert yo == yo2 == (0 if full else 64)
            for e, c in zip(es, got):
                assert isinstance(e, Fraction) and Fraction(c) <= 16384 * e + Fraction(1, 2) < Fraction(c + 1)
            assert got == Y.HEADER_TABLE[(m, full)], flags
            row = re.search(r"%s %s\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)" % (mname, "full" if full else "limited"), section)
            assert row and tuple(int(v) for v in row.groups()) == got, (mname, full)
    # the issue's rows
    assert Y.HEADER_TABLE[(Y.BT2020, False)] == (76590, 110418, 12322, 42783, 140879) and Y.HEADER_TABLE[(Y.BT709, True)] == (65584, 103282, 12285, 30701, 121698)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "%s-%d" % (m[1], m[0]))
def test_neutral_input_stays_neutral(mode):
    flags = mode[0]
    v = np.arange(1024)
    mid = np.full(1024, 512)
    r, g, b = Y.pixel(v, mid, mid, flags)
    assert (r == g).all() and (g == b).all() and (np.diff(r) >= 0).all()
    assert r[0] == 0 and r[1023] == 255
    if not flags & Y.FULL_RANGE:
        assert (r[:65] == 0).all()
        if mode[1] == "sdr":
            assert r[940] == 255


@pytest.mark.parametrize("flags", [m | r for m in MATRICES for r in (0, Y.FULL_RANGE)])
def test_sdr_is_within_one_level_of_the_exact_formula(flags):
    """All 1024 Y x 256 seeded chroma pairs (the corners among them).  The share of triples that differ at all is capped so that "within
    1" cannot hide a wrong coefficient: the 12-bit intermediate lies within a step (half a step of rounding, the rest the coefficients'
    own rounding) of the real value, and a level changes only where the real value lies that close to one of the 255 boundaries, which
    are 4095 / 255 = 16.06 steps apart: at most 1 / 16 of the triples."""
    rng = np.random.default_rng(16)
    pairs = np.concatenate([np.array([(a, b) for a in (0, 512, 1023) for b in (0, 512, 1023)]), rng.integers(0, 1024, (247, 2))])
    Yv = np.broadcast_to(np.arange(1024)[None, :], (256, 1024))
    U, V = (np.broadcast_to(pairs[:, k:k + 1], (256, 1024)) for k in (0, 1))
    got, want = Y.pixel(Yv, U, V, flags), Y.exact(Yv, U, V, flags)
    worst = max(int(np.abs(g - w).max()) for g, w in zip(got, want))
    share = [float((g != w).mean()) for g, w in zip(got, want)]
    print("flags %d: worst %d, share of differing triples R %.2e G %.2e B %.2e" % ((flags, worst) + tuple(share)))
    assert worst <= 1
    assert max(share) <= 1.0 / 16.0, share


# The largest distance, in 8-bit levels, between the integer pipeline and the float64 statement of it on the grid frame, measured on the
# CPU and rounded up to the next whole level: PQ limited 5.28, PQ full 11.47, HLG limited 3.02, HLG full 2.16.  The
# distance comes from the 12-bit signal in front of E: half a step of it is up to 0.4 % of linear light at the top of the PQ curve, the
# gamut rows carry that into a channel that is almost black (a saturated colour outside BT.709), and there one level is 0.03 % of white.
HDR_BOUND = {Y.BT2020 | Y.PQ: 6, Y.BT2020 | Y.PQ | Y.FULL_RANGE: 12, Y.BT2020 | Y.HLG: 4, Y.BT2020 | Y.HLG | Y.FULL_RANGE: 3}


@pytest.mark.parametrize("flags", sorted(HDR_BOUND))
def test_hdr_restatement_against_the_float64_pipeline_on_the_grid_frame(flags):
    pairs = Y.grid_chroma()
    assert len(pairs) == 64 and pairs[:9] == [(a, b) for a in (0, 512, 1023) for b in (0, 512, 1023)]
    Yv = np.broadcast_to(np.arange(1024)[None, :], (64, 1024))
    U, V = (np.broadcast_to(np.array([p[k] for p in pairs])[:, None], (64, 1024)) for k in (0, 1))
    got, real = Y.pixel(Yv, U, V, flags), Y.exact(Yv, U, V, flags, rounded=False)
    dist = [np.abs(g - r) for g, r in zip(got, real)]
    worst = max(float(d.max()) for d in dist)
    print("flags %d: worst %.2f levels, mean %.3f, share beyond one level %.2e" % (flags, worst, float(np.mean(dist)), float(np.mean(np.stack(dist) > 1.0))))
    grey = max(float(np.abs(g[4] - r[4]).max()) for g, r in zip(got, real))
    print("flags %d: on the grey axis (row %s) worst %.2f levels" % (flags, pairs[4], grey))
    assert worst <= HDR_BOUND[flags]


@pytest.mark.parametrize("name", ["PQ", "HLG"])
def test_bucketed_tone_table_against_the_unbucketed_curve(name):
    E, O = Y.TABLES["NQ_HDR_E_" + name], Y.TABLES["NQ_HDR_O_" + name]
    p = 65535.0 / 8192.0 if name == "PQ" else float(Y.TABLES["NQ_HDR_E_HLG"][4095]) / 8192.0
    l = np.arange(65536)
    real = 255.0 * Y.srgb_encode(Y.tone(l / 8192.0, p))
    worst = float(np.abs(O[Y.index(l)] - real).max())
    print("%s: the bucketed table is within %.4f of a level of the curve" % (name, worst))
    assert worst <= 0.68


def test_samples_ignore_the_other_six_bits_and_the_word_layout():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 1024, 4096)
    junk = rng.integers(0, 64, 4096)
    assert (Y.samples(s << 6 | junk, Y.MSB) == s).all() and (Y.samples(junk << 10 | s, 0) == s).all()
    # the word: alpha 255, channels at shifts 16, 8, 0; the chroma sample of pixel (x, y) is (x >> 1, y >> 1)
    y = np.full((3, 5), 512, np.uint16)
    u = np.array([[512, 512, 512], [1023, 512, 512]], np.uint16)
    v = np.full((2, 3), 512, np.uint16)
    got = Y.convert_one(y, u, v, Y.FULL_RANGE).view(np.uint32)
    assert (got >> 24 == 255).all()
    blue = got & 255
    assert (blue[:2] == 128).all() and (blue[2, :2] == 255).all() and (blue[2, 2:] == 128).all()


@pytest.mark.parametrize("layout", ["p010", "p010_vu", "i010", "yv12_10"])
@pytest.mark.parametrize("size", [(7, 5), (8, 4), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_yuv16_planes_returns_views_with_the_layouts_strides(nq, layout, size):
    w, h = size
    cw2, ch2 = (w + 1) // 2, (h + 1) // 2
    inter = layout.startswith("p010")
    for pad in (0, 6):                                                  # tight rows, and Android's byte strides with padding
        ys, cs = 2 * w + pad, (4 if inter else 2) * cw2 + pad
        words = (h * ys + (1 if inter else 2) * ch2 * cs) // 2
        buf = np.arange(words, dtype=np.uint16)
        y, u, v = nq.yuv16_planes(buf, w, h, layout, ys if pad else None, cs if pad else None)
        assert y.shape == (h, w) and u.shape == v.shape == (ch2, cw2) and all(p.dtype == np.uint16 and np.shares_memory(p, buf) for p in (y, u, v))
        base, c0 = buf.ctypes.data, h * ys
        assert y.ctypes.data == base and y.strides == (ys, 2)
        off = {"p010": (0, 2), "p010_vu": (2, 0), "i010": (0, ch2 * cs), "yv12_10": (ch2 * cs, 0)}[layout]
        assert (u.ctypes.data - base - c0, v.ctypes.data - base - c0) == off
        assert u.strides == v.strides == (cs, 4 if inter else 2)
        # a byte buffer is taken as well
        y8 = nq.yuv16_planes(buf.view(np.uint8), w, h, layout, ys if pad else None, cs if pad else None)[0]
        assert y8.ctypes.data == base and (y8 == y).all()


@pytest.mark.parametrize("layout", ["p010", "p010_vu", "i010", "yv12_10"])
def test_yuv16_planes_takes_a_buffer_that_ends_with_its_last_sample(nq, layout):
    """Android's buffers end at (rows - 1) * stride + row bytes: the padding behind the last row may be missing, wholly or in part; one
    sample less, or one more than the full stride, is refused."""
    w, h, pad = 7, 5, 6
    cw2, ch2 = 4, 3
    inter = layout.startswith("p010")
    ys, cs = 2 * w + pad, (4 if inter else 2) * cw2 + pad
    full = (h * ys + (1 if inter else 2) * ch2 * cs) // 2
    buf = np.arange(full + 1, dtype=np.uint16)
    want = nq.yuv16_planes(buf[:full], w, h, layout, ys, cs)
    for cut in (pad // 2, 1):
        got = nq.yuv16_planes(buf[:full - cut], w, h, layout, ys, cs)
        assert all(g.shape == r.shape and g.strides == r.strides and g.ctypes.data == r.ctypes.data and (g == r).all() for g, r in zip(got, want))
    last = max(int(p.max()) for p in want)
    assert last == full - pad // 2 - 1                                  # the views end with the last sample that must be there
    for size in (full - pad // 2 - 1, full + 1):
        with pytest.raises(ValueError):
            nq.yuv16_planes(buf[:size], w, h, layout, ys, cs)


def test_yuv16_planes_argument_errors(nq):
    buf = np.zeros(7 * 5 + 2 * 4 * 3, np.uint16)
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf, 7, 5, "nv12")
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf[:-1], 7, 5, "p010")
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf, 0, 5, "p010")
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf, 7, 5, "p010", 15, 16)                      # an odd byte stride
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf, 7, 5, "i010", 14, 7)
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf, 7, 5, "p010", 12, 16)                      # shorter than a row
    with pytest.raises(ValueError):
        nq.yuv16_planes(buf.view(np.uint8)[1:-1], 7, 5, "p010")         # an odd address
    with pytest.raises(TypeError):
        nq.yuv16_planes(buf.astype(np.int32), 7, 5, "p010")
    with pytest.raises(TypeError):
        nq.yuv16_planes(np.zeros(2 * buf.size, np.uint16)[::2], 7, 5, "p010")


def test_python_argument_errors_need_no_device(nq):
    from nquant.android_amd import yuv16 as M
    y, u, v = Y.random_planes(7, 5, 1)
    for bad in ([], [(y, u)], [y], [(y.astype(np.uint8), u, v)], [(y, u[:, :2], v)], [(y, u, v), (y[:4], u, v)], [(y.reshape(-1), u, v)]):
        with pytest.raises((ValueError, TypeError)):
            M._host_frames(bad)
    # views that one set of strides describes are passed as they are; anything else is copied tight
    buf = np.zeros(7 * 5 + 2 * 4 * 3, np.uint16)
    planes, w, h, ys, cs, step = M._host_frames([nq.yuv16_planes(buf, 7, 5, "p010")])
    assert (w, h, ys, cs, step) == (7, 5, 7, 8, 2) and all(np.shares_memory(p, buf) for p in planes[0])
    planes, w, h, ys, cs, step = M._host_frames([(y, u, v)])
    assert (ys, cs, step) == (7, 4, 1) and planes[0][0] is y
    planes, w, h, ys, cs, step = M._host_frames([(y, u, v), nq.yuv16_planes(buf, 7, 5, "p010")])     # two layouts in one call
    assert (ys, cs, step) == (7, 4, 1) and not np.shares_memory(planes[1][1], buf)
    planes, w, h, ys, cs, step = M._host_frames([(y[::-1], u, v)])                                    # a negative stride
    assert (ys, cs, step) == (7, 4, 1) and (planes[0][0] == y[::-1]).all()
    # the keywords
    assert M._flags() == Y.BT709 | Y.MSB and M._flags(transfer="pq") == Y.BT2020 | Y.PQ | Y.MSB
    assert M._flags("bt601", True, "hlg", False) == Y.FULL_RANGE | Y.HLG and M._flags("bt2020", msb=False) == Y.BT2020
    assert M._yuv16_keyword({}) == Y.BT709 | Y.MSB and M._yuv16_keyword({"transfer": "hlg", "full_range": True}) == Y.BT2020 | Y.HLG | Y.FULL_RANGE | Y.MSB
    for bad in ("pq", {"bt709": True}, 1):
        with pytest.raises(TypeError):
            M._yuv16_keyword(bad)
    for bad in ({"transfer": "gamma"}, {"matrix": "bt2100"}):
        with pytest.raises(ValueError):
            M._yuv16_keyword(bad)
    with pytest.raises(TypeError):
        nq.convert_frames_to_gif(1, [(y, u, v)], 16, True, yuv={}, yuv16={})                          # exclusive
    with pytest.raises(ValueError):
        nq.frames_from_yuv16([(y, u, v)], orient=9)
    with pytest.raises(ValueError):
        nq.frames_from_yuv16_device([], [], [], 4, 4, 4, 2, 1, [])
    with pytest.raises(ValueError):
        nq.resample_frames_yuv16_device([], [], [], 4, 4, 4, 2, 1, [], (2, 2))


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_without_a_device_every_call_raises_no_device(nq):
    frames = [Y.random_planes(8, 4, 2)]
    calls = [lambda: nq.frames_from_yuv16(frames), lambda: nq.resample_frames_yuv16(frames, (4, 2), transfer="pq"),
             lambda: nq.convert_frames_to_gif(1, frames, 16, True, yuv16={}),
             lambda: nq.convert_frames_to_apng(1, frames, 16, True, size=(4, 2), yuv16={"transfer": "hlg"}),
             lambda: nq.convert_frames_ordered(1, frames, 16, 8, yuv16={})]
    for call in calls:
        with pytest.raises(nq.NqError) as e:
            call()
        assert e.value.status == -5


def test_the_overlap_sweep_from_both_sides(nq):
    """The host-side sweep of nq_frames_from_yuv16 at its edges, on 8 x 4 P010 planes in one arena: what it allows passes every check
    (0 with a GPU, -5 without: the checks come before any device is touched) and what it refuses is -1 with the sweep's own text.
    Plane pointers are 2-byte and outputs 4-byte aligned, so the narrowest overlap an output can have with a plane is one sample."""
    import ctypes as C
    L = nq.load_library()
    arena = np.zeros(2048, np.uint8)
    base = (arena.ctypes.data + 15) & ~15
    Y0, U0, OUT = base + 512, base + 768, 8 * 4 * 4    # y spans 64 bytes (stride 8); u, v = u + 2 span 30 bytes each: chroma ends at U0 + 32
    arr = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)

    def call(dst, y=(Y0,), u=(U0,), ys=8, form="host"):
        n = len(dst)
        y, u = y * n if len(y) == 1 else y, u * n if len(u) == 1 else u
        tail = (n, arr(y), arr(u), arr([p + 2 for p in u]), 8, 4, ys, 8, 2, Y.MSB, arr(dst))
        return L.nq_frames_from_yuv16(0, *tail) if form == "host" else L.nq_frames_from_yuv16_device(0, None, *tail)

    allowed = [dict(dst=(U0 + 32,)),                         # begins at the last byte + 1 of the chroma span
               dict(dst=(Y0 + 64,)),                         # ... of the luma plane
               dict(dst=(Y0 - OUT,)),                        # ends where the luma plane begins
               dict(dst=(base,), u=(Y0 + 8,)),               # sources that overlap each other: the chroma inside the luma plane
               dict(dst=(base, base + OUT))]                 # two outputs, the second where the first ends (and one set of planes twice)
    refused = [dict(dst=(Y0 + 64,), y=(Y0 + 2,)),            # one sample into the end of the luma plane
               dict(dst=(U0 + 28,)),                         # one sample into the end of u's span, two into v's
               dict(dst=(Y0 + 64,), ys=40),                  # wholly inside a source: luma rows 40 samples apart span 256 bytes
               dict(dst=(U0 - 16,)),                         # a source wholly inside an output: the chroma span
               dict(dst=(base, base)),                       # two identical outputs
               dict(dst=(base, base + OUT - 4))]             # two outputs that share one word
    for kw in refused:
        for form in ("host", "device"):
            assert call(form=form, **kw) == -1 and b"an output overlaps a source plane or another output" in L.nq_last_error(None), (form, kw)
    assert not arena.any()
    for kw in allowed:
        assert call(**kw) == (0 if HAS_GPU else -5), (kw, L.nq_last_error(None))

