"""CPU-side checks of the retiming (include/nquant_abi.h "retiming"): the interface (the three calls and the two constants in the header
and in the built library, none of the calls taking a handle, and the Python entry points), every refusal of the header before a device
is touched, nq_retime_plan against the restatement in retime_ref.py over a few hundred seeded variable-rate clips and its invariants
stated directly, and the restated mix -- what the GPU tests compare against -- against a float64 mean in linear light."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import retime_ref as R
from conftest import HAS_GPU, ROOT

SYMBOLS = ("nq_retime_plan", "nq_retime_frames_device", "nq_retime_frames")


def _header():
    return open(os.path.join(ROOT, "include", "nquant_abi.h")).read()


def test_symbols_are_declared_exported_and_take_no_handle(nq):
    L = nq.load_library()
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert name in nq.abi_symbols() and hasattr(L, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, name
        assert "nq_handle" not in m.group(1), name
        if name != "nq_retime_plan":
            assert re.match(r"\s*int\s+device\b", m.group(1)), name
            assert ("void* hip_stream" in m.group(1)) == name.endswith("_device"), name
            assert "const uint32_t* const*" in m.group(1) and re.search(r"(?<!const )uint32_t\* const\*", m.group(1)), name
    for flag, value in (("NQ_RETIME_LINEAR", 1), ("NQ_RETIME_MAX_WINDOW", 64)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), header), flag
    assert L.nq_abi_version() == 1
    for name in ("timestamps_from_pts", "retime_plan", "retime_frames", "retime_frames_device", "RetimePlan"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    assert nq.RetimePlan._fields == ("m", "offset", "source", "weight", "delays_cs")
    for fn in (nq.convert_frames_to_gif, nq.convert_clip_to_gif, nq.convert_shots_to_gif, nq.convert_frames_to_apng, nq.convert_frames_to_webp):
        assert inspect.signature(fn).parameters["retime"].default is None, fn.__name__
    p = inspect.signature(nq.retime_plan).parameters
    assert [p[k].default for k in ("period_us", "fps", "shutter_us")] == [None, None, None]
    assert inspect.signature(nq.retime_frames_device).parameters["linear"].default is True


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _plan_call(L, t, period, shutter, cap_m=0, cap_pairs=0, arrays=None, out=True):
    t = None if t is None else np.asarray(t, np.int64)
    m, pairs = C.c_int32(-7), C.c_int32(-7)
    a = arrays or (None, None, None, None)
    rc = L.nq_retime_plan(0 if t is None else t.size - 1, None if t is None else t.ctypes.data, period, shutter, cap_m, cap_pairs,
                          C.byref(m) if out else None, C.byref(pairs) if out else None, *[None if x is None else x.ctypes.data for x in a])
    return rc, m.value, pairs.value


def test_plan_refusals_leave_the_outputs_untouched(nq):
    L = nq.load_library()
    t = [0, 10000, 30000, 60000]
    bad = [dict(t=[5]), dict(t=None), dict(t=[0, 10000, 10000, 60000]), dict(t=[0, 10000, 9999, 60000]), dict(period=0), dict(period=-3), dict(shutter=0),
           dict(shutter=20001), dict(period=2**32, shutter=2**31), dict(t=[0, 2**33], period=1, shutter=1),
           dict(t=[-2**62, 2**62], period=2**30, shutter=1), dict(out=False)]
    for kw in bad:
        args = dict(t=t, period=20000, shutter=20000)
        args.update(kw)
        rc, m, pairs = _plan_call(L, args["t"], args["period"], args["shutter"], out=args.get("out", True))
        assert rc == -1 and (m, pairs) == (-7, -7), kw
        assert (L.nq_last_error(None) or b"") != b"", kw
    # counting; a cap that is too small writes the counts and nothing else; arrays that are needed and missing
    assert _plan_call(L, t, 20000, 20000) == (0, 3, 5)
    arrays = [np.full(6, -9, np.int32), np.full(8, -9, np.int32), np.full(8, 9, np.uint32), np.full(5, -9, np.int32)]
    for cap_m, cap_pairs in ((2, 8), (3, 4), (0, 0)):
        assert _plan_call(L, t, 20000, 20000, cap_m, cap_pairs, arrays) == (-1, 3, 5)
        assert all((a == a[0]).all() for a in arrays)
    assert _plan_call(L, t, 20000, 20000, 3, 5, (arrays[0], None, arrays[2], arrays[3])) == (-1, -7, -7)
    assert _plan_call(L, t, 20000, 20000, 4, 8, arrays) == (0, 3, 5)
    assert list(arrays[0][:4]) == [0, 2, 4, 5] and arrays[0][4] == -9 and list(arrays[1][:5]) == [0, 1, 1, 2, 2] and arrays[1][5] == -9
    assert list(arrays[2][:5]) == [10000] * 4 + [20000] and arrays[2][5] == 9 and list(arrays[3][:3]) == [2, 2, 2] and arrays[3][3] == -9
    # the largest shutter there is, and a clip that starts before zero
    assert _plan_call(L, [-2**40, 2**40], 2**40, 2**31 - 1) == (0, 2, 2)


def test_mix_refusals_come_before_any_device_is_touched(nq):
    """These hold with or without a GPU: the checks come first, and the text is the thread's handle-free one."""
    L = nq.load_library()
    w, h = 6, 4
    buf = np.full(5 * 32, -9, np.int32)                             # sources at 0 and 32, outputs at 64 and 96 (16-byte aligned)
    base = buf.ctypes.data
    arr = lambda ptrs: None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
    vec = lambda v, t: None if v is None else np.asarray(v, t)

    def call(device=0, n=2, w=w, h=h, m=2, offset=(0, 1, 3), source=(0, 0, 1), weight=(5, 1, 2), flags=1, src=(base, base + 128),
             dst=(base + 256, base + 384), form="host"):
        o, s, wt = vec(offset, np.int32), vec(source, np.int32), vec(weight, np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data
        if form == "host":
            return L.nq_retime_frames(device, n, arr(src), w, h, m, ptr(o), ptr(s), ptr(wt), arr(dst), flags)
        return L.nq_retime_frames_device(device, None, n, arr(src), w, h, m, ptr(o), ptr(s), ptr(wt), arr(dst), flags)

    long = dict(m=1, offset=(0, 65), source=(0,) * 65, weight=(1,) * 65, dst=(base + 256,))
    bad = [dict(n=0), dict(n=65536), dict(m=0), dict(m=65536), dict(w=0), dict(w=65536), dict(h=0), dict(h=65536),
           dict(n=40000, w=65535, h=1), dict(m=40000, w=65535, h=1), dict(flags=2), dict(flags=-1), dict(device=-1),
           dict(src=None), dict(dst=None), dict(offset=None), dict(source=None), dict(weight=None),
           dict(src=(base, None)), dict(dst=(None, base + 384)), dict(src=(base + 2, base + 128)), dict(dst=(base + 256, base + 385)),
           dict(offset=(1, 2, 3)), dict(offset=(0, 0, 3)), dict(offset=(0, 2, 1)), long,
           dict(source=(0, 2, 1)), dict(source=(0, -1, 1)), dict(weight=(0, 1, 2)), dict(weight=(5, 2**31 - 1, 1)), dict(weight=(5, 2**32 - 1, 2**32 - 1)),
           dict(dst=(base + 4, base + 384)), dict(dst=(base + 256, base + 256 + 4 * (w * h - 1))), dict(dst=(base + 128, base + 384))]
    for form in ("host", "device"):
        for kw in bad:
            assert call(form=form, **kw) == -1, (form, kw)
            assert (L.nq_last_error(None) or b"") != b"", (form, kw)
            assert (buf == -9).all(), (form, kw)
    # what is allowed: a weight of 0 beside others, repeated and unordered sources, two sources at one address, W = 2^31 - 1
    if not HAS_GPU:
        for kw in (dict(), dict(weight=(5, 0, 2)), dict(source=(1, 1, 0)), dict(src=(base, base)), dict(weight=(7, 2**31 - 2, 1)),
                   dict(m=1, offset=(0, 64), source=(0, 1) * 32, weight=(1,) * 64, dst=(base + 256,))):
            for form in ("host", "device"):
                assert call(form=form, **kw) == -5 and b"no HIP device" in L.nq_last_error(None), (form, kw)
        assert (buf == -9).all()


def test_the_overlap_sweep_from_both_sides(nq):
    """The host-side sweep of nq_retime_frames at its edges, on 4 x 2 frames (32 bytes) in one arena: what it allows passes every
    check (0 with a GPU, -5 without: the checks come before any device is touched) and what it refuses is -1 with the sweep's own
    text.  Every pointer is 4-byte aligned, so the narrowest overlap is one word; sources and outputs have one size, so a buffer
    that lies wholly inside another one coincides with it."""
    L = nq.load_library()
    arena = np.zeros(256, np.int32)
    base = (arena.ctypes.data + 15) & ~15
    S0, S1, D0, D1 = base + 256, base + 320, base + 512, base + 576
    arr = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)
    offset, source, weight = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1, 1], np.uint32)

    def call(src=(S0, S1), dst=(D0, D1), form="host"):
        tail = (2, arr(src), 4, 2, 2, offset.ctypes.data, source.ctypes.data, weight.ctypes.data, arr(dst), 1)
        return L.nq_retime_frames(0, *tail) if form == "host" else L.nq_retime_frames_device(0, None, *tail)

    allowed = [dict(dst=(S1 + 32, D1)),                      # begins at the last byte + 1 of a source
               dict(dst=(S0 - 32, D1)),                      # ends where a source begins
               dict(dst=(S0 - 32, S0 + 32), src=(S0, S0 + 64)),   # ... and both, with an output between two sources
               dict(src=(S0, S0 + 4)),                       # sources that overlap each other
               dict(src=(S0, S0)),                           # two sources that are one buffer
               dict(dst=(D0, D0 + 32))]                      # an output that begins where the other ends
    refused = [dict(dst=(S1 + 28, D1)),                      # one word into the end of a source
               dict(dst=(S0 - 28, D1)),                      # ... into its beginning
               dict(dst=(S0, D1)),                           # an output wholly inside a source, a source wholly inside an output
               dict(dst=(D0, S1)),
               dict(dst=(D0, D0)),                           # two identical outputs
               dict(dst=(D0, D0 + 28))]                      # two outputs that share one word
    for kw in refused:
        for form in ("host", "device"):
            assert call(form=form, **kw) == -1 and b"an output overlaps a source frame or another output" in L.nq_last_error(None), (form, kw)
    assert not arena.any()
    for kw in allowed:
        assert call(**kw) == (0 if HAS_GPU else -5), (kw, L.nq_last_error(None))


def test_python_argument_errors_need_no_device(nq):
    t = nq.timestamps_from_pts([0, 33333, 66667])
    assert t.dtype == np.int64 and list(t) == [0, 33333, 66667, 100001]
    assert list(nq.timestamps_from_pts([5], 40)) == [5, 45] and list(nq.timestamps_from_pts([0, 10], last_duration_us=3)) == [0, 10, 13]
    for bad in (lambda: nq.timestamps_from_pts([]), lambda: nq.timestamps_from_pts([5]), lambda: nq.timestamps_from_pts([0, 10], 0),
                lambda: nq.retime_plan(t), lambda: nq.retime_plan(t, 1000, 15), lambda: nq.retime_plan([0], 1000), lambda: nq.retime_plan(t, fps=0),
                lambda: nq.retime_frames([np.zeros((2, 2), np.int32)], t, fps=15),
                lambda: nq.retime_frames_device(0, 0, [], [1], 2, 2, (1, [0, 1], [0], [1])),
                lambda: nq.retime_frames_device(0, 0, [16], [32, 48], 2, 2, (1, [0, 1], [0], [1])),
                lambda: nq.retime_frames_device(0, 0, [16], [32], 2, 2, (1, [0, 2], [0], [1]))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(nq.NqError) as e:
        nq.retime_plan([0, 10, 10], 5)
    assert e.value.status == -1 and "t_us" in str(e.value)
    with pytest.raises(nq.NqError):
        nq.retime_plan(t, 1000, shutter_us=1001)
    assert nq.retime_plan(t, fps=15).m == 2 and nq.retime_plan(t, fps=30.0).m == 3
    # the converters' keyword
    frames = [np.zeros((4, 4), np.int32)] * 3
    rt = dict(timestamps_us=t, fps=15)
    for fn in (nq.convert_frames_to_gif, nq.convert_clip_to_gif, nq.convert_frames_to_apng, nq.convert_frames_to_webp):
        with pytest.raises(ValueError):
            fn(1, frames, 16, True, delays_cs=[4, 4, 4], retime=rt)
        with pytest.raises(ValueError):
            fn(1, frames, 16, True, seeds=[1, 2, 3], retime=rt)
        with pytest.raises(ValueError):
            fn(1, frames, 16, True, retime=dict(timestamps_us=t[:-1], fps=15))
        with pytest.raises(ValueError):
            fn(1, frames, 16, True, retime=dict(timestamps_us=t))
        for bad in (15, dict(fps=15), dict(timestamps_us=t, rate=15)):
            with pytest.raises(TypeError):
                fn(1, frames, 16, True, retime=bad)
    with pytest.raises(ValueError):
        nq.convert_shots_to_gif(1, frames, [0], 16, True, retime=rt)


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_without_a_device_every_call_raises_no_device(nq):
    frames = [R.random_argb(8, 4, i) for i in range(3)]
    t = [0, 30000, 70000, 100000]
    calls = [lambda: nq.retime_frames(frames, t, fps=15),
             lambda: nq.retime_frames_device(0, 0, [16, 1024, 2048], [4096], 8, 4, nq.retime_plan(t, 100000)),
             lambda: nq.convert_frames_to_gif(1, frames, 16, True, retime=dict(timestamps_us=t, fps=15)),
             lambda: nq.convert_frames_to_webp(1, frames, 16, True, size=(4, 2), retime=dict(timestamps_us=t, period_us=50000, shutter_us=1))]
    for call in calls:
        with pytest.raises(nq.NqError) as e:
            call()
        assert e.value.status == -5


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------------
def _plan_cases():
    """(timestamps, period, shutter): clips of 1..10 frames at scales from a microsecond to ten seconds per frame, durations varying by
    up to 30 : 1 inside a clip; periods below the shortest duration, at the median and above the longest; shutter 1, half, whole."""
    rng = np.random.default_rng(2024)
    cases = []
    for c in range(100):
        n = int(rng.integers(1, 11))
        hi = int(10 ** rng.uniform(0, 7))
        lo = max(1, hi // int(rng.integers(1, 31)))
        t = R.variable_timestamps(n, 100 + c, lo, hi)
        d = np.diff(t)
        for period in {max(1, int(d.min()) // 2), int(np.median(d)), int(d.max()) + int(rng.integers(1, 1 + int(d.max())))}:
            for shutter in {1, max(1, period // 2), period}:
                if shutter <= 2**31 - 1:
                    cases.append((t, period, shutter))
    # the extremes of a duration next to each other in one clip (1 us and 10 s), at a period that keeps m small
    cases.append(([7, 8, 10_000_008, 10_000_009, 20_000_009], 2_500_000, 2_500_000))
    cases.append(([7, 8, 10_000_008, 10_000_009, 20_000_009], 2_500_000, 1))
    return cases


def test_plan_equals_the_restatement_and_keeps_its_invariants(nq):
    cases = _plan_cases()
    assert len(cases) >= 300
    regimes = set()
    for t, period, shutter in cases:
        got = nq.retime_plan(t, period, shutter_us=shutter)
        m, offset, source, weight, delays = R.plan(t, period, shutter)
        what = (t, period, shutter)
        assert got.m == m and list(got.offset) == offset and list(got.source) == source and list(got.weight) == weight, what
        assert list(got.delays_cs) == delays, what
        assert got.offset.dtype == np.int32 and got.source.dtype == np.int32 and got.weight.dtype == np.uint32 and got.delays_cs.dtype == np.int32
        # the invariants, on the library's output
        n, D = len(t) - 1, t[-1] - t[0]
        assert (m - 1) * period < D and 2 * D < (2 * m + 1) * period, what
        assert got.offset[0] == 0 and len(got.source) == got.offset[-1] <= n + m - 1, what
        for j in range(m):
            k0, k1 = int(got.offset[j]), int(got.offset[j + 1])
            lo = t[0] + j * period
            assert k1 > k0 and (np.diff(got.source[k0:k1]) == 1).all() and (got.weight[k0:k1] >= 1).all(), what
            assert int(got.weight[k0:k1].astype(np.int64).sum()) == min(lo + shutter, t[-1]) - lo >= 1, what
            assert t[got.source[k0]] <= lo < t[got.source[k0] + 1], what                  # the first source is the one on display at o_j
            end = D if j == m - 1 else (j + 1) * period
            assert got.delays_cs[j] >= 0 and abs(10000 * int(got.delays_cs[j]) - (end - j * period)) <= 10000, what
        assert int(got.delays_cs.astype(np.int64).sum()) == R.cs(D), what
        if shutter == 1:
            assert (np.diff(got.offset) == 1).all() and (got.weight == 1).all(), what
        regimes.add((period < np.diff(t).min(), period > np.diff(t).max(), shutter == 1, shutter == period))
    assert len(regimes) >= 6, regimes


def test_fifteen_frames_per_second_gives_seven_six_seven(nq):
    """60 fps for two seconds to 15 fps: 66 667 us is 6.67 cs; the delays follow the rounded grid and do not drift."""
    t = [round(i * 1e6 / 60) for i in range(121)]
    plan = nq.retime_plan(t, fps=15)
    assert plan.m == 30 and list(plan.delays_cs[:6]) == [7, 6, 7, 7, 6, 7] and int(plan.delays_cs.sum()) == 200
    assert set(plan.delays_cs.tolist()) == {6, 7}
    assert (np.diff(plan.offset) >= 4).all() and (np.diff(plan.offset) <= 5).all()
    # shutter 1 at half the source's rate picks every other frame
    pick = nq.retime_plan(t, period_us=33334, shutter_us=1)
    assert pick.m == 60 and list(pick.source[:5]) == [0, 2, 4, 6, 8]
    # a period below every source duration repeats frames
    rep = nq.retime_plan([0, 40000, 80000], period_us=10000, shutter_us=1)
    assert rep.m == 8 and list(rep.source) == [0, 0, 0, 0, 1, 1, 1, 1] and list(rep.delays_cs) == [1] * 8


# ---------------------------------------------------------------------------------------------------------------------------------
# the restated mix
# ---------------------------------------------------------------------------------------------------------------------------------
def _srgb_decode(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def _srgb_encode(l):
    l = np.asarray(l, np.float64)
    return np.where(l <= 0.0031308, l * 12.92, 1.055 * np.maximum(l, 0.0) ** (1 / 2.4) - 0.055)


def _channels(argb):
    u = np.asarray(argb).view(np.uint32)
    return np.stack([(u >> 16) & 255, (u >> 8) & 255, u & 255], -1).astype(np.int64)


def test_restated_mix_is_within_one_level_of_the_float64_mean_in_linear_light():
    """decode, weighted mean, encode, round -- in float64, on opaque frames.  The margin is the two roundings involved (the table's and
    the result's), as for the frame reduction (tests/test_resample_cpu.py holds its restatement to the same bound)."""
    n, w, h = 9, 31, 17
    frames = [(R.random_argb(w, h, 40 + i).view(np.uint32) | np.uint32(0xFF000000)).view(np.int32) for i in range(n)]
    t = R.variable_timestamps(n, 77, 8000, 40000, start=0)
    for period, shutter in ((66667, 66667), (66667, 20000), (100000, 100000)):
        m, offset, source, weight, _ = R.plan(t, period, shutter)
        got = R.mix(frames, m, offset, source, weight, R.LINEAR)
        worst = 0
        for j in range(m):
            ks = range(offset[j], offset[j + 1])
            W = float(sum(weight[k] for k in ks))
            mean = sum(weight[k] / W * _srgb_decode(_channels(frames[source[k]]) / 255.0) for k in ks)
            want = np.floor(255.0 * _srgb_encode(mean) + 0.5).astype(np.int64)
            worst = max(worst, int(np.abs(_channels(got[j]) - want).max()))
            assert (got[j].view(np.uint32) >> 24 == 255).all()
        print("period %d shutter %d: max |restatement - float64 formula| = %d" % (period, shutter, worst))
        assert worst <= 1


@pytest.mark.parametrize("flags", [0, R.LINEAR])
def test_restated_mix_copies_a_window_that_lies_in_one_source(flags):
    frames = [R.random_argb(13, 7, 60 + i) for i in range(4)]
    t = [0, 40000, 80000, 120000, 160000]
    m, offset, source, weight, _ = R.plan(t, 40000, 1)
    assert source == [0, 1, 2, 3]
    for whole in (R.plan(t, 40000, 40000), (m, offset, source, weight), (2, [0, 1, 3], [2, 1, 1], [2**31 - 1, 3, 4])):
        got = R.mix(frames, *whole[:4], flags=flags)
        for j, g in enumerate(got):
            f = frames[whole[2][whole[1][j]]].view(np.uint32)
            assert (g.view(np.uint32) == np.where(f >> 24 == 0, 0, f)).all(), (flags, j)


def test_restated_mix_takes_no_colour_from_transparent_sources_and_holds_at_the_top_of_its_range():
    a = np.full((2, 3), 0x00FF8040, np.uint32).view(np.int32)      # transparent, with colour bits
    b = np.full((2, 3), 0xFF123456, np.uint32).view(np.int32)
    got = R.mix([a, b, a], 2, [0, 3, 5], [0, 1, 2, 0, 2], [1, 1, 2, 3, 4])
    assert (got[0].view(np.uint32) == 0x40123456).all()             # A = round(255 / 4) = 64
    assert (got[1] == 0).all()
    white = np.full((1, 5), 0xFFFFFFFF, np.uint32).view(np.int32)
    faint = np.full((1, 5), 0x01FFFFFF, np.uint32).view(np.int32)
    for flags in (0, R.LINEAR):
        assert (R.mix([white, white], 1, [0, 2], [0, 1], [2**30, 2**30 - 1], flags)[0].view(np.uint32) == 0xFFFFFFFF).all()
        assert (R.mix([faint, faint], 1, [0, 2], [0, 1], [2**30, 2**30 - 1], flags)[0].view(np.uint32) == 0x01FFFFFF).all()
