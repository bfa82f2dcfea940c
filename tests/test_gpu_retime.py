"""GPU tests of the retiming (include/nquant_abi.h "retiming"; csrc/nq_retime.hip): every case is bit-exact against the restatement in
retime_ref.py, with guard words before, between and behind the outputs and the sources unchanged.  Geometry (one pixel, a tail, a
full block and a vector body with a 3-pixel tail) on both paths and in both table modes; windows at the in-flight depth and at the cap,
launch packing at both of its limits, repeated sources and weights of 0; the top of the 64-bit range; alpha; shutter 1; a caller's
stream behind the gate of stream_gate.py; the host form; the converters' keyword."""
import numpy as np
import pytest

import retime_ref as R
import stream_gate as G
from test_gpu_yuv import _Stream

pytestmark = pytest.mark.gpu

SENT = -9
_REF = {}


def _frames(w, h, n, seed=0):
    key = ("frames", w, h, n, seed)
    if key not in _REF:
        _REF[key] = [R.random_argb(w, h, 9000 + 100 * seed + 7 * w + h + i) for i in range(n)]
    return _REF[key]


def _want(key, frames, plan, flags):
    """The restatement of one case, computed once."""
    if key not in _REF:
        _REF[key] = R.mix(frames, *plan[:4], flags=flags)
    return _REF[key]


def _run(nq, frames, plan, linear, shift, stream=0):
    """The device form on the NULL stream (or `stream`) with sources and outputs `shift` words behind a 16-byte boundary.  Returns
    (the whole output buffer as read back, the _Stream of the outputs)."""
    import torch
    h, w = frames[0].shape
    src = _Stream(frames, shift, SENT)
    dst = _Stream([np.full((h, w), SENT, np.int32) for _ in range(plan[0])], shift, SENT)
    assert all(p % 16 == 4 * shift for p in src.ptrs + dst.ptrs)
    nq.retime_frames_device(0, stream, src.ptrs, dst.ptrs, w, h, plan, linear)
    torch.cuda.synchronize()
    assert (src.read() == src.host).all(), "a source was written"
    return dst.read(), dst


def _check(nq, key, frames, plan, flags=R.LINEAR, shifts=(0, 1)):
    want = _want(key, frames, plan, flags)
    for shift in shifts:
        got, dst = _run(nq, frames, plan, bool(flags & R.LINEAR), shift)
        bad = int((got != dst.expect(want)).sum())
        assert bad == 0, "%s at shift %d: %d words differ from the restatement (guards included)" % (key, shift, bad)
    return want


# a plan of the library over variable-rate timestamps: 7 sources, windows of 1 to 3 pairs with uneven weights
def _library_plan(nq, n):
    t = R.variable_timestamps(n, 31, 9000, 40000, start=0)
    return nq.retime_plan(t, period_us=45000)


@pytest.mark.parametrize("flags", [R.LINEAR, 0], ids=["linear", "stored"])
@pytest.mark.parametrize("size", [(1, 1), (3, 1), (5, 7), (64, 4), (79, 13)], ids=lambda s: "%dx%d" % s)
def test_geometry_on_both_paths_in_both_table_modes(nq, size, flags):
    """79 x 13 = 1027 pixels: a full block of 1024, whose vector body is followed by a 3-pixel tail in a second block.  The frames one
    word off alignment take the one-pixel path and must give the same words."""
    w, h = size
    frames = _frames(w, h, 7)
    plan = _library_plan(nq, 7)
    assert plan.m >= 3 and max(np.diff(plan.offset)) >= 2
    ref = R.plan(R.variable_timestamps(7, 31, 9000, 40000, start=0), 45000, 45000)
    assert (plan.m, list(plan.offset), list(plan.source), list(plan.weight)) == ref[:4]
    _check(nq, ("geometry", size, flags), frames, plan, flags)


@pytest.mark.parametrize("window", [1, 4, 5, 64])
def test_windows_at_the_in_flight_depth_and_at_the_cap(nq, window):
    w, h = 37, 5
    n = min(window, 9)
    frames = _frames(w, h, n, 1)
    rng = np.random.default_rng(window)
    source = rng.integers(0, n, window) if window > n else rng.permutation(n)[:window]
    weight = rng.integers(1, 100000, window)
    _check(nq, ("window", window), frames, (1, [0, window], source, weight))


def test_one_source_and_one_output(nq):
    frames = _frames(9, 3, 1, 2)
    want = _check(nq, "n1m1", frames, (1, [0, 1], [0], [3]))
    f = frames[0].view(np.uint32)
    assert (want[0].view(np.uint32) == np.where(f >> 24 == 0, 0, f)).all()


def test_launch_packing_at_both_limits(nq):
    """17 outputs of one pair each: the 17th opens a second launch.  5 outputs of 20 pairs each: the fourth would pass 64 pairs, so a
    launch takes three.  Then both at once: windows of 1, 64, 1, 63, 2 pairs."""
    w, h = 21, 3
    frames = _frames(w, h, 6, 3)
    rng = np.random.default_rng(17)
    _check(nq, "pack17", frames, (17, np.arange(18), rng.integers(0, 6, 17), rng.integers(1, 9, 17)))
    _check(nq, "pack5x20", frames, (5, 20 * np.arange(6), rng.integers(0, 6, 100), rng.integers(1, 1000, 100)))
    sizes = [1, 64, 1, 63, 2]
    total = sum(sizes)
    _check(nq, "packmixed", frames, (5, np.concatenate([[0], np.cumsum(sizes)]), rng.integers(0, 6, total), rng.integers(1, 1000, total)))


def test_repeated_sources_and_weights_of_zero(nq):
    frames = _frames(18, 4, 3, 4)
    plan = (3, [0, 3, 6, 8], [1, 1, 0, 2, 0, 1, 2, 2], [5, 7, 1, 0, 4, 0, 0, 9])
    want = _check(nq, "repeat0", frames, plan)
    f0, f2 = (frames[i].view(np.uint32) for i in (0, 2))
    assert (want[1].view(np.uint32) == np.where(f0 >> 24 == 0, 0, f0)).all()        # weights 0, 4, 0: a copy of source 0
    assert (want[2].view(np.uint32) == np.where(f2 >> 24 == 0, 0, f2)).all()


@pytest.mark.parametrize("word", [0xFFFFFFFF, 0x01FFFFFF], ids=["white", "faint"])
def test_the_top_of_the_range(nq, word):
    """W = 2^31 - 1 over two sources of one word: the sums are near 2^55 (white) and must give the word back."""
    frames = [np.full((3, 11), word, np.uint32).view(np.int32) for _ in range(2)]
    for flags in (R.LINEAR, 0):
        want = _check(nq, ("top", word, flags), frames, (1, [0, 2], [0, 1], [2**30, 2**30 - 1]), flags)
        assert (want[0].view(np.uint32) == word).all()


def test_large_weights_on_random_frames(nq):
    """Weights of 2^20 to 2^30 (three of a window stay below 2^31) over random words of every alpha: the divisions' operands at every
    magnitude up to the largest, with quotients that are not special.  The kernel divides through a float estimate that it corrects
    in integers; the restatement divides in integers."""
    w, h = 64, 16
    frames = _frames(w, h, 4, 7)
    rng = np.random.default_rng(23)
    weight = [int(2 ** rng.uniform(20, 29)) for _ in range(15)] + [2**30, 2**30 - 1]
    plan = (6, [0, 3, 6, 9, 12, 15, 17], list(rng.integers(0, 4, 15)) + [1, 2], weight)
    for flags in (R.LINEAR, 0):
        _check(nq, ("large", flags), frames, plan, flags)


def test_alpha(nq):
    w, h = 23, 3
    rng = np.random.default_rng(8)
    clear = [(rng.integers(0, 1 << 24, (h, w), dtype=np.int64)).astype(np.uint32).view(np.int32) for _ in range(3)]       # a = 0, colour bits set
    opaque = (rng.integers(0, 1 << 24, (h, w), dtype=np.int64).astype(np.uint32) | np.uint32(0xFF000000)).view(np.int32)
    partial = _frames(w, h, 3, 5)
    frames = clear + [opaque] + partial
    plan = (3, [0, 3, 7, 10], [0, 1, 2, 0, 1, 3, 2, 4, 5, 6], [1, 2, 3, 1, 1, 1, 1, 3, 5, 2])
    want = _check(nq, "alpha", frames, plan)
    assert (want[0] == 0).all()                                                     # all sources transparent
    assert (want[1].view(np.uint32) == (np.uint32(64 << 24) | (opaque.view(np.uint32) & np.uint32(0xFFFFFF)))).all()   # 255 / 4 -> 64, colour kept
    assert len(np.unique(want[2].view(np.uint32) >> 24)) > 8


def test_shutter_one_copies_the_picked_frames_and_a_short_period_repeats_them(nq):
    w, h = 15, 6
    frames = _frames(w, h, 6, 6)
    t = R.variable_timestamps(6, 5, 15000, 50000, start=0)
    copies = lambda i: np.where(frames[i].view(np.uint32) >> 24 == 0, 0, frames[i].view(np.uint32))
    for name, period in (("pick", 60000), ("repeat", 7000)):
        plan = nq.retime_plan(t, period_us=period, shutter_us=1)
        assert (np.diff(plan.offset) == 1).all()
        if name == "repeat":
            assert plan.m > 12 and (np.bincount(plan.source, minlength=6) >= 2).all()
        want = _check(nq, ("shutter1", name), frames, plan, shifts=(0,))
        for j in range(plan.m):
            assert (want[j].view(np.uint32) == copies(int(plan.source[j]))).all(), (name, j)


def test_on_a_callers_stream_the_call_returns_while_the_gate_runs(nq):
    """The protocol of stream_gate.py: the sources hold the poison until a copy behind the spin, on the caller's stream, makes them
    true; the call follows with no host wait, then the snapshot on the same stream.  The stream must still be busy when the call has
    returned, and the snapshot equals the restatement of the TRUE frames."""
    import torch
    stream = torch.cuda.Stream()
    cycles, _ = G.calibrate(stream)
    w, h, shift = G.WIDE
    frames = G.argb_frames(w, h, 5, 8100)
    plan = nq.retime_plan(R.variable_timestamps(5, 3, 10000, 30000, start=0), period_us=35000)
    assert plan.m >= 2
    want = _want("stream", frames, plan, R.LINEAR)
    gate = G.Gate(stream, cycles)
    src = gate.input("argb", frames, [G.invert_rgb(f) for f in frames], shift)
    dst = gate.output("out_argb", want, shift)
    for spin in (False, True):                                       # the first round loads the kernel; the second runs behind the gate
        gate.arm(spin)
        nq.retime_frames_device(0, stream.cuda_stream, src.ptrs, dst.ptrs, w, h, plan)
        gate.finish(spin, "retime_frames_device")
        gate.check(dst, want, "retime_frames_device")
        gate.check_inputs("retime_frames_device")
    torch.cuda.synchronize()


def test_host_form_equals_the_device_form(nq):
    for (w, h), linear in (((79, 13), True), ((5, 7), False)):
        frames = _frames(w, h, 7)
        keep = [f.copy() for f in frames]
        t = R.variable_timestamps(7, 31, 9000, 40000, start=0)
        before = nq.device_bytes()
        outs, delays = nq.retime_frames(frames, t, period_us=45000, linear=linear)
        assert nq.device_bytes() == before
        plan = nq.retime_plan(t, period_us=45000)
        got, dst = _run(nq, frames, plan, linear, 0)
        assert (got == dst.expect(outs)).all() and (delays == plan.delays_cs).all()
        assert all((f == k).all() for f, k in zip(frames, keep))
        want = _want(("geometry", (w, h), R.LINEAR if linear else 0), frames, plan, R.LINEAR if linear else 0)
        assert all((o == r).all() and o.dtype == np.int32 and o.shape == (h, w) for o, r in zip(outs, want))


def test_converters_with_retime_equal_retime_frames_followed_by_the_converter(nq):
    from nquant.android_amd import synth
    w, h, n = 64, 48, 8
    frames = [synth.gradient_noise(w, h, 300 + i // 2) for i in range(n)]
    t = nq.timestamps_from_pts([0, 16000, 34000, 50000, 67000, 83000, 100000, 117000])
    rt = dict(timestamps_us=t, fps=30)
    mixed, delays = nq.retime_frames(frames, t, fps=30)
    assert len(mixed) == 4 and int(delays.sum()) == 13
    got = nq.convert_frames_to_gif(1, frames, 32, True, hold=4, delta=True, retime=rt)
    want = nq.convert_frames_to_gif(1, mixed, 32, True, hold=4, delta=True, delays_cs=delays)
    assert got[0] == want[0] and (got[1] == want[1]).all()
    # with size= the reducer runs first, on the source frames
    small = nq.resample_frames(frames, (32, 24))
    mixed, delays = nq.retime_frames(small, t, period_us=50000, shutter_us=20000, linear=False)
    got = nq.convert_frames_to_webp(0, frames, 16, True, size=(32, 24), retime=dict(timestamps_us=t, period_us=50000, shutter_us=20000, linear=False))
    want = nq.convert_frames_to_webp(0, mixed, 16, True, delays_cs=delays)
    assert got[0] == want[0] and (got[1] == want[1]).all()
    assert got[0] != nq.convert_frames_to_webp(0, small[:len(mixed)], 16, True, delays_cs=delays)[0]
