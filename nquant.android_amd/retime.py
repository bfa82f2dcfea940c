"""Retime a frame sequence: timestamps in, blended frames and their delays out (nq_retime_plan / nq_retime_frames /
nq_retime_frames_device, include/nquant_abi.h "retiming"): the step between what a phone records -- 30, 60 or 120 frames per second at
a variable rate, one presentationTimeUs per frame -- and what a GIF shows, 10 to 20 frames per second on a centisecond grid.
retime_plan turns the timestamps into output frames, each the weighted mean of a window of source frames (exact overlap weights), and
into the delays_cs every encoder takes (they sum to the clip's length: no drift); retime_frames forms the means on the GPU, in linear
light, alpha premultiplied, with one rounding at the end.  The arithmetic is integer: tests/retime_ref.py restates it bit for bit.
The calls take no handle.  The frame converters (convert_frames_to_gif, convert_clip_to_gif, convert_frames_to_apng,
convert_frames_to_webp) take retime={"timestamps_us": ..., "period_us": ... or "fps": ..., "shutter_us": ..., "linear": ...} and then
retime the frames -- after the YUV, orient and reduce steps where those are asked for -- and supply the delays.
timestamps_from_pts and retime_plan are host arithmetic and need no device; the rest has no CPU fallback: without a HIP device every
call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import collections
import ctypes as C

import numpy as np

from ._frames_in import _arr, _reduced_on
from .host import NqError, _as_i32, load_library

RETIME_LINEAR = 1
RETIME_MAX_WINDOW = 64

RetimePlan = collections.namedtuple("RetimePlan", "m offset source weight delays_cs")


def timestamps_from_pts(pts_us, last_duration_us=None):
    """The n + 1 timestamps retime_plan takes, from the n presentation times of the frames (MediaCodec.BufferInfo.presentationTimeUs):
    frame i is on display until frame i + 1 begins, the last one for last_duration_us (None: as long as the frame before it; a single
    frame then needs the duration given).  Returns an int64 array."""
    pts = [int(v) for v in pts_us]
    if len(pts) == 0:
        raise ValueError("no frames")
    if last_duration_us is None:
        if len(pts) < 2:
            raise ValueError("timestamps_from_pts: one frame has no previous duration to repeat; pass last_duration_us")
        last_duration_us = pts[-1] - pts[-2]
    if int(last_duration_us) < 1:
        raise ValueError("timestamps_from_pts: the last duration must be at least 1 microsecond, got %r" % (last_duration_us,))
    return np.array(pts + [pts[-1] + int(last_duration_us)], np.int64)


def _check(L, rc, what):
    if rc != 0:
        raise NqError(rc, (L.nq_last_error(None) or b"").decode() or what)


def _period(period_us, fps):
    if (period_us is None) == (fps is None):
        raise ValueError("retime: give exactly one of period_us and fps")
    if fps is not None:
        if not fps > 0:
            raise ValueError("retime: fps must be positive, got %r" % (fps,))
        return int(round(1e6 / fps))
    return int(period_us)


def retime_plan(timestamps_us, period_us=None, fps=None, shutter_us=None):
    """nq_retime_plan (no device needed): timestamps_us are the n + 1 strictly increasing times in microseconds between which the n
    source frames are on display (timestamps_from_pts makes them); period_us, or fps (period = round(10^6 / fps)), the duration of an
    output frame; shutter_us (1 .. period; None: the period) the part of it that gathers light -- 1 picks the frame on display at the
    output's start.  Returns RetimePlan(m, offset, source, weight, delays_cs): output j is the mean of the frames
    source[offset[j] : offset[j + 1]] with the weights weight[...] (their overlap with the output's window, in microseconds), shown for
    delays_cs[j] hundredths of a second."""
    t = np.ascontiguousarray(np.asarray(timestamps_us, np.int64).reshape(-1))
    if t.size < 2:
        raise ValueError("retime_plan: n frames need n + 1 timestamps")
    period = _period(period_us, fps)
    shutter = period if shutter_us is None else int(shutter_us)
    L = load_library()
    n = int(t.size) - 1
    m, pairs = C.c_int32(0), C.c_int32(0)
    _check(L, L.nq_retime_plan(n, t.ctypes.data, period, shutter, 0, 0, C.byref(m), C.byref(pairs), None, None, None, None), "nq_retime_plan")
    offset = np.zeros(m.value + 1, np.int32)
    source = np.zeros(pairs.value, np.int32)
    weight = np.zeros(pairs.value, np.uint32)
    delays = np.zeros(m.value, np.int32)
    _check(L, L.nq_retime_plan(n, t.ctypes.data, period, shutter, m.value, pairs.value, C.byref(m), C.byref(pairs), offset.ctypes.data,
                               source.ctypes.data, weight.ctypes.data, delays.ctypes.data), "nq_retime_plan")
    return RetimePlan(int(m.value), offset, source, weight, delays)


def _plan_arrays(plan):
    """(m, offset, source, weight) of a RetimePlan or of any (m, offset, source, weight[, ...]) tuple, as contiguous arrays of the
    library's types.  The library checks the values."""
    m = int(plan[0])
    offset = np.ascontiguousarray(np.asarray(plan[1], np.int32).reshape(-1))
    source = np.ascontiguousarray(np.asarray(plan[2], np.int32).reshape(-1))
    weight = np.ascontiguousarray(np.asarray(plan[3], np.uint32).reshape(-1))
    if offset.size != m + 1 or source.size != weight.size or source.size < int(offset.max()):
        raise ValueError("retime: a plan needs m + 1 offsets and one weight per source, as many as the last offset says")
    return m, offset, source, weight


def _retime_host(frames, plan, linear, device):
    """nq_retime_frames of host frames with a plan.  Returns the m frames as a list of int32 arrays."""
    frames = [np.ascontiguousarray(_as_i32(f)) for f in frames]
    if len(frames) == 0:
        raise ValueError("no frames")
    if len({f.shape for f in frames}) != 1 or frames[0].ndim != 2:
        raise ValueError("retime: the frames must be 2-D arrays of one size, got %s" % sorted({f.shape for f in frames}))
    m, offset, source, weight = _plan_arrays(plan)
    height, width = frames[0].shape
    outs = [np.zeros((height, width), np.int32) for _ in range(max(m, 0))]
    L = load_library()
    _check(L, L.nq_retime_frames(int(device), len(frames), _arr([f.ctypes.data for f in frames]), width, height, m, offset.ctypes.data,
                                 source.ctypes.data, weight.ctypes.data, _arr([o.ctypes.data for o in outs]), RETIME_LINEAR if linear else 0),
           "nq_retime_frames")
    return outs


def retime_frames(frames, timestamps_us, period_us=None, fps=None, shutter_us=None, linear=True, device=0):
    """retime_plan followed by nq_retime_frames on host arrays: `frames` are the n 2-D int32/uint32 ARGB_8888 arrays of one size that
    timestamps_us (n + 1 values) times.  linear=True averages in linear light, False in stored values.  Returns (frames, delays_cs):
    the m output frames as int32 arrays and the delay of each, what the encoders and converters take as delays_cs."""
    frames = list(frames)
    t = np.asarray(timestamps_us, np.int64).reshape(-1)
    if t.size != len(frames) + 1:
        raise ValueError("retime: %d frames need %d timestamps, got %d" % (len(frames), len(frames) + 1, t.size))
    plan = retime_plan(t, period_us, fps, shutter_us)
    return _retime_host(frames, plan, linear, device), plan.delays_cs


def retime_frames_device(device, stream, d_src, d_dst, width, height, plan, linear=True):
    """nq_retime_frames_device: d_src[i] is the HIP device address of source frame i (width x height ARGB words, never written),
    d_dst[j] that of output j of `plan` -- a RetimePlan, or any (m, offset, source, weight) such as a crossfade: indices may repeat,
    weights may be 0, a window has 1..64 pairs.  4-byte aligned pointers; with every one 16-byte aligned the kernel moves 16 bytes per
    access.  Asynchronous on `stream` (a hipStream_t as an integer, 0 = the default stream) of `device`; allocates nothing."""
    m, offset, source, weight = _plan_arrays(plan)
    if len(d_src) == 0:
        raise ValueError("no frames")
    if len(d_dst) != m:
        raise ValueError("one output per frame of the plan")
    L = load_library()
    _check(L, L.nq_retime_frames_device(int(device), int(stream) or None, len(d_src), _arr(list(d_src)), int(width), int(height), m,
                                        offset.ctypes.data, source.ctypes.data, weight.ctypes.data, _arr(list(d_dst)),
                                        RETIME_LINEAR if linear else 0), "nq_retime_frames_device")


def _retime_keyword(retime):
    """The `retime` keyword of the converters: a dict with the keys timestamps_us (required) / period_us or fps / shutter_us / linear."""
    if not isinstance(retime, dict) or set(retime) - {"timestamps_us", "period_us", "fps", "shutter_us", "linear"} or "timestamps_us" not in retime:
        raise TypeError("retime is None or a dict with the keys timestamps_us / period_us or fps / shutter_us / linear, got %r" % (retime,))
    return retime


def _converter_frames(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient, device):
    """The `retime` keyword of the frame converters: (the ARGB frames the converter then runs on, their delays_cs).  The YUV, orient and
    reduce steps the converter was asked for run first, as the converter itself runs them, because the frames are small by then."""
    retime = _retime_keyword(retime)
    if delays_cs is not None:
        raise ValueError("retime supplies delays_cs: pass one of the two")
    if seeds is not None:
        raise ValueError("retime: seeds are given per frame, and the frames that are dithered are not the ones passed in")
    frames = list(frames)
    t = np.asarray(retime["timestamps_us"], np.int64).reshape(-1)
    if t.size != len(frames) + 1:
        raise ValueError("retime: %d frames need %d timestamps, got %d" % (len(frames), len(frames) + 1, t.size))
    plan = retime_plan(t, retime.get("period_us"), retime.get("fps"), retime.get("shutter_us"))
    from .orient import _code
    if yuv16 is not None:
        from .yuv16 import _converter_frames as _yuv16_frames
        frames = _yuv16_frames(frames, yuv, yuv16, size, crop, linear_resample, orient, device)
    elif yuv is not None or size is not None or crop is not None or _code(orient) != 1:
        from .gif import _Handle
        hd = _Handle(device)
        try:
            from .yuv import _yuv_keyword
            frames = _reduced_on(hd._L, hd._h, hd._check, frames, None if yuv is None else _yuv_keyword(yuv), size, crop, linear_resample,
                                 _code(orient))
        finally:
            hd.close()
    return _retime_host(frames, plan, retime.get("linear", True), device), plan.delays_cs
