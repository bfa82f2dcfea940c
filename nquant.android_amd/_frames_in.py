"""What the frame converters share (convert_frames_to_gif, convert_shots_to_gif, convert_clip_to_gif, convert_frames_to_apng,
convert_frames_to_webp, convert_frames_refined, convert_frames_ordered): the keywords that say what `frames` are and what happens to
them before the palette is made.  A converter calls _pre_steps first, runs its own checks, and opens its quantizer with _opened.

size / crop / linear_resample: with size=(width, height) or crop=(x, y, width, height) given, the frames (then all of one size) are
first cropped and area-averaged down to `size` (None: the crop's size) as resample_frames does it (resample.py; in linear light unless
linear_resample=False), and everything else runs on the result, on the same handle.
yuv (None: the frames are ARGB words): a dict with the keys bt709 / full_range says that `frames` are (y, u, v) tuples of 8-bit YUV
4:2:0 planes (yuv.py); they are converted -- with size or crop: converted and reduced in one kernel -- on the same handle.
orient (1: as they are): an orientation 1..8 (orient.py) turns / mirrors the frames first, on the same handle -- YUV frames in the
converting kernel --; size and crop are then those of the oriented frames.
yuv16 (None; exclusive with yuv): a dict with the keys matrix / full_range / transfer / msb says that `frames` are (y, u, v) tuples of
10-bit YUV 4:2:0 planes in 16-bit words (yuv16.py); they are converted -- with size or crop: converted and reduced in one kernel, with
orient: then turned -- before anything else runs.
retime (None: the frames are shown as they are; the converters that take delays_cs): a dict with the keys timestamps_us / period_us or
fps / shutter_us / linear (retime.py) blends the frames to that rate -- after the YUV, orient and reduce steps, which then run before
anything else -- and supplies delays_cs, which may not be given as well; seeds (one per frame) may not be given either.

_host_frames, _strides and _arr are what yuv.py and yuv16.py share for their host frames."""
import contextlib
import ctypes as C

import numpy as np

from .host import _frames_quantizer


def _pre_steps(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient, device):
    """The top of a converter: the retime step where `retime` is given, else the yuv16 step where `yuv16` is.  Returns (frames,
    delays_cs, yuv, size, crop, orient) with what the step consumed reset (a converter without retime / delays_cs passes None)."""
    if retime is not None:
        from .retime import _converter_frames
        frames, delays_cs = _converter_frames(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient, device)
        return frames, delays_cs, None, None, None, 1
    if yuv16 is not None:
        from .yuv16 import _converter_frames
        return _converter_frames(frames, yuv, yuv16, size, crop, linear_resample, orient, device), delays_cs, yuv, None, None, 1
    return frames, delays_cs, yuv, size, crop, orient


def _reduced_on(L, handle, check, frames, yuv_flags, size, crop, linear_resample, orient):
    """The ARGB frames a converter runs on, made on an open handle: yuv_flags None: `frames` are ARGB frames, reduced and oriented where
    size, crop or orient (a checked code) ask for it; else they are YUV frames with that flag word."""
    if yuv_flags is not None:
        from .yuv import _yuv_host
        return _yuv_host(L, handle, check, frames, size, crop, linear_resample, yuv_flags, orient)
    if size is not None or crop is not None or orient != 1:
        from .resample import _resample_host
        return _resample_host(L, handle, check, frames, size, crop, linear_resample, orient)
    return frames


@contextlib.contextmanager
def _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, mode, tile):
    """Opens the converter's quantizer of `kind` and makes its ARGB frames on that handle (orient: a checked code).  Yields (q, frames);
    q is closed on exit."""
    flags = None
    if yuv is None:
        frames, q = _frames_quantizer(kind, frames, device, mode, tile)
    else:
        from .yuv import _yuv_quantizer
        frames, q, flags = _yuv_quantizer(kind, frames, yuv, device, mode, tile)
    try:
        yield q, _reduced_on(q._L, q._h, q._check, frames, flags, size, crop, linear_resample, orient)
    finally:
        q.close()


def _arr(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[int(p) for p in ptrs])


def _strides(plane):
    """(row stride, element stride) of a 2-D view in bytes; a side of one sample leaves its stride open (None)."""
    return (plane.strides[0] if plane.shape[0] > 1 else None, plane.strides[1] if plane.shape[1] > 1 else None)


def _host_frames(frames, dtype, what):
    """(planes, width, height, y_stride, c_stride, c_step), strides and step in samples: `planes` a list of (y, u, v) arrays of `dtype`
    (uint8, or uint16 for the 10-bit formats; `what`: "yuv" or "yuv16") that stay alive for the call.  The views are passed as they are
    when one (y_stride, c_stride, c_step) describes all of them; otherwise they are copied tight."""
    s = np.dtype(dtype).itemsize
    shape_text = "a %s frame is a tuple (y, u, v) of 2-D %s arrays" % ({"yuv": "YUV", "yuv16": "10-bit YUV"}[what], np.dtype(dtype).name)
    frames = list(frames)
    if len(frames) == 0:
        raise ValueError("no frames")
    planes = []
    for f in frames:
        if not isinstance(f, (tuple, list)) or len(f) != 3:
            raise TypeError(shape_text)
        y, u, v = (np.asarray(p) for p in f)
        if any(p.dtype != dtype or p.ndim != 2 for p in (y, u, v)):
            raise TypeError(shape_text)
        planes.append((y, u, v))
    height, width = planes[0][0].shape
    if height < 1 or width < 1:
        raise ValueError("%s: empty frame" % what)
    cshape = ((height + 1) // 2, (width + 1) // 2)
    for y, u, v in planes:
        if y.shape != (height, width) or u.shape != cshape or v.shape != cshape:
            raise ValueError("%s: every frame needs y of shape %s and u, v of shape %s, got %s, %s, %s" % (
                what, (height, width), cshape, y.shape, u.shape, v.shape))

    def common(values, default, ok):
        """The one value every plane of `values` that fixes it agrees on (default: none fixes it), or None."""
        fixed = {v for v in values if v is not None}
        if len(fixed) > 1:
            return None
        value = fixed.pop() if fixed else default
        return value if ok(value) else None

    # in bytes: rows and steps must count whole samples (and, where a sample has 2 bytes, every plane begin at one)
    ys = [_strides(y) for y, _, _ in planes]
    cs = [_strides(p) for _, u, v in planes for p in (u, v)]
    y_step = common([t[1] for t in ys], s, lambda v: v == s)
    y_stride = common([t[0] for t in ys], s * width, lambda v: v % s == 0 and width <= v // s < 2**31)
    c_step = common([t[1] for t in cs], s, lambda v: v in (s, 2 * s))
    c_stride = None if c_step is None else common([t[0] for t in cs], c_step * (cshape[1] - 1) + s,
                                                  lambda v: v % s == 0 and c_step * (cshape[1] - 1) + s <= v < s * 2**31)
    aligned = s == 1 or all(p.ctypes.data % s == 0 for f in planes for p in f)
    if None in (y_step, y_stride, c_step, c_stride) or not aligned:
        planes = [tuple(np.ascontiguousarray(p) for p in f) for f in planes]
        y_stride, c_stride, c_step = s * width, s * cshape[1], s
    return planes, width, height, int(y_stride) // s, int(c_stride) // s, int(c_step) // s
