"""Crop and area-average a frame sequence down to the size of the file, on the GPU (nq_resample_frames / nq_resample_frames_device,
include/nquant_abi.h "frame reduction"): the step in front of the quantizer that camera or decoder output needs.  Averaging is in
linear light (linear=False: in stored values), alpha is premultiplied while averaging so that transparent pixels do not bleed colour,
and the arithmetic is integer throughout: the result is deterministic and tests/resample_ref.py restates it bit for bit.  This is a
reducer: a target larger than the crop is refused.  The frame converters (convert_frames_to_gif, convert_shots_to_gif,
convert_clip_to_gif, convert_frames_to_apng, convert_frames_refined) take size= and crop= and run it first, on their own handle.
fit_size is host arithmetic and needs no device; the rest has no CPU fallback: without a HIP device every call raises NqError with
status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from .gif import _Handle
from .host import _as_i32

RESAMPLE_LINEAR = 1


def fit_size(src_w, src_h, max_w, max_h):
    """The largest (w, h) with w <= max_w, h <= max_h, both >= 1, that keeps the aspect of src_w x src_h: the limiting side is scaled
    exactly, the other rounded to nearest (halves up).  Never enlarges: a source that fits is returned as it is."""
    src_w, src_h, max_w, max_h = int(src_w), int(src_h), int(max_w), int(max_h)
    if min(src_w, src_h, max_w, max_h) < 1:
        raise ValueError("fit_size: all four sides must be >= 1")
    if src_w <= max_w and src_h <= max_h:
        return src_w, src_h
    if max_w * src_h <= max_h * src_w:                  # the width limits: scale = max_w / src_w
        return max_w, min(max_h, max(1, (2 * src_h * max_w + src_w) // (2 * src_w)))
    return min(max_w, max(1, (2 * src_w * max_h + src_h) // (2 * src_h))), max_h


def _geometry(src_width, src_height, size, crop, orient=1):
    """(crop_x, crop_y, crop_w, crop_h, dst_w, dst_h) as ints: crop None is the whole frame -- with orient (a checked code of orient.py)
    the whole ORIENTED frame, in whose coordinates crop and size are given --, size None the crop's size.  The library checks the
    values."""
    if orient >= 5:
        src_width, src_height = src_height, src_width
    cx, cy, cw, ch = (0, 0, int(src_width), int(src_height)) if crop is None else (int(v) for v in crop)
    dw, dh = (cw, ch) if size is None else (int(v) for v in size)
    return cx, cy, cw, ch, dw, dh


def _resample(L, handle, check, entry, src_ptrs, src_width, src_height, dst_ptrs, geometry, linear, orient=1):
    """entry (nq_resample_frames or nq_resample_frames_device), or with orient != 1 its _oriented form."""
    n = len(src_ptrs)
    if len(dst_ptrs) != n:
        raise ValueError("one output per frame")
    arr = lambda ptrs: (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
    cx, cy, cw, ch, dw, dh = geometry
    if orient != 1:
        check(getattr(L, entry.replace("nq_resample_frames", "nq_resample_frames_oriented"))(
            handle, n, arr(src_ptrs), int(src_width), int(src_height), int(orient), cx, cy, cw, ch, arr(dst_ptrs), dw, dh,
            RESAMPLE_LINEAR if linear else 0))
        return
    check(getattr(L, entry)(handle, n, arr(src_ptrs), int(src_width), int(src_height), cx, cy, cw, ch, arr(dst_ptrs), dw, dh,
                            RESAMPLE_LINEAR if linear else 0))


def _resample_host(L, handle, check, frames, size, crop, linear, orient=1):
    """nq_resample_frames of host frames on an open handle; with orient != 1 (a checked code of orient.py) nq_resample_frames_oriented
    or, size and crop both None, nq_orient_frames.  Returns the resulting frames as a list of int32 arrays."""
    if orient != 1 and size is None and crop is None:
        from .orient import _orient_host
        return _orient_host(L, handle, check, frames, orient)
    frames = [np.ascontiguousarray(_as_i32(f)) for f in frames]
    if len(frames) == 0:
        raise ValueError("no frames")
    if len({f.shape for f in frames}) != 1 or frames[0].ndim != 2:
        raise ValueError("resample: the frames must be 2-D arrays of one size, got %s" % sorted({f.shape for f in frames}))
    height, width = frames[0].shape
    geometry = _geometry(width, height, size, crop, orient)
    if geometry[4] < 1 or geometry[5] < 1:
        raise ValueError("resample: the target must be at least 1 x 1, got %d x %d" % geometry[4:])
    outs = [np.zeros((geometry[5], geometry[4]), np.int32) for _ in frames]
    _resample(L, handle, check, "nq_resample_frames", [f.ctypes.data for f in frames], width, height, [o.ctypes.data for o in outs],
              geometry, linear, orient)
    return outs


def resample_frames(frames, size, crop=None, linear=True, device=0, orient=1):
    """nq_resample_frames on host arrays: `frames` are 2-D int32/uint32 ARGB_8888 arrays of one size, size = (width, height) of the
    result (None: the crop's), crop = (x, y, width, height) inside the frames (None: the whole frame).  linear=True averages in linear
    light, False in stored values.  orient (1..8, orient.py): the frames are oriented first, and size and crop are those of the oriented
    frames (nq_resample_frames_oriented).  Returns a list of int32 arrays of shape (height, width)."""
    from .orient import _code, oriented_size
    orient = _code(orient)
    frames = list(frames)
    if orient != 1 and size is None and crop is None and frames and np.ndim(frames[0]) == 2:
        crop = (0, 0) + oriented_size(*np.shape(frames[0])[::-1], orient)       # (not nq_orient_frames: this call zeroes a = 0 pixels)
    hd = _Handle(device)
    try:
        return _resample_host(hd._L, hd._h, hd._check, frames, size, crop, linear, orient)
    finally:
        hd.close()


def resample_frames_device(q, d_src_ptrs, src_width, src_height, d_dst_ptrs, size, crop=None, linear=True, orient=1):
    """nq_resample_frames_device on the handle of quantizer `q`: d_src_ptrs[i] is the HIP device address of frame i (src_width x
    src_height ARGB pixels, never written), d_dst_ptrs[i] that of its result (size[0] x size[1] pixels); 4-byte aligned, and when every
    source is 16-byte aligned and src_width a multiple of 4 the kernel reads 16 bytes per access.  The work is left running on the
    handle's stream.  size, crop, linear, orient as for resample_frames."""
    from .orient import _code
    orient = _code(orient)
    if len(d_src_ptrs) == 0:
        raise ValueError("no frames")
    _resample(q._L, q._h, q._check, "nq_resample_frames_device", list(d_src_ptrs), src_width, src_height, list(d_dst_ptrs),
              _geometry(src_width, src_height, size, crop, orient), linear, orient)
