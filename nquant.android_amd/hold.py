"""Temporal hold of palette indices over a frame sequence, on the GPU (nq_hold_frames / nq_hold_frames_device, include/nquant_abi.h
"temporal hold").  A pixel whose SOURCE colour stays within `threshold` (largest difference of the four 8-bit channels) of its anchor
keeps the palette index, and the ARGB output, it had in the frame before; the anchor moves only when the pixel is released.  It runs
between convert_frames and the delta GIF / APNG encoders and is what makes the still regions of real footage -- camera noise, a video
decoder's output -- repeat from frame to frame, which equal seeds alone do only for bit-identical pixels.  The trade: a held pixel does
not diffuse its quantisation error again.
There is no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from .gif import _Handle, _index_maps
from .host import _as_i32


def _threshold(threshold):
    if isinstance(threshold, bool) or int(threshold) != threshold or not 0 <= int(threshold) <= 255:
        raise ValueError("the hold threshold must be an integer in 0..255, got %r" % (threshold,))
    return int(threshold)


def _hold(L, handle, entry, src_ptrs, idx_ptrs, out_ptrs, width, height, threshold, check, counts=True):
    """One call of either form.  Returns the held counts (n int64 values), None when they are not wanted."""
    n = len(src_ptrs)
    if len(idx_ptrs) != n or (out_ptrs is not None and len(out_ptrs) != n):
        raise ValueError("one index map (and one output) per frame")
    arr = lambda ptrs: (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
    held = np.zeros(max(n, 1), np.int64) if counts else None
    check(getattr(L, entry)(handle, n, arr(src_ptrs), arr(idx_ptrs), arr(out_ptrs) if out_ptrs is not None else None, int(width), int(height),
                            int(threshold), held.ctypes.data if counts else None))
    return held[:n] if counts else None


def _hold_host(L, handle, check, frames, indices, outs, threshold):
    """nq_hold_frames on int32 frames; `indices` (uint16) and `outs` (int32, or None) are contiguous arrays of the caller's that are
    updated in place.  Returns the held counts."""
    height, width = frames[0].shape
    return _hold(L, handle, "nq_hold_frames", [f.ctypes.data for f in frames], [a.ctypes.data for a in indices],
                 None if outs is None else [o.ctypes.data for o in outs], width, height, threshold, check)


def hold_frames(frames, indices, threshold, out_argb=None, device=0):
    """nq_hold_frames on host arrays: `frames` the 2-D int32/uint32 ARGB_8888 source frames, `indices` their index maps (what
    convert_frames returned), out_argb (optional) their ARGB outputs; all of one size.  Nothing is modified: returns
    (held index maps, held counts), with out_argb (held index maps, held counts, held outputs).  held counts[i] = pixels of frame i that
    kept the index of frame i - 1 (counts[0] = 0)."""
    threshold = _threshold(threshold)
    frames = [np.ascontiguousarray(_as_i32(f)) for f in frames]
    maps = [a.copy() for a in _index_maps(indices)]
    outs = None if out_argb is None else [np.ascontiguousarray(_as_i32(o)).copy() for o in out_argb]
    if len(frames) == 0:
        raise ValueError("no frames")
    shapes = {a.shape for a in frames} | {a.shape for a in maps} | ({o.shape for o in outs} if outs is not None else set())
    if len(shapes) != 1 or len(frames[0].shape) != 2:
        raise ValueError("hold: frames, index maps and outputs must be 2-D arrays of one size, got %s" % sorted(shapes))
    if len(maps) != len(frames) or (outs is not None and len(outs) != len(frames)):
        raise ValueError("one index map (and one output) per frame")
    hd = _Handle(device)
    try:
        held = _hold_host(hd._L, hd._h, hd._check, frames, maps, outs, threshold)
    finally:
        hd.close()
    return (maps, held) if outs is None else (maps, held, outs)


def hold_frames_device(q, d_argb_ptrs, d_index_ptrs, width, height, threshold, d_out_argb_ptrs=None, counts=True):
    """nq_hold_frames_device on the handle of quantizer `q`: d_argb_ptrs[i], d_index_ptrs[i] and (optional) d_out_argb_ptrs[i] are the
    HIP device addresses of frame i's source pixels, uint16 index map and ARGB output (width x height; index maps 2-byte, pixels
    4-byte aligned; 16-byte aligned buffers take the fast path).  Index maps and outputs of frames 1.. are updated in place.  Returns
    the held counts; counts=False does not fetch them, returns None and leaves the work running on the handle's stream."""
    if len(d_argb_ptrs) == 0:
        raise ValueError("no frames")
    return _hold(q._L, q._h, "nq_hold_frames_device", list(d_argb_ptrs), list(d_index_ptrs),
                 None if d_out_argb_ptrs is None else list(d_out_argb_ptrs), width, height, _threshold(threshold), q._check, counts)
