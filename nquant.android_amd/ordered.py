"""Ordered (positional) dither of frame sequences on the GPU (nq_dither_ordered / nq_dither_ordered_device / nq_convert_frames_ordered,
include/nquant_abi.h "ordered dither").  A pixel takes the nearest palette entry with alpha != 0 or, at a share of the positions of a
64 x 64 blue-noise mask that grows with how far it lies towards the second nearest one, that one -- provided the two entries differ by
no more than `limit` per channel.  The index depends on the pixel's colour, its coordinates and the palette only: unchanged pixels keep
their index from frame to frame without seeds, which is what the delta GIF and APNG encoders need.  limit=0 is the plain nearest entry.
A source pixel that moves by one level can still flip an index near a threshold: noisy footage still wants the temporal hold (hold.py).
There is no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from ._frames_in import _opened, _pre_steps
from .gif import _Handle
from .host import MODE_PARALLEL_TILED, QuantizedImage, _convert_frames_on, _frame_sizes
from .refine import _host_frames, _palette_io


def _limit(limit):
    if isinstance(limit, (bool, np.bool_)):
        raise TypeError("limit is an integer 0..255")
    return int(limit)


def _dither(L, handle, check, entry, src_ptrs, widths, heights, palette, limit, idx_ptrs, out_ptrs, return_stats):
    """One nq_dither_ordered* call.  Returns the statistics as an (n, 2) int64 array, or None."""
    n = len(src_ptrs)
    w, h = _frame_sizes(widths, heights, n)
    pal = _palette_io(palette)
    arr = lambda ptrs: (C.c_void_p * max(n, 1))(*[int(p) or None for p in ptrs])
    stats = np.zeros((n, 2), np.int64) if return_stats else None
    check(getattr(L, entry)(handle, n, arr(src_ptrs), w.ctypes.data, h.ctypes.data, pal.ctypes.data, int(pal.size), _limit(limit),
                            None if out_ptrs is None else arr(out_ptrs), arr(idx_ptrs), None if stats is None else stats.ctypes.data))
    return stats


def dither_ordered(frames, palette, limit, device=0, return_stats=False):
    """nq_dither_ordered on host arrays: `frames` is a sequence of 2-D int32/uint32 ARGB_8888 arrays (sizes may differ), `palette` 1..256
    ARGB entries, limit 0..255.  Returns [QuantizedImage per frame]; with return_stats=True ([QuantizedImage per frame], stats), stats an
    (n, 2) int64 array: per frame the counted pixels that took the second nearest entry, and the squared error of the counted pixels."""
    frames = _host_frames(frames)
    pal = _palette_io(palette)
    outs = [np.empty(f.shape, np.int32) for f in frames]
    idxs = [np.empty(f.shape, np.uint16) for f in frames]
    hd = _Handle(device)
    try:
        stats = _dither(hd._L, hd._h, hd._check, "nq_dither_ordered", [f.ctypes.data for f in frames], [f.shape[1] for f in frames],
                        [f.shape[0] for f in frames], pal, limit, [i.ctypes.data for i in idxs], [o.ctypes.data for o in outs], return_stats)
    finally:
        hd.close()
    images = [QuantizedImage(o, i, pal.view(np.int32)) for o, i in zip(outs, idxs)]
    return (images, stats) if return_stats else images


def dither_ordered_device(q, d_pixels, widths, heights, palette, limit, d_out_index, d_out_argb=None, return_stats=False):
    """nq_dither_ordered_device on the handle of quantizer `q`: d_pixels[i] is the HIP device address of frame i (widths[i] x heights[i]
    ARGB pixels, 4-byte aligned, never written), d_out_index[i] that of its uint16 index map (2-byte aligned), d_out_argb[i] (optional)
    that of its ARGB output.  16-byte aligned frames and outputs with 8-byte aligned index maps take the fast path.  Without
    return_stats the call is asynchronous on the handle's stream and returns None; with it, the (n, 2) statistics of dither_ordered."""
    if len(d_pixels) == 0:
        raise ValueError("no frames")
    if len(d_out_index) != len(d_pixels) or (d_out_argb is not None and len(d_out_argb) != len(d_pixels)):
        raise ValueError("one index map (and one output) per frame")
    return _dither(q._L, q._h, q._check, "nq_dither_ordered_device", list(d_pixels), widths, heights, palette, limit, list(d_out_index),
                   None if d_out_argb is None else list(d_out_argb), return_stats)


def convert_frames_ordered(kind, frames, nMaxColors, limit, refine=0, device=0, size=None, crop=None, linear_resample=True, yuv=None, orient=1, yuv16=None):
    """nq_convert_frames_ordered on host arrays: one shared palette for the frames (convert_frames' palette), `refine` (0..64) k-means
    passes on it over the same frames (refine.py), then the ordered dither with `limit` (0..255).  nMaxColors <= 256.
    size / crop / linear_resample, yuv, orient and yuv16 say what `frames` are and what is done to them first: _frames_in.py.
    Returns what convert_frames returns: (palette, [QuantizedImage per frame])."""
    frames, _, yuv, size, crop, orient = _pre_steps(frames, None, None, None, yuv, yuv16, size, crop, linear_resample, orient, device)
    if not 0 <= int(refine) <= 64:
        raise ValueError("refine must be 0..64, got %r" % (refine,))
    from .orient import _code as _orient_code
    orient = _orient_code(orient)
    with _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, MODE_PARALLEL_TILED, None) as (q, frames):
        return _convert_frames_on(q, frames, nMaxColors, False, MODE_PARALLEL_TILED, None, int(refine), _limit(limit))
