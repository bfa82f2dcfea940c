"""Palette refinement: k-means (Lloyd) passes over a palette on the GPU, and the squared error of a palette against the pixels
(nq_refine_palette / nq_refine_palette_device / nq_convert_frames_refined, include/nquant_abi.h "palette refinement").
A pass assigns every pixel with alpha != 0 to the nearest palette entry with alpha != 0 (squared ARGB distance, lowest index on a tie)
and moves every entry that got pixels to the rounded mean of their r, g, b; the alpha of an entry never changes.  The passes stop early
when an update changes nothing.  All sums are integers: the results are deterministic.  iterations=0 only measures.
There is no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from ._frames_in import _opened, _pre_steps
from .gif import _Handle
from .host import MODE_PARALLEL_TILED, _as_i32, _convert_frames_on, _frame_sizes


def _palette_io(palette):
    pal = np.array(np.asarray(palette).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32).reshape(-1)
    if pal.size < 1:
        raise ValueError("an empty palette")
    return pal


def _refine(L, handle, check, entry, ptrs, widths, heights, palette, iterations):
    """One nq_refine_palette* call.  Returns (palette as uint32, sse as iterations + 1 int64, counts as K int64, passes)."""
    n = len(ptrs)
    w, h = _frame_sizes(widths, heights, n)
    pal = _palette_io(palette)
    sse = np.zeros(max(int(iterations), 0) + 1, np.int64)
    counts = np.zeros(pal.size, np.int64)
    passes = C.c_int32(0)
    src = (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
    check(getattr(L, entry)(handle, n, src, w.ctypes.data, h.ctypes.data, pal.ctypes.data, int(pal.size), int(iterations), sse.ctypes.data,
                            counts.ctypes.data, C.byref(passes)))
    return pal, sse, counts, passes.value


def _host_frames(frames):
    frames = [np.ascontiguousarray(_as_i32(f)) for f in frames]
    if len(frames) == 0:
        raise ValueError("no frames")
    for f in frames:
        if f.ndim != 2:
            raise ValueError("every frame must be a 2-D (height, width) array")
    return frames


def refine_palette(frames, palette, iterations, device=0):
    """nq_refine_palette on host arrays: `frames` is a sequence of 2-D int32/uint32 ARGB_8888 arrays (sizes may differ), `palette` 1..256
    ARGB entries, iterations 0..64.  Returns (palette, sse, counts, passes): the refined palette (uint32), the squared error of every
    pass (iterations + 1 int64 values, non-increasing), the pixels per entry in the last assignment pass that ran, and how many ran."""
    frames = _host_frames(frames)
    hd = _Handle(device)
    try:
        return _refine(hd._L, hd._h, hd._check, "nq_refine_palette", [f.ctypes.data for f in frames], [f.shape[1] for f in frames],
                       [f.shape[0] for f in frames], palette, iterations)
    finally:
        hd.close()


def refine_palette_device(q, d_pixels, widths, heights, palette, iterations):
    """nq_refine_palette_device on the handle of quantizer `q`: d_pixels[i] is the HIP device address of frame i (widths[i] x heights[i]
    ARGB pixels, 4-byte aligned; 16-byte aligned frames take the fast path; never written).  Returns as refine_palette."""
    if len(d_pixels) == 0:
        raise ValueError("no frames")
    return _refine(q._L, q._h, q._check, "nq_refine_palette_device", list(d_pixels), widths, heights, palette, iterations)


def palette_error(frames, palette, device=0):
    """The summed squared ARGB distance of every pixel with alpha != 0 to its nearest palette entry: refine_palette with iterations=0."""
    return int(refine_palette(frames, palette, 0, device)[1][0])


def convert_frames_refined(kind, frames, nMaxColors, dither, refine, device=0, mode=MODE_PARALLEL_TILED, seeds=None, tile=None, size=None,
                           crop=None, linear_resample=True, yuv=None, orient=1, yuv16=None):
    """nq_convert_frames_refined on host arrays: convert_frames with `refine` (0..64) k-means passes on the shared palette, over the
    same frames, between the palette and the dither.  nMaxColors <= 256 unless refine is 0, which gives convert_frames' results.
    size / crop / linear_resample, yuv, orient and yuv16 say what `frames` are and what is done to them first: _frames_in.py.
    Returns (palette, [QuantizedImage per frame])."""
    frames, _, yuv, size, crop, orient = _pre_steps(frames, None, None, None, yuv, yuv16, size, crop, linear_resample, orient, device)
    if not 0 <= int(refine) <= 64:
        raise ValueError("refine must be 0..64, got %r" % (refine,))
    from .orient import _code as _orient_code
    orient = _orient_code(orient)
    with _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, mode, tile) as (q, frames):
        return _convert_frames_on(q, frames, nMaxColors, dither, mode, seeds, refine)
