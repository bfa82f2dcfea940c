"""Animated PNG (APNG) files from the quantizer's index maps, encoded on the GPU (nq_encode_apng / nq_encode_apng_device,
include/nquant_abi.h "APNG encoding").  All frames have one size and share one palette of K <= 256 ARGB entries (what convert_frames
returns); every frame after the first stores only the bounding rectangle of the pixels that changed, and all 8 bits of a palette
entry's alpha are kept (tRNS), so an animation over a transparent background works -- which delta-mode GIF refuses.  An opaque palette
with K <= 255 marks the unchanged pixels inside a rectangle with a transparent index of its own; any other palette is cropped only
(the palettes convert_frames returns for opaque pictures hold alpha-254 entries, so they are cropped only).
As for delta GIF, static regions repeat from frame to frame only when the dither makes them repeat: MODE_PARALLEL_TILED with equal
seeds.  There is no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from ._frames_in import _opened, _pre_steps
from .gif import _Handle, _delays, _index_maps, _palette
from .hold import _hold_host, _threshold
from .host import MODE_PARALLEL_TILED, NqError, _convert_frames_on, _ordered_keyword, load_library


def _one_size(maps):
    shapes = {a.shape for a in maps}
    if len(shapes) != 1:
        raise ValueError("APNG: all frames must have one size, got %s" % sorted(shapes))
    return maps[0].shape


def apng_max_bytes(n, width, height, segment_bytes=0):
    """nq_apng_max_bytes: an upper bound of the file size for n frames of width x height (any content, any K; no device needed)."""
    out = C.c_int64(0)
    rc = load_library().nq_apng_max_bytes(int(n), int(width), int(height), int(segment_bytes), C.byref(out))
    if rc != 0:
        raise NqError(rc, "invalid APNG shape arguments")
    return out.value


def _encode(L, handle, entry, ptrs, width, height, palette, delays_cs, loop, segment_bytes, check):
    """Returns (file bytes, rectangles as an (n, 4) int32 array of x, y, w, h)."""
    n = len(ptrs)
    pal = _palette(palette)
    d = _delays(delays_cs, n)
    try:
        cap = apng_max_bytes(n, width, height, segment_bytes)
    except NqError:
        cap = 0                                     # (bad sizes: the encode call below says which)
    buf = np.empty(max(cap, 1), np.uint8)
    rects = np.zeros((max(n, 1), 4), np.int32)
    size = C.c_int64(0)
    src = (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
    check(getattr(L, entry)(handle, n, src, int(width), int(height), pal.ctypes.data, int(pal.size), d.ctypes.data if d is not None else None,
                            int(loop), int(segment_bytes), buf.ctypes.data, int(cap), C.byref(size), rects.ctypes.data))
    return buf[:size.value].tobytes(), rects[:n]


def encode_apng(frames, palette, delays_cs=None, loop=0, segment_bytes=0, device=0, return_rects=False):
    """nq_encode_apng: `frames` is one 2-D index map or a sequence of them, all of one size; `palette` the ARGB_8888 entries they index
    (K = len(palette) <= 256).  delays_cs: per-frame delay in hundredths of a second (None: 0); loop: how often the animation plays
    (0 = for ever); segment_bytes: bytes of a frame's raw stream per deflate chain (0 = 32768, at most 65535).  One frame gives
    encode_png's file.  Returns the file; with return_rects=True the pair (file, (n, 4) int32 array of every frame's x, y, w, h)."""
    maps = _index_maps(frames)
    height, width = _one_size(maps)
    hd = _Handle(device)
    try:
        data, rects = _encode(hd._L, hd._h, "nq_encode_apng", [a.ctypes.data for a in maps], width, height, palette, delays_cs, loop,
                              segment_bytes, hd._check)
    finally:
        hd.close()
    return (data, rects) if return_rects else data


def encode_apng_device(q, d_index_ptrs, width, height, palette, delays_cs=None, loop=0, segment_bytes=0, return_rects=False):
    """nq_encode_apng_device on the handle of quantizer `q`: d_index_ptrs[i] is the HIP device address of frame i's uint16 index map
    (width x height, 2-byte aligned; never written).  Arguments and result otherwise as encode_apng."""
    if len(d_index_ptrs) == 0:
        raise ValueError("no frames")
    data, rects = _encode(q._L, q._h, "nq_encode_apng_device", list(d_index_ptrs), width, height, palette, delays_cs, loop, segment_bytes,
                          q._check)
    return (data, rects) if return_rects else data


def write_apng(path, frames, palette, delays_cs=None, loop=0, segment_bytes=0, device=0):
    """encode_apng, written to `path`.  Returns the number of bytes written."""
    data = encode_apng(frames, palette, delays_cs, loop, segment_bytes, device)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def convert_frames_to_apng(kind, frames, nMaxColors, dither, delays_cs=None, loop=0, seeds=None, tile=None, segment_bytes=0, device=0,
                           mode=MODE_PARALLEL_TILED, return_rects=False, hold=None, refine=0, size=None, crop=None, linear_resample=True,
                           ordered=None, yuv=None, retime=None, orient=1, yuv16=None):
    """convert_frames (one shared palette for the ARGB frames, which must have one size) followed by encode_apng of the index maps on
    the same handle.  nMaxColors <= 256.  Seeds are passed on as given: regions that do not move repeat in the index maps, and so drop
    out of the file, when the frames are dithered with equal seeds in MODE_PARALLEL_TILED.  hold (None: no such pass): an integer
    0..255 runs the temporal hold (hold.py) with that threshold between the two steps, on the same handle, so that pixels whose source
    moved by no more than it keep their index (footage with sensor or codec noise); the index maps pass through host memory in between.
    refine (0..64): that many k-means passes on the palette over the frames before the dither (refine.py); 0 is the call without it.
    ordered (None: the error-diffusion dither): an integer 0..255 dithers the frames with the ordered dither (ordered.py) with that
    limit instead; dither, mode and tile then take no part, and seeds may not be given.
    size / crop / linear_resample, yuv, orient, yuv16 and retime say what `frames` are and what is done to them first: _frames_in.py.
    Returns (file bytes, palette); with return_rects=True (file bytes, palette, rectangles)."""
    frames, delays_cs, yuv, size, crop, orient = _pre_steps(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient,
                                                            device)
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("a PNG palette holds at most 256 entries")
    if yuv is None and len({np.asarray(f).shape for f in frames}) > 1:
        raise ValueError("APNG: all frames must have one size")
    ordered = _ordered_keyword(ordered, seeds)
    if hold is not None:
        hold = _threshold(hold)
    from .orient import _code as _orient_code
    orient = _orient_code(orient)
    with _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, mode, tile) as (q, frames):
        palette, outs = _convert_frames_on(q, frames, nMaxColors, dither, mode, seeds, int(refine) or None, ordered)
        maps = _index_maps([o.index for o in outs])
        height, width = _one_size(maps)
        if hold is not None:
            _hold_host(q._L, q._h, q._check, frames, maps, None, hold)
        data, rects = _encode(q._L, q._h, "nq_encode_apng", [a.ctypes.data for a in maps], width, height, palette, delays_cs, loop,
                              segment_bytes, q._check)
    return (data, palette, rects) if return_rects else (data, palette)
