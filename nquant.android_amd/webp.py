"""Lossless WebP files (VP8L) from the quantizer's index maps, encoded on the GPU (nq_encode_webp / nq_encode_webp_device,
include/nquant_abi.h "WebP encoding"): a still image from one map, an animation from several.  All frames have one size and share
one palette of K <= 256 ARGB entries (what convert_frames returns); with delta=True every frame after the first stores only the
bounding rectangle of the pixels that changed (left and top rounded down to even), which replaces what was there, so all 8 bits of a
palette entry's alpha work, alpha 0 included.  K <= 16 / 4 / 2 packs 2 / 4 / 8 indices into a pixel.
As for delta GIF and APNG, static regions repeat from frame to frame only when the dither makes them repeat: MODE_PARALLEL_TILED with
equal seeds.  The calls take no handle.  There is no CPU fallback: without a HIP device every call raises NqError with status -5
(NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from ._frames_in import _opened, _pre_steps
from .gif import _delays, _index_maps, _palette
from .hold import _hold_host, _threshold
from .host import (MODE_PARALLEL_TILED, NQ_KIND_LAB, NqError, PnnLABQuantizer, PnnQuantizer, _convert_frames_on, _ordered_keyword,
                   load_library)


def _one_size(maps):
    shapes = {a.shape for a in maps}
    if len(shapes) != 1:
        raise ValueError("WebP: all frames must have one size, got %s" % sorted(shapes))
    return maps[0].shape


def webp_max_bytes(n, width, height, band_bits=0):
    """nq_webp_max_bytes: an upper bound of the file size for n frames of width x height (any content, any K; no device needed)."""
    out = C.c_int64(0)
    rc = load_library().nq_webp_max_bytes(int(n), int(width), int(height), int(band_bits), C.byref(out))
    if rc != 0:
        raise NqError(rc, "invalid WebP shape arguments")
    return out.value


def _encode(L, entry, device, stream, ptrs, width, height, palette, delays_cs, loop, band_bits, delta):
    """Returns (file bytes, rectangles as an (n, 4) int32 array of x, y, w, h)."""
    n = len(ptrs)
    pal = _palette(palette)
    d = _delays(delays_cs, n)
    try:
        cap = webp_max_bytes(n, width, height, band_bits)
    except NqError:
        cap = 0                                     # (bad sizes: the encode call below says which)
    buf = np.empty(max(cap, 1), np.uint8)
    rects = np.zeros((max(n, 1), 4), np.int32)
    size = C.c_int64(0)
    src = (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
    args = [int(device)] + ([int(stream) or None] if entry.endswith("_device") else [])
    rc = getattr(L, entry)(*args, n, src, int(width), int(height), pal.ctypes.data, int(pal.size), d.ctypes.data if d is not None else None,
                           int(loop), int(band_bits), 1 if delta else 0, buf.ctypes.data, int(cap), C.byref(size), rects.ctypes.data)
    if rc != 0:
        raise NqError(rc, (L.nq_last_error(None) or b"").decode() or entry)
    return buf[:size.value].tobytes(), rects[:n]


def encode_webp(frames, palette, delays_cs=None, loop=0, band_bits=0, delta=True, device=0, return_rects=False):
    """nq_encode_webp: `frames` is one 2-D index map or a sequence of them, all of one size; `palette` the ARGB_8888 entries they index
    (K = len(palette) <= 256).  delays_cs: per-frame delay in hundredths of a second (None: 0); loop: how often the animation plays
    (0 = for ever, at most 65535); band_bits: a band of 2^band_bits packed rows is one chain (0 = the largest that fits 32768 packed
    pixels); delta: store only the changed rectangle of every frame after the first.  Returns the file; with return_rects=True the
    pair (file, (n, 4) int32 array of every frame's x, y, w, h)."""
    maps = _index_maps(frames)
    height, width = _one_size(maps)
    data, rects = _encode(load_library(), "nq_encode_webp", device, 0, [a.ctypes.data for a in maps], width, height, palette, delays_cs, loop,
                          band_bits, delta)
    return (data, rects) if return_rects else data


def encode_webp_device(d_index_ptrs, width, height, palette, delays_cs=None, loop=0, band_bits=0, delta=True, device=0, stream=0,
                       return_rects=False):
    """nq_encode_webp_device: d_index_ptrs[i] is the HIP device address of frame i's uint16 index map (width x height, 2-byte aligned;
    never written); the work runs on `stream` (a hipStream_t as an integer, 0 = the default stream) of `device`.  Arguments and result
    otherwise as encode_webp."""
    if len(d_index_ptrs) == 0:
        raise ValueError("no frames")
    data, rects = _encode(load_library(), "nq_encode_webp_device", device, stream, list(d_index_ptrs), width, height, palette, delays_cs, loop,
                          band_bits, delta)
    return (data, rects) if return_rects else data


def write_webp(path, frames, palette, delays_cs=None, loop=0, band_bits=0, delta=True, device=0):
    """encode_webp, written to `path`.  Returns the number of bytes written."""
    data = encode_webp(frames, palette, delays_cs, loop, band_bits, delta, device)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def convert_to_webp(kind, image, nMaxColors, dither, band_bits=0, device=0, mode=MODE_PARALLEL_TILED, seed=0, tile=None):
    """convert(nMaxColors, dither) of the RGB (kind 0) or LAB (kind 1) quantizer followed by the WebP encoding of its index map on the
    same device.  nMaxColors <= 256.  Returns (file bytes, palette)."""
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("the colour table of a lossless WebP holds at most 256 entries")
    q = (PnnLABQuantizer if kind == NQ_KIND_LAB else PnnQuantizer)(image, device=device, mode=mode, seed=seed, tile=tile)
    try:
        out = q.convert(nMaxColors, dither)
    finally:
        q.close()
    return encode_webp(out.index, out.palette, band_bits=band_bits, device=device), out.palette


def convert_frames_to_webp(kind, frames, nMaxColors, dither, delays_cs=None, loop=0, seeds=None, tile=None, band_bits=0, device=0,
                           mode=MODE_PARALLEL_TILED, return_rects=False, hold=None, refine=0, size=None, crop=None, linear_resample=True,
                           ordered=None, yuv=None, retime=None, orient=1, delta=True, yuv16=None):
    """convert_frames (one shared palette for the ARGB frames, which must have one size) followed by encode_webp of the index maps on
    the same device.  nMaxColors <= 256.  The keywords are convert_frames_to_apng's (apng.py), with band_bits in place of
    segment_bytes and delta (True: every later frame stores its changed rectangle only) in addition: seeds, tile and mode go to the
    dither; hold runs the temporal hold between the two steps; refine the k-means passes on the palette; ordered the ordered dither.
    size / crop / linear_resample, yuv, orient, yuv16 and retime say what `frames` are and what is done to them first: _frames_in.py.
    Returns (file bytes, palette); with return_rects=True (file bytes, palette, rectangles)."""
    frames, delays_cs, yuv, size, crop, orient = _pre_steps(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient,
                                                            device)
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("the colour table of a lossless WebP holds at most 256 entries")
    if yuv is None and len({np.asarray(f).shape for f in frames}) > 1:
        raise ValueError("WebP: all frames must have one size")
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
        data, rects = _encode(q._L, "nq_encode_webp", device, 0, [a.ctypes.data for a in maps], width, height, palette, delays_cs, loop,
                              band_bits, delta)
    return (data, palette, rects) if return_rects else (data, palette)
