"""GIF89a files from the quantizer's index maps, encoded on the GPU (nq_encode_gif / nq_encode_gif_device, include/nquant_abi.h
"GIF encoding").  One global colour table for all frames: the palette convert() or convert_frames() returned (K <= 256).  GIF has
1-bit transparency: the first palette entry whose alpha is 0 becomes the transparent index, other alpha values are dropped.
Delta mode (nq_encode_gif_delta / nq_encode_gif_delta_device, "GIF encoding, delta mode"): frames of one size, each after the first
stored as the rectangle that changed with the unchanged pixels transparent.  Static regions repeat from frame to frame only when the
dither makes them repeat: MODE_PARALLEL_TILED with equal seeds for all frames does (a tile's chain depends on its pixels, its
position and the seed alone).
Lossy mode (the nq_encode_gif*_lossy* calls, "GIF encoding, lossy mode"): every encoder here takes a trailing lossy=0..255.  Above 0 the
LZW chains may write a palette colour within `lossy` per channel of a pixel's own where that continues the current dictionary string,
which is what shrinks dithered content; 0 calls the lossless entry points.
Local colour tables (the nq_encode_gif_local* calls, "GIF encoding, local colour tables"): one palette per frame, so an animation is not
tied to 256 colours for its whole length.  The practical unit is the shot: convert_shots_to_gif gives every shot its own palette, and
delta mode there compares the colours shown, not the indices; convert_clip_to_gif finds the shots itself (shots.py).
There is no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from ._frames_in import _opened, _pre_steps
from .host import MODE_PARALLEL_TILED, NqError, _convert_frames_on, _frame_sizes, _ordered_keyword, convert_frames, load_library


def _palette(palette):
    pal = np.ascontiguousarray(np.asarray(palette).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32).reshape(-1)
    return pal


def _index_maps(indices):
    if isinstance(indices, np.ndarray) and indices.ndim == 2:
        indices = [indices]
    out = []
    for a in indices:
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError("every index map must be a 2-D (height, width) array")
        if a.dtype != np.uint16:
            if a.dtype.kind not in "iu":
                raise TypeError("index maps must hold integers, got %s" % a.dtype)
            if a.size and (a.min() < 0 or a.max() > 65535):
                raise ValueError("index out of the uint16 range")
            a = a.astype(np.uint16)
        out.append(np.ascontiguousarray(a))
    if not out:
        raise ValueError("no frames")
    return out


def _delays(delays_cs, n):
    if delays_cs is None:
        return None
    d = np.ascontiguousarray(delays_cs, np.int32).reshape(-1)
    if d.size != n:
        raise ValueError("one delay per frame")
    return d


def gif_max_bytes(widths, heights, K=256, segment_pixels=0):
    """nq_gif_max_bytes: an upper bound of the file size for frames of these sizes (any content; no device needed)."""
    L = load_library()
    w = np.ascontiguousarray(widths, np.int32).reshape(-1)
    h = np.ascontiguousarray(heights, np.int32).reshape(-1)
    if w.size != h.size:
        raise ValueError("one width and one height per frame")
    out = C.c_int64(0)
    rc = L.nq_gif_max_bytes(int(w.size), w.ctypes.data, h.ctypes.data, int(K), int(segment_pixels), C.byref(out))
    if rc != 0:
        raise NqError(rc, "invalid GIF shape arguments")
    return out.value


# the lossy counterpart of every encoder entry point (include/nquant_abi.h, "GIF encoding, lossy mode")
_LOSSY = {"nq_encode_gif": "nq_encode_gif_lossy", "nq_encode_gif_device": "nq_encode_gif_lossy_device",
          "nq_encode_gif_delta": "nq_encode_gif_delta_lossy", "nq_encode_gif_delta_device": "nq_encode_gif_delta_lossy_device"}


def _entry(L, entry, segment_pixels, lossy):
    """(the function to call, its arguments from segment_pixels on up to the output buffer): lossy 0 is the lossless export."""
    if int(lossy) == 0:
        return getattr(L, entry), (int(segment_pixels),)
    return getattr(L, _LOSSY[entry]), (int(segment_pixels), int(lossy))


def _encode(L, handle, entry, ptrs, w, h, palette, delays_cs, loop, segment_pixels, check, lossy=0):
    n = len(ptrs)
    pal = _palette(palette)
    d = _delays(delays_cs, n)
    try:
        cap = gif_max_bytes(w, h, 256, segment_pixels)
    except NqError:
        cap = 0                                     # (bad sizes: the encode call below says which)
    buf = np.empty(max(cap, 1), np.uint8)
    size = C.c_int64(0)
    src = (C.c_void_p * n)(*[int(p) for p in ptrs])
    fn, seg = _entry(L, entry, segment_pixels, lossy)
    check(fn(handle, n, src, w.ctypes.data, h.ctypes.data, pal.ctypes.data, int(pal.size), d.ctypes.data if d is not None else None,
             int(loop), *seg, buf.ctypes.data, int(cap), C.byref(size)))
    return buf[:size.value].tobytes()


def _encode_delta(L, handle, entry, ptrs, width, height, palette, delays_cs, loop, segment_pixels, check, lossy=0):
    """The delta entry points: one size for all frames.  Returns (file bytes, rectangles as an (n, 4) int32 array of x, y, w, h)."""
    n = len(ptrs)
    pal = _palette(palette)
    d = _delays(delays_cs, n)
    try:
        cap = gif_max_bytes([width] * n, [height] * n, 256, segment_pixels)
    except NqError:
        cap = 0                                     # (bad sizes: the encode call below says which)
    buf = np.empty(max(cap, 1), np.uint8)
    rects = np.zeros((max(n, 1), 4), np.int32)
    size = C.c_int64(0)
    src = (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
    fn, seg = _entry(L, entry, segment_pixels, lossy)
    check(fn(handle, n, src, int(width), int(height), pal.ctypes.data, int(pal.size), d.ctypes.data if d is not None else None, int(loop),
             *seg, buf.ctypes.data, int(cap), C.byref(size), rects.ctypes.data))
    return buf[:size.value].tobytes(), rects[:n]


def _one_size(maps):
    shapes = {a.shape for a in maps}
    if len(shapes) != 1:
        raise ValueError("delta mode: all frames must have one size, got %s" % sorted(shapes))
    return maps[0].shape


class _Handle:
    """A bare library handle (the GIF calls use only its stream, scratch and error text)."""

    def __init__(self, device=0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.nq_create(0, int(device), C.byref(h))
        if rc != 0:
            raise NqError(rc, (self._L.nq_last_error(None) or b"").decode())
        self._h = h

    def _check(self, rc):
        if rc != 0:
            raise NqError(rc, (self._L.nq_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            self._L.nq_destroy(self._h)
            self._h = None


def encode_gif(indices, palette, delays_cs=None, loop=0, segment_pixels=0, device=0, lossy=0):
    """nq_encode_gif: `indices` is one 2-D index map or a sequence of them (sizes may differ), `palette` the ARGB_8888 entries they
    index (K = len(palette) <= 256).  delays_cs: per-frame delay in hundredths of a second (None: 0); loop: the NETSCAPE2.0 loop
    count of an animation (0 = for ever, -1 = no loop block); segment_pixels: pixels per LZW chain (0 = 16384); lossy: 0..255, the
    largest per-channel colour error a chain may trade for a longer match (0: none, nq_encode_gif_lossy otherwise).  Returns the file."""
    maps = _index_maps(indices)
    w = np.array([a.shape[1] for a in maps], np.int32)
    h = np.array([a.shape[0] for a in maps], np.int32)
    hd = _Handle(device)
    try:
        return _encode(hd._L, hd._h, "nq_encode_gif", [a.ctypes.data for a in maps], w, h, palette, delays_cs, loop, segment_pixels, hd._check,
                       lossy)
    finally:
        hd.close()


def encode_gif_device(q, d_index_ptrs, widths, heights, palette, delays_cs=None, loop=0, segment_pixels=0, lossy=0):
    """nq_encode_gif_device on the handle of quantizer `q`: d_index_ptrs[i] is the HIP device address of frame i's uint16 index map
    (widths[i] x heights[i], 2-byte aligned).  Arguments otherwise as encode_gif.  Returns the file."""
    n = len(d_index_ptrs)
    w, h = _frame_sizes(widths, heights, n)
    return _encode(q._L, q._h, "nq_encode_gif_device", list(d_index_ptrs), w, h, palette, delays_cs, loop, segment_pixels, q._check,
                   lossy)


def encode_gif_delta(indices, palette, delays_cs=None, loop=0, segment_pixels=0, device=0, return_rects=False, lossy=0):
    """nq_encode_gif_delta: as encode_gif, but all frames have one size, every frame after the first stores only the bounding rectangle
    of the pixels that differ from the frame before, and the unchanged pixels in it are transparent (index K; K = 256: cropped only).
    A palette entry with alpha 0 is an error when there are two frames or more.  lossy as for encode_gif (the rectangles do not
    depend on it).  Returns the file; with return_rects=True the pair
    (file, (n, 4) int32 array of every frame's x, y, w, h)."""
    maps = _index_maps(indices)
    height, width = _one_size(maps)
    hd = _Handle(device)
    try:
        data, rects = _encode_delta(hd._L, hd._h, "nq_encode_gif_delta", [a.ctypes.data for a in maps], width, height, palette, delays_cs,
                                    loop, segment_pixels, hd._check, lossy)
    finally:
        hd.close()
    return (data, rects) if return_rects else data


def encode_gif_delta_device(q, d_index_ptrs, width, height, palette, delays_cs=None, loop=0, segment_pixels=0, return_rects=False, lossy=0):
    """nq_encode_gif_delta_device on the handle of quantizer `q`: d_index_ptrs[i] is the HIP device address of frame i's uint16 index
    map (width x height, 2-byte aligned; never written).  Arguments and result otherwise as encode_gif_delta."""
    if len(d_index_ptrs) == 0:
        raise ValueError("no frames")
    data, rects = _encode_delta(q._L, q._h, "nq_encode_gif_delta_device", list(d_index_ptrs), width, height, palette, delays_cs, loop,
                                segment_pixels, q._check, lossy)
    return (data, rects) if return_rects else data


# ---- local colour tables: one palette per frame ----
def gif_local_max_bytes(widths, heights, segment_pixels=0):
    """nq_gif_local_max_bytes: an upper bound of the size of a file with a local colour table per frame (any content, any K; no device
    needed).  Delta mode: one width and one height per frame, all equal."""
    L = load_library()
    w = np.ascontiguousarray(widths, np.int32).reshape(-1)
    h = np.ascontiguousarray(heights, np.int32).reshape(-1)
    if w.size != h.size:
        raise ValueError("one width and one height per frame")
    out = C.c_int64(0)
    rc = L.nq_gif_local_max_bytes(int(w.size), w.ctypes.data, h.ctypes.data, int(segment_pixels), C.byref(out))
    if rc != 0:
        raise NqError(rc, "invalid GIF shape arguments")
    return out.value


def _palettes(palettes, n):
    """(the palettes packed to one stride as a (n, stride) uint32 array, K per frame): ragged lengths are allowed."""
    pals = [_palette(p) for p in palettes]
    if len(pals) != n:
        raise ValueError("one palette per frame: %d palettes for %d frames" % (len(pals), n))
    K = np.array([p.size for p in pals], np.int32)
    packed = np.zeros((max(n, 1), max(int(K.max()) if n else 1, 1)), np.uint32)
    for i, p in enumerate(pals):
        packed[i, :p.size] = p
    return packed, K


def _encode_local(L, handle, entry, ptrs, w, h, palettes, delays_cs, loop, segment_pixels, lossy, check, delta):
    """One call of any of the four local exports; delta: w and h are the one size.  Returns (file bytes, rectangles or None)."""
    n = len(ptrs)
    if n == 0:
        raise ValueError("no frames")
    pal, K = _palettes(palettes, n)
    d = _delays(delays_cs, n)
    try:
        cap = gif_local_max_bytes([w] * n if delta else w, [h] * n if delta else h, segment_pixels)
    except NqError:
        cap = 0                                     # (bad sizes: the encode call below says which)
    buf = np.empty(max(cap, 1), np.uint8)
    size = C.c_int64(0)
    src = (C.c_void_p * n)(*[int(p) for p in ptrs])
    sizes = (int(w), int(h)) if delta else (w.ctypes.data, h.ctypes.data)
    rects = np.zeros((n, 4), np.int32) if delta else None
    check(getattr(L, entry)(handle, n, src, *sizes, pal.ctypes.data, int(pal.shape[1]), K.ctypes.data, d.ctypes.data if d is not None else None,
                            int(loop), int(segment_pixels), int(lossy), buf.ctypes.data, int(cap), C.byref(size),
                            *((rects.ctypes.data,) if delta else ())))
    return buf[:size.value].tobytes(), rects


def encode_gif_local(indices, palettes, delays_cs=None, loop=0, segment_pixels=0, device=0, lossy=0):
    """nq_encode_gif_local: as encode_gif, but `palettes` is a sequence of one palette per frame (lengths may differ, each <= 256) and
    every frame is written with its own local colour table; the file has no global one.  Returns the file."""
    maps = _index_maps(indices)
    w = np.array([a.shape[1] for a in maps], np.int32)
    h = np.array([a.shape[0] for a in maps], np.int32)
    _palettes(palettes, len(maps))                   # (argument errors come before the device is asked for)
    hd = _Handle(device)
    try:
        return _encode_local(hd._L, hd._h, "nq_encode_gif_local", [a.ctypes.data for a in maps], w, h, palettes, delays_cs, loop,
                             segment_pixels, lossy, hd._check, False)[0]
    finally:
        hd.close()


def encode_gif_local_device(q, d_index_ptrs, widths, heights, palettes, delays_cs=None, loop=0, segment_pixels=0, lossy=0):
    """nq_encode_gif_local_device on the handle of quantizer `q`: as encode_gif_device with one palette per frame."""
    w, h = _frame_sizes(widths, heights, len(d_index_ptrs))
    return _encode_local(q._L, q._h, "nq_encode_gif_local_device", list(d_index_ptrs), w, h, palettes, delays_cs, loop, segment_pixels,
                         lossy, q._check, False)[0]


def encode_gif_local_delta(indices, palettes, delays_cs=None, loop=0, segment_pixels=0, device=0, return_rects=False, lossy=0):
    """nq_encode_gif_local_delta: as encode_gif_delta with one palette per frame.  A pixel is unchanged when the COLOUR it shows is the
    one the frame before showed there, whatever the two indices are: frames of one shot, which share a palette, drop their still regions
    as before, and where the palette changes the frame is repainted.  Returns the file; with return_rects=True (file, rectangles)."""
    maps = _index_maps(indices)
    height, width = _one_size(maps)
    _palettes(palettes, len(maps))                   # (argument errors come before the device is asked for)
    hd = _Handle(device)
    try:
        data, rects = _encode_local(hd._L, hd._h, "nq_encode_gif_local_delta", [a.ctypes.data for a in maps], width, height, palettes,
                                    delays_cs, loop, segment_pixels, lossy, hd._check, True)
    finally:
        hd.close()
    return (data, rects) if return_rects else data


def encode_gif_local_delta_device(q, d_index_ptrs, width, height, palettes, delays_cs=None, loop=0, segment_pixels=0, return_rects=False,
                                  lossy=0):
    """nq_encode_gif_local_delta_device on the handle of quantizer `q`: as encode_gif_delta_device with one palette per frame."""
    data, rects = _encode_local(q._L, q._h, "nq_encode_gif_local_delta_device", list(d_index_ptrs), width, height, palettes, delays_cs, loop,
                                segment_pixels, lossy, q._check, True)
    return (data, rects) if return_rects else data


def _shots(shot_starts, n):
    """[(first frame, one past the last)] per shot."""
    starts = [int(s) for s in shot_starts]
    if not starts or starts[0] != 0 or any(b <= a for a, b in zip(starts[:-1], starts[1:])) or starts[-1] >= n:
        raise ValueError("shot_starts must be an increasing list of frame numbers below %d that begins with 0, got %r" % (n, starts))
    return list(zip(starts, starts[1:] + [n]))


def convert_shots_to_gif(kind, frames, shot_starts, nMaxColors, dither, delays_cs=None, loop=0, segment_pixels=0, device=0,
                         mode=MODE_PARALLEL_TILED, seeds=None, tile=None, hold=None, lossy=0, refine=0, size=None, crop=None,
                         linear_resample=True, ordered=None, yuv=None, retime=None, orient=1, yuv16=None, delta=True):
    """One palette per shot: frames shot_starts[k] .. shot_starts[k + 1] - 1 are shot k and get a convert_frames palette of their own
    (shot_starts=range(n): one palette per frame), then encode_gif_local_delta (delta=False: encode_gif_local) writes all frames, each
    with its shot's palette as its local colour table.  hold (delta=True only) runs per shot and never across a cut: a held index means
    nothing under another table.  seeds, tile, lossy as for convert_frames_to_gif; refine (0..64) runs that many k-means passes
    (refine.py) on every shot's palette over that shot's frames.  ordered as for convert_frames_to_gif.
    size / crop / linear_resample, yuv, orient and yuv16 say what `frames` are and what is done to them first: _frames_in.py.
    Everything runs on one handle.  Cuts are the caller's to give here; convert_clip_to_gif finds them.
    retime is refused here (ValueError): shot_starts name source frames, and retimed frames are other frames; convert_clip_to_gif
    takes it.
    Returns (file bytes, list of per-shot palettes)."""
    if retime is not None:
        raise ValueError("retime changes the frames that shot_starts name: retime first (retime.py), or let convert_clip_to_gif find the cuts")
    frames, delays_cs, yuv, size, crop, orient = _pre_steps(frames, None, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient,
                                                            device)
    lossy = _lossy_keyword(lossy)
    ordered = _ordered_keyword(ordered, seeds)
    from .orient import _code as _orient_code
    orient = _orient_code(orient)
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("a GIF colour table holds at most 256 entries")
    if hold is not None and not delta:
        raise ValueError("hold needs delta=True: full frames store every pixel whether it repeats or not")
    if yuv is None and delta and len({np.asarray(f).shape for f in frames}) > 1:
        raise ValueError("delta mode: all frames must have one size")
    shots = _shots(shot_starts, len(frames))
    if seeds is not None and len(list(seeds)) != len(frames):
        raise ValueError("one seed per frame")
    if hold is not None:
        from .hold import _threshold
        hold = _threshold(hold)
    with _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, mode, tile) as (q, frames):
        return _shots_to_gif_on(q, frames, shots, nMaxColors, dither, delays_cs, loop, segment_pixels, mode, seeds, hold, lossy, delta, refine, ordered)


def _shots_to_gif_on(q, frames, shots, nMaxColors, dither, delays_cs, loop, segment_pixels, mode, seeds, hold, lossy, delta, refine=0,
                     ordered=None):
    """convert_shots_to_gif after its checks, on the handle of quantizer `q`, which stays open: `frames` int32 arrays, `shots` the
    (first frame, one past the last) pairs, hold a checked threshold or None, refine the k-means passes per shot (0: none), ordered a
    checked limit of the ordered dither or None."""
    if hold is not None:
        from .hold import _hold_host
    maps, palettes = [], []
    for a, b in shots:
        palette, outs = _convert_frames_on(q, frames[a:b], nMaxColors, dither, mode, None if seeds is None else list(seeds)[a:b], int(refine) or None,
                                           ordered)
        shot_maps = [o.index for o in outs]
        if hold is not None:
            _hold_host(q._L, q._h, q._check, frames[a:b], shot_maps, None, hold)
        maps += shot_maps
        palettes.append(palette)
    per_frame = [palettes[k] for k, (a, b) in enumerate(shots) for _ in range(a, b)]
    ptrs = [m.ctypes.data for m in maps]
    if delta:
        height, width = _one_size(maps)
        data, _ = _encode_local(q._L, q._h, "nq_encode_gif_local_delta", ptrs, width, height, per_frame, delays_cs, loop, segment_pixels,
                                lossy, q._check, True)
    else:
        w = np.array([m.shape[1] for m in maps], np.int32)
        h = np.array([m.shape[0] for m in maps], np.int32)
        data, _ = _encode_local(q._L, q._h, "nq_encode_gif_local", ptrs, w, h, per_frame, delays_cs, loop, segment_pixels, lossy,
                                q._check, False)
    return data, palettes


def convert_clip_to_gif(kind, frames, nMaxColors, dither, cut=60, min_shot=8, delays_cs=None, loop=0, segment_pixels=0, device=0,
                        mode=MODE_PARALLEL_TILED, seeds=None, tile=None, hold=None, lossy=0, refine=0, size=None, crop=None,
                        linear_resample=True, ordered=None, yuv=None, retime=None, orient=1, yuv16=None, delta=True):
    """A list of frames in, an animation out: detect_shots (shots.py; cut in per mille, min_shot in frames) finds where the clip needs
    a new palette, then exactly convert_shots_to_gif with those starts -- both on one handle.  The frames must have one size (delta or
    not: a signature is compared between frames of one size).  With size or crop the frames are reduced first (resample.py) and the
    shots are detected on the result.  Keywords otherwise as for convert_shots_to_gif, and retime is taken.
    size / crop / linear_resample, yuv, orient, yuv16 and retime say what `frames` are and what is done to them first: _frames_in.py.
    Returns (file bytes, list of per-shot palettes, shot_starts)."""
    frames, delays_cs, yuv, size, crop, orient = _pre_steps(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient,
                                                            device)
    lossy = _lossy_keyword(lossy)
    ordered = _ordered_keyword(ordered, seeds)
    from .orient import _code as _orient_code
    orient = _orient_code(orient)
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("a GIF colour table holds at most 256 entries")
    if hold is not None and not delta:
        raise ValueError("hold needs delta=True: full frames store every pixel whether it repeats or not")
    if yuv is None and len({np.asarray(f).shape for f in frames}) > 1:
        raise ValueError("shot detection: all frames must have one size")
    if seeds is not None and len(list(seeds)) != len(frames):
        raise ValueError("one seed per frame")
    if hold is not None:
        from .hold import _threshold
        hold = _threshold(hold)
    from .shots import _detect_host
    with _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, mode, tile) as (q, frames):
        starts, _ = _detect_host(q._L, q._h, q._check, frames, cut, min_shot)
        data, palettes = _shots_to_gif_on(q, frames, _shots(starts, len(frames)), nMaxColors, dither, delays_cs, loop, segment_pixels, mode,
                                          seeds, hold, lossy, delta, refine, ordered)
    return data, palettes, starts


def _lossy_keyword(lossy):
    """write_gif and convert_frames_to_gif keep `delta` as their last parameter, so `lossy` sits where an older positional call put
    delta: a bool there is that call, not a threshold."""
    if isinstance(lossy, (bool, np.bool_)):
        raise TypeError("lossy is an integer 0..255; pass delta by keyword")
    return int(lossy)


def write_gif(path, indices, palette, delays_cs=None, loop=0, segment_pixels=0, device=0, lossy=0, delta=False):
    """encode_gif (delta=True: encode_gif_delta), written to `path`; lossy as there.  Returns the number of bytes written."""
    lossy = _lossy_keyword(lossy)
    data = (encode_gif_delta if delta else encode_gif)(indices, palette, delays_cs, loop, segment_pixels, device, lossy=lossy)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def convert_frames_to_gif(kind, frames, nMaxColors, dither, delays_cs=None, loop=0, segment_pixels=0, device=0, mode=MODE_PARALLEL_TILED,
                          seeds=None, tile=None, hold=None, lossy=0, refine=0, size=None, crop=None, linear_resample=True, ordered=None,
                          yuv=None, retime=None, orient=1, yuv16=None, delta=False):
    """convert_frames (one shared palette for the ARGB frames) followed by encode_gif of the index maps.  nMaxColors <= 256.
    delta=True: encode_gif_delta instead; the frames must have one size.  Seeds are passed on as given: regions that do not move repeat
    in the index maps, and so drop out of the file, when the frames are dithered with equal seeds in MODE_PARALLEL_TILED.
    hold (delta=True only; None: no such pass): an integer 0..255 runs the temporal hold (hold.py) with that threshold between the
    two steps, so that pixels whose source moved by no more than it keep their index -- what footage with sensor or codec noise needs
    for its still regions to drop out.  All three steps then run on one handle; the index maps pass through host memory in between.
    lossy: as for encode_gif, applied to whichever encoder runs (with hold: on that same handle).
    refine (0..64): that many k-means passes on the palette over the frames before the dither (refine.py, convert_frames_refined);
    0 is the call without it.
    ordered (None: the error-diffusion dither): an integer 0..255 dithers the frames with the ordered dither (ordered.py,
    convert_frames_ordered) with that limit instead: a pixel's index then depends on its colour, its position and the palette only, so
    unchanged pixels repeat without seeds.  dither, mode and tile then take no part, and seeds may not be given.
    size / crop / linear_resample, yuv, orient, yuv16 and retime say what `frames` are and what is done to them first: _frames_in.py.
    Returns (file bytes, palette)."""
    frames, delays_cs, yuv, size, crop, orient = _pre_steps(frames, retime, delays_cs, seeds, yuv, yuv16, size, crop, linear_resample, orient,
                                                            device)
    lossy = _lossy_keyword(lossy)
    ordered = _ordered_keyword(ordered, seeds)
    from .orient import _code as _orient_code
    orient = _orient_code(orient)
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("a GIF colour table holds at most 256 entries")
    if hold is not None and not delta:
        raise ValueError("hold needs delta=True: full frames store every pixel whether it repeats or not")
    if yuv is None and delta and len({np.asarray(f).shape for f in frames}) > 1:
        raise ValueError("delta mode: all frames must have one size")
    if size is not None or crop is not None or yuv is not None or orient != 1:
        if hold is not None:
            from .hold import _hold_host, _threshold
            hold = _threshold(hold)
        with _opened(kind, frames, yuv, size, crop, linear_resample, orient, device, mode, tile) as (q, frames):
            palette, outs = _convert_frames_on(q, frames, nMaxColors, dither, mode, seeds, int(refine) or None, ordered)
            maps = _index_maps([o.index for o in outs])
            height, width = _one_size(maps)
            if hold is not None:
                _hold_host(q._L, q._h, q._check, frames, maps, None, hold)
            ptrs = [a.ctypes.data for a in maps]
            if delta:
                data, _ = _encode_delta(q._L, q._h, "nq_encode_gif_delta", ptrs, width, height, palette, delays_cs, loop, segment_pixels,
                                        q._check, lossy)
            else:
                data = _encode(q._L, q._h, "nq_encode_gif", ptrs, np.array([width] * len(maps), np.int32),
                               np.array([height] * len(maps), np.int32), palette, delays_cs, loop, segment_pixels, q._check, lossy)
        return data, palette
    if hold is not None:
        from .hold import _hold_host, _threshold
        hold = _threshold(hold)
        with _opened(kind, frames, None, None, None, linear_resample, 1, device, mode, tile) as (q, frames):
            palette, outs = _convert_frames_on(q, frames, nMaxColors, dither, mode, seeds, int(refine) or None, ordered)
            maps = [o.index for o in outs]
            height, width = _one_size(maps)
            _hold_host(q._L, q._h, q._check, frames, maps, None, hold)
            data, _ = _encode_delta(q._L, q._h, "nq_encode_gif_delta", [a.ctypes.data for a in maps], width, height, palette, delays_cs, loop,
                                    segment_pixels, q._check, lossy)
        return data, palette
    if ordered is not None:
        from .ordered import convert_frames_ordered
        palette, outs = convert_frames_ordered(kind, frames, nMaxColors, ordered, refine, device=device)
    elif int(refine) == 0:
        palette, outs = convert_frames(kind, frames, nMaxColors, dither, device=device, mode=mode, seeds=seeds, tile=tile)
    else:
        from .refine import convert_frames_refined
        palette, outs = convert_frames_refined(kind, frames, nMaxColors, dither, refine, device=device, mode=mode, seeds=seeds, tile=tile)
    data = (encode_gif_delta if delta else encode_gif)([o.index for o in outs], palette, delays_cs, loop, segment_pixels, device, lossy=lossy)
    return data, palette
