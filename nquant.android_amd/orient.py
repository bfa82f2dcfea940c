"""Turn and mirror frame sequences on the GPU (nq_orient_frames* and the *_oriented entry points, include/nquant_abi.h
"orientation"): a camera or a decoder writes frames in sensor orientation, and a portrait clip would otherwise come out lying on its
side.  The codes are EXIF's 1..8; `orientation` makes one from Android's rotation (sensorOrientation, MediaCodec's KEY_ROTATION) and a
mirror flag.  orient_frames turns ARGB frames; frames_from_yuv, resample_frames, resample_frames_yuv, their _device forms and the
frame converters that take size= / crop= / yuv= take orient= and then produce the oriented frames: size and crop are given in oriented
(as displayed) coordinates.  Words are moved, never changed: tests/orient_ref.py restates the codes.  orientation, oriented_size and
source_rect are host arithmetic and need no device; the rest has no CPU fallback: without a HIP device every call raises NqError with
status -5 (NQ_ERR_NO_DEVICE)."""
import numpy as np

from ._frames_in import _arr
from .gif import _Handle
from .host import _as_i32

# (rotation clockwise, mirrored left-right afterwards) -> EXIF code
_CODES = {(0, False): 1, (90, False): 6, (180, False): 3, (270, False): 8, (0, True): 2, (90, True): 5, (180, True): 4, (270, True): 7}


def orientation(rotation, mirror=False):
    """The code of a frame that has to be turned clockwise by `rotation` degrees (0, 90, 180 or 270: Android's sensorOrientation and
    KEY_ROTATION) and then, with mirror=True, mirrored left-right (a front camera).  Anything else raises ValueError."""
    key = (rotation, bool(mirror))
    if isinstance(rotation, (bool, np.bool_)) or key not in _CODES:
        raise ValueError("rotation must be 0, 90, 180 or 270 (clockwise), got %r" % (rotation,))
    return _CODES[key]


def _code(orient):
    """The checked code of an `orient` keyword."""
    if isinstance(orient, (bool, np.bool_)) or int(orient) != orient or not 1 <= int(orient) <= 8:
        raise ValueError("orient is an EXIF orientation 1..8 (see orientation()), got %r" % (orient,))
    return int(orient)


def oriented_size(width, height, code):
    """(width, height) of a width x height frame after orientation `code`: the sides swap for codes 5..8."""
    width, height = int(width), int(height)
    return (height, width) if _code(code) >= 5 else (width, height)


def source_rect(width, height, code, rect):
    """The rectangle (x, y, w, h) of the width x height SOURCE frame that orientation `code` carries onto rect = (x, y, w, h) of the
    oriented frame: the crop mapping of the reducing *_oriented calls."""
    width, height, code = int(width), int(height), _code(code)
    x, y, w, h = (int(v) for v in rect)
    turn, fx, fy = code >= 5, code in (2, 3, 7, 8), code in (3, 4, 6, 7)
    # along the source's columns lies the oriented y axis when the code turns, else the x axis
    a, al, b, bl = (y, h, x, w) if turn else (x, w, y, h)
    return (width - a - al if fx else a), (height - b - bl if fy else b), al, bl


def _orient(L, handle, check, entry, src_ptrs, width, height, dst_ptrs, code):
    if len(dst_ptrs) != len(src_ptrs):
        raise ValueError("one output per frame")
    check(getattr(L, entry)(handle, len(src_ptrs), _arr(src_ptrs), int(width), int(height), int(code), _arr(dst_ptrs)))


def _orient_host(L, handle, check, frames, code):
    """nq_orient_frames of host frames on an open handle.  Returns the oriented frames as a list of int32 arrays."""
    frames = [np.ascontiguousarray(_as_i32(f)) for f in frames]
    if len(frames) == 0:
        raise ValueError("no frames")
    if len({f.shape for f in frames}) != 1 or frames[0].ndim != 2:
        raise ValueError("orient: the frames must be 2-D arrays of one size, got %s" % sorted({f.shape for f in frames}))
    height, width = frames[0].shape
    ow, oh = oriented_size(width, height, code)
    outs = [np.zeros((oh, ow), np.int32) for _ in frames]
    _orient(L, handle, check, "nq_orient_frames", [f.ctypes.data for f in frames], width, height, [o.ctypes.data for o in outs], code)
    return outs


def orient_frames(frames, orient, device=0):
    """nq_orient_frames on host arrays: `frames` are 2-D int32/uint32 ARGB_8888 arrays of one size, orient the code 1..8.  Returns a
    list of int32 arrays of shape oriented_size(width, height, orient)[::-1]."""
    code = _code(orient)
    hd = _Handle(device)
    try:
        return _orient_host(hd._L, hd._h, hd._check, frames, code)
    finally:
        hd.close()


def orient_frames_device(q, d_src, width, height, d_dst, orient):
    """nq_orient_frames_device on the handle of quantizer `q`: d_src[i] is the HIP device address of frame i (width x height ARGB
    words, never written), d_dst[i] that of its oriented frame (as many words; it may not overlap any source); 4-byte aligned, and when
    all are 16-byte aligned, width is a multiple of 4 and, for codes 5..8, so is height, the kernel moves 16 bytes per access.  The
    work is left running on the handle's stream."""
    if len(d_src) == 0:
        raise ValueError("no frames")
    _orient(q._L, q._h, q._check, "nq_orient_frames_device", list(d_src), width, height, list(d_dst), _code(orient))
