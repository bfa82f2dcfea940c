"""8-bit YUV 4:2:0 frames (NV12, NV21, I420, YV12) into the frame path, on the GPU (nq_frames_from_yuv* / nq_resample_frames_yuv*,
include/nquant_abi.h "YUV input"): what a hardware video decoder, Android's camera and MediaCodec write.  frames_from_yuv converts a
sequence 1:1 to ARGB_8888; resample_frames_yuv converts and reduces it in one kernel, equal bit for bit to frames_from_yuv followed by
resample_frames (resample.py) without the full-size ARGB frames ever existing.  The arithmetic is integer: tests/yuv_ref.py restates
it.  The frame converters (convert_frames_to_gif, convert_shots_to_gif, convert_clip_to_gif, convert_frames_to_apng,
convert_frames_refined, convert_frames_ordered) take yuv={"bt709": ..., "full_range": ...} and then read such frames, on their own
handle.  yuv_planes is host arithmetic and needs no device; the rest has no CPU fallback: without a HIP device every call raises
NqError with status -5 (NQ_ERR_NO_DEVICE).

A host frame is a tuple (y, u, v) of 2-D uint8 arrays: y is (height, width), u and v are ((height + 1) // 2, (width + 1) // 2).  They
may be strided views (yuv_planes gives those of one buffer): where the views of every frame share the row strides and the chroma
element stride (1 or 2), pointers and strides are passed as they are; otherwise the planes are copied tight first."""
import numpy as np

from ._frames_in import _arr, _host_frames as _shared_host_frames
from .gif import _Handle
from .orient import _code, oriented_size
from .resample import RESAMPLE_LINEAR, _geometry

YUV_BT709 = 1
YUV_FULL_RANGE = 2
LAYOUTS = ("nv12", "nv21", "i420", "yv12")


def yuv_planes(buf, width, height, layout):
    """The (y, u, v) views of one contiguous uint8 buffer of width * height + 2 * cw2 * ch2 bytes, cw2 = (width + 1) // 2 and
    ch2 = (height + 1) // 2: the luma plane, then "nv12": u and v interleaved (u first); "nv21": v first; "i420": the u plane, then
    the v plane; "yv12": the v plane first.  No byte is copied."""
    width, height = int(width), int(height)
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (", ".join(LAYOUTS), layout))
    if width < 1 or height < 1:
        raise ValueError("yuv_planes: width and height must be >= 1")
    buf = np.asarray(buf)
    if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
        raise TypeError("yuv_planes: a contiguous 1-D uint8 buffer is needed")
    cw2, ch2 = (width + 1) // 2, (height + 1) // 2
    if buf.size != width * height + 2 * cw2 * ch2:
        raise ValueError("yuv_planes: %d x %d needs %d bytes, got %d" % (width, height, width * height + 2 * cw2 * ch2, buf.size))
    y = buf[:width * height].reshape(height, width)
    c = buf[width * height:]
    if layout in ("nv12", "nv21"):
        c = c.reshape(ch2, cw2, 2)
        first, second = c[:, :, 0], c[:, :, 1]
    else:
        first, second = c[:cw2 * ch2].reshape(ch2, cw2), c[cw2 * ch2:].reshape(ch2, cw2)
    return (y, first, second) if layout in ("nv12", "i420") else (y, second, first)


def _flags(bt709, full_range):
    return (YUV_BT709 if bt709 else 0) | (YUV_FULL_RANGE if full_range else 0)


def _yuv_keyword(yuv):
    """The `yuv` keyword of the converters: a dict with the keys bt709 / full_range (both optional) -> the flag word."""
    if not isinstance(yuv, dict) or set(yuv) - {"bt709", "full_range"}:
        raise TypeError("yuv is None or a dict with the keys bt709 / full_range, got %r" % (yuv,))
    return _flags(yuv.get("bt709", False), yuv.get("full_range", False))


def _host_frames(frames):
    """_frames_in._host_frames for 8-bit planes."""
    return _shared_host_frames(frames, np.uint8, "yuv")


def _call(L, handle, check, entry, y, u, v, width, height, y_stride, c_stride, c_step, flags, dst, geometry, linear, orient=1):
    """One of the four entry points: geometry None is the 1:1 conversion, else (crop_x, crop_y, crop_w, crop_h, dst_w, dst_h).  With
    orient != 1 (a checked code of orient.py) the _oriented form of `entry` is called."""
    n = len(y)
    if not (len(u) == len(v) == len(dst) == n):
        raise ValueError("one u, v and output per frame")
    head = (handle, n, _arr(y), _arr(u), _arr(v), int(width), int(height), int(y_stride), int(c_stride), int(c_step), int(flags))
    if orient != 1:
        entry = entry[:-len("_device")] + "_oriented_device" if entry.endswith("_device") else entry + "_oriented"
        head += (int(orient),)
    if geometry is None:
        check(getattr(L, entry)(*head, _arr(dst)))
    else:
        cx, cy, cw, ch, dw, dh = geometry
        check(getattr(L, entry)(*head, cx, cy, cw, ch, _arr(dst), dw, dh, RESAMPLE_LINEAR if linear else 0))


def _yuv_host(L, handle, check, frames, size, crop, linear, flags, orient=1):
    """nq_frames_from_yuv (size and crop None) or nq_resample_frames_yuv of host frames on an open handle; with orient != 1 (a checked
    code of orient.py) their _oriented forms.  Returns the ARGB frames as a list of int32 arrays."""
    planes, width, height, y_stride, c_stride, c_step = _host_frames(frames)
    geometry = None
    out_w, out_h = (height, width) if orient >= 5 else (width, height)
    if size is not None or crop is not None:
        geometry = _geometry(width, height, size, crop, orient)
        out_w, out_h = geometry[4:]
        if out_w < 1 or out_h < 1:
            raise ValueError("resample: the target must be at least 1 x 1, got %d x %d" % (out_w, out_h))
    outs = [np.zeros((out_h, out_w), np.int32) for _ in planes]
    _call(L, handle, check, "nq_frames_from_yuv" if geometry is None else "nq_resample_frames_yuv", [p[0].ctypes.data for p in planes],
          [p[1].ctypes.data for p in planes], [p[2].ctypes.data for p in planes], width, height, y_stride, c_stride, c_step, flags,
          [o.ctypes.data for o in outs], geometry, linear, orient)
    return outs


def _yuv_quantizer(kind, frames, yuv, device, mode, tile):
    """What _frames_quantizer is to ARGB frames: (the frames, a quantizer of `kind` whose handle runs the frame-sequence calls, the
    flag word of the converters' yuv keyword)."""
    from .host import NQ_KIND_LAB, PnnLABQuantizer, PnnQuantizer
    flags = _yuv_keyword(yuv)
    frames = list(frames)
    if len(frames) == 0:
        raise ValueError("no frames")
    cls = PnnLABQuantizer if int(kind) == NQ_KIND_LAB else PnnQuantizer
    return frames, cls(np.zeros((2, 2), np.int32), device=device, mode=mode, tile=tile), flags


def frames_from_yuv(frames, bt709=False, full_range=False, device=0, orient=1):
    """nq_frames_from_yuv on host arrays: `frames` are (y, u, v) tuples of one size (see the module text).  bt709: the BT.709 matrix
    instead of BT.601; full_range: Y, U, V use 0..255 instead of 16..235 / 16..240.  orient (1..8, orient.py): the frames come out
    oriented (nq_frames_from_yuv_oriented: one kernel).  Returns a list of int32 ARGB_8888 arrays of shape (height, width) -- the
    oriented frame's --, alpha 255."""
    orient = _code(orient)
    hd = _Handle(device)
    try:
        return _yuv_host(hd._L, hd._h, hd._check, frames, None, None, True, _flags(bt709, full_range), orient)
    finally:
        hd.close()


def resample_frames_yuv(frames, size, crop=None, linear=True, bt709=False, full_range=False, device=0, orient=1):
    """nq_resample_frames_yuv on host arrays: frames_from_yuv followed by resample_frames(size, crop, linear), bit for bit, in one
    kernel.  size = (width, height) of the result (None: the crop's), crop = (x, y, width, height) inside the frames (None: the whole
    frame).  orient (1..8, orient.py): the frames are oriented before they are reduced, and size and crop are those of the oriented
    frames (nq_resample_frames_yuv_oriented).  Returns a list of int32 arrays of shape (height, width)."""
    orient = _code(orient)
    frames = list(frames)
    hd = _Handle(device)
    try:
        if size is None and crop is None:
            crop = (0, 0) + oriented_size(*_host_frames(frames)[1:3], orient)
        return _yuv_host(hd._L, hd._h, hd._check, frames, size, crop, linear, _flags(bt709, full_range), orient)
    finally:
        hd.close()


def frames_from_yuv_device(q, d_y, d_u, d_v, width, height, y_stride, c_stride, c_step, d_dst, bt709=False, full_range=False, orient=1):
    """nq_frames_from_yuv_device on the handle of quantizer `q`: d_y[i], d_u[i], d_v[i] are the HIP device addresses of frame i's planes
    (never written), d_dst[i] that of its width x height ARGB words (4-byte aligned).  NV12: d_v[i] = d_u[i] + 1 and c_step 2; NV21:
    d_u[i] = d_v[i] + 1.  orient as for frames_from_yuv.  The work is left running on the handle's stream."""
    orient = _code(orient)
    if len(d_y) == 0:
        raise ValueError("no frames")
    _call(q._L, q._h, q._check, "nq_frames_from_yuv_device", list(d_y), list(d_u), list(d_v), width, height, y_stride, c_stride, c_step,
          _flags(bt709, full_range), list(d_dst), None, True, orient)


def resample_frames_yuv_device(q, d_y, d_u, d_v, src_width, src_height, y_stride, c_stride, c_step, d_dst, size, crop=None, linear=True,
                               bt709=False, full_range=False, orient=1):
    """nq_resample_frames_yuv_device on the handle of quantizer `q`: planes as for frames_from_yuv_device, d_dst[i] the address of frame
    i's size[0] x size[1] result; size, crop, linear, orient as for resample_frames_yuv.  The work is left running on the handle's
    stream."""
    orient = _code(orient)
    if len(d_y) == 0:
        raise ValueError("no frames")
    _call(q._L, q._h, q._check, "nq_resample_frames_yuv_device", list(d_y), list(d_u), list(d_v), src_width, src_height, y_stride, c_stride,
          c_step, _flags(bt709, full_range), list(d_dst), _geometry(src_width, src_height, size, crop, orient), linear, orient)
