"""10-bit YUV 4:2:0 frames (P010, I010 and their chroma-swapped forms; SDR, PQ or HLG) into the frame path, on the GPU
(nq_frames_from_yuv16* / nq_resample_frames_yuv16*, include/nquant_abi.h "10-bit YUV input"): what a 10-bit MediaCodec and the camera's
YCBCR_P010 write.  frames_from_yuv16 converts a sequence 1:1 to ARGB_8888 (8-bit sRGB; PQ and HLG through the tone curve of
include/nq_hdr_luts.inc); resample_frames_yuv16 converts and reduces it in one kernel, equal bit for bit to frames_from_yuv16 followed
by resample_frames (resample.py) without the full-size ARGB frames ever existing.  The arithmetic is integer: tests/yuv16_ref.py
restates it.  The calls take no handle.  The frame converters (convert_frames_to_gif, convert_shots_to_gif, convert_clip_to_gif,
convert_frames_to_apng, convert_frames_to_webp, convert_frames_refined, convert_frames_ordered) take
yuv16={"matrix": ..., "full_range": ..., "transfer": ..., "msb": ...} and then read such frames.  yuv16_planes is host arithmetic and
needs no device; the rest has no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE).

A host frame is a tuple (y, u, v) of 2-D uint16 arrays: y is (height, width), u and v are ((height + 1) // 2, (width + 1) // 2).  They
may be strided views (yuv16_planes gives those of one buffer): where the views of every frame share the row strides and the chroma
element stride (1 or 2 samples), pointers and strides are passed as they are; otherwise the planes are copied tight first."""
import numpy as np

from ._frames_in import _arr, _host_frames as _shared_host_frames
from .host import NqError, load_library
from .orient import _code, oriented_size, source_rect
from .resample import RESAMPLE_LINEAR, _geometry

YUV_BT709 = 1
YUV_FULL_RANGE = 2
YUV16_BT2020 = 4
YUV16_MSB = 8
YUV16_PQ = 16
YUV16_HLG = 32
LAYOUTS = ("p010", "p010_vu", "i010", "yv12_10")
MATRICES = {"bt601": 0, "bt709": YUV_BT709, "bt2020": YUV16_BT2020}
TRANSFERS = {"sdr": 0, "pq": YUV16_PQ, "hlg": YUV16_HLG}


def yuv16_planes(buf, width, height, layout, row_stride=None, chroma_row_stride=None):
    """The (y, u, v) uint16 views of one contiguous buffer (uint8 or uint16, 1-D) that holds the luma plane, then "p010": u and v
    interleaved (u first); "p010_vu": v first; "i010": the u plane, then the v plane; "yv12_10": the v plane first.  row_stride and
    chroma_row_stride are Android's Image.Plane.getRowStride() of the luma and of a chroma plane, in BYTES (None: tight rows); an odd
    stride cannot be counted in samples and is refused.  The buffer holds height luma rows and (height + 1) // 2 rows per chroma
    plane at these strides; its last row may end with its last sample, as Android's buffers do ((rows - 1) * stride + row bytes), or
    anywhere up to the full stride.  No byte is copied."""
    width, height = int(width), int(height)
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (", ".join(LAYOUTS), layout))
    if width < 1 or height < 1:
        raise ValueError("yuv16_planes: width and height must be >= 1")
    buf = np.asarray(buf)
    if buf.dtype not in (np.uint8, np.uint16) or buf.ndim != 1 or not buf.flags.c_contiguous:
        raise TypeError("yuv16_planes: a contiguous 1-D uint8 or uint16 buffer is needed")
    if buf.dtype == np.uint8:
        if buf.size % 2 or buf.ctypes.data % 2:
            raise ValueError("yuv16_planes: a byte buffer must hold whole 16-bit words at an even address")
        buf = buf.view(np.uint16)
    cw2, ch2 = (width + 1) // 2, (height + 1) // 2
    inter = layout in ("p010", "p010_vu")
    ys = 2 * width if row_stride is None else int(row_stride)
    cs = (4 if inter else 2) * cw2 if chroma_row_stride is None else int(chroma_row_stride)
    if ys % 2 or cs % 2:
        raise ValueError("yuv16_planes: row strides of %d and %d bytes: an odd stride cannot be counted in 16-bit samples" % (ys, cs))
    ys, cs = ys // 2, cs // 2
    if ys < width or cs < (2 if inter else 1) * cw2:
        raise ValueError("yuv16_planes: a row stride is shorter than its row")
    need = height * ys + (1 if inter else 2) * ch2 * cs
    least = need - cs + (2 if inter else 1) * cw2                       # the padding behind the last row may be missing
    if not least <= buf.size <= need:
        raise ValueError("yuv16_planes: %d x %d at these strides needs %d to %d samples, got %d" % (width, height, least, need, buf.size))
    view = lambda off, rows, cols, stride, step: np.lib.stride_tricks.as_strided(buf[off:], (rows, cols), (2 * stride, 2 * step), writeable=False)
    y = view(0, height, width, ys, 1)
    if inter:
        first, second = view(height * ys, ch2, cw2, cs, 2), view(height * ys + 1, ch2, cw2, cs, 2)
    else:
        first, second = view(height * ys, ch2, cw2, cs, 1), view(height * ys + ch2 * cs, ch2, cw2, cs, 1)
    return (y, first, second) if layout in ("p010", "i010") else (y, second, first)


def _flags(matrix=None, full_range=False, transfer="sdr", msb=True):
    """The flag word.  matrix None: "bt2020" with the PQ and HLG transfers, "bt709" for SDR."""
    if transfer not in TRANSFERS:
        raise ValueError("transfer must be one of %s, got %r" % (", ".join(TRANSFERS), transfer))
    if matrix is None:
        matrix = "bt709" if transfer == "sdr" else "bt2020"
    if matrix not in MATRICES:
        raise ValueError("matrix must be one of %s, got %r" % (", ".join(MATRICES), matrix))
    return MATRICES[matrix] | (YUV_FULL_RANGE if full_range else 0) | TRANSFERS[transfer] | (YUV16_MSB if msb else 0)


def _yuv16_keyword(yuv16):
    """The `yuv16` keyword of the converters: a dict with the keys matrix / full_range / transfer / msb (all optional) -> the flag word."""
    if not isinstance(yuv16, dict) or set(yuv16) - {"matrix", "full_range", "transfer", "msb"}:
        raise TypeError("yuv16 is None or a dict with the keys matrix / full_range / transfer / msb, got %r" % (yuv16,))
    return _flags(**yuv16)


def _host_frames(frames):
    """_frames_in._host_frames for 10-bit planes in 16-bit words."""
    return _shared_host_frames(frames, np.uint16, "yuv16")


def _check(L, rc, what):
    if rc != 0:
        raise NqError(rc, (L.nq_last_error(None) or b"").decode() or what)


def _call(L, entry, lead, y, u, v, width, height, y_stride, c_stride, c_step, flags, dst, geometry, linear):
    """One of the four entry points: `lead` is (device,) or (device, stream), geometry None the 1:1 conversion, else (crop_x, crop_y,
    crop_w, crop_h, dst_w, dst_h)."""
    n = len(y)
    if not (len(u) == len(v) == len(dst) == n):
        raise ValueError("one u, v and output per frame")
    head = lead + (n, _arr(y), _arr(u), _arr(v), int(width), int(height), int(y_stride), int(c_stride), int(c_step), int(flags))
    if geometry is None:
        _check(L, getattr(L, entry)(*head, _arr(dst)), entry)
    else:
        cx, cy, cw, ch, dw, dh = geometry
        _check(L, getattr(L, entry)(*head, cx, cy, cw, ch, _arr(dst), dw, dh, RESAMPLE_LINEAR if linear else 0), entry)


def _yuv16_host(frames, size, crop, linear, flags, orient, device):
    """nq_frames_from_yuv16 (size and crop None) or nq_resample_frames_yuv16 of host frames.  With orient != 1 (a checked code of
    orient.py) size and crop are those of the oriented frames: the frames are converted -- and reduced -- as they lie, and the small
    result is turned by orient_frames, which is exact (orientation moves words, and the reducer treats both axes alike).  Returns
    the ARGB frames as a list of int32 arrays."""
    planes, width, height, y_stride, c_stride, c_step = _host_frames(frames)
    L = load_library()
    geometry = None
    out_w, out_h = width, height
    if size is not None or crop is not None:
        cx, cy, cw, ch, dw, dh = _geometry(width, height, size, crop, orient)
        if dw < 1 or dh < 1:
            raise ValueError("resample: the target must be at least 1 x 1, got %d x %d" % (dw, dh))
        if orient != 1:                                 # the oriented crop and target, in the coordinates of the frames as they lie
            cx, cy, cw, ch = source_rect(width, height, orient, (cx, cy, cw, ch))
            if orient >= 5:
                dw, dh = dh, dw
        geometry = (cx, cy, cw, ch, dw, dh)
        out_w, out_h = dw, dh
    outs = [np.zeros((out_h, out_w), np.int32) for _ in planes]
    _call(L, "nq_frames_from_yuv16" if geometry is None else "nq_resample_frames_yuv16", (int(device),), [p[0].ctypes.data for p in planes],
          [p[1].ctypes.data for p in planes], [p[2].ctypes.data for p in planes], width, height, y_stride, c_stride, c_step, flags,
          [o.ctypes.data for o in outs], geometry, linear)
    if orient != 1:
        from .orient import orient_frames
        outs = orient_frames(outs, orient, device=device)
    return outs


def _converter_frames(frames, yuv, yuv16, size, crop, linear_resample, orient, device):
    """The `yuv16` keyword of the frame converters: the ARGB frames the converter then runs on, already reduced and oriented."""
    if yuv is not None:
        raise TypeError("yuv and yuv16 exclude each other")
    return _yuv16_host(frames, size, crop, linear_resample, _yuv16_keyword(yuv16), _code(orient), device)


def frames_from_yuv16(frames, matrix=None, full_range=False, transfer="sdr", msb=True, device=0, orient=1):
    """nq_frames_from_yuv16 on host arrays: `frames` are (y, u, v) tuples of one size (see the module text).  matrix: "bt601", "bt709" or
    "bt2020" (None: bt2020 with transfer "pq" / "hlg", bt709 with "sdr"); full_range: 0..1023 instead of 64..940 / 64..960; transfer:
    "sdr", "pq" or "hlg"; msb: the sample is the high ten bits of its word (P010), else the low ten (I010).  orient (1..8, orient.py):
    the frames come out oriented (orient_frames on the result).  Returns a list of int32 ARGB_8888 arrays of shape (height, width) --
    the oriented frame's --, alpha 255."""
    return _yuv16_host(frames, None, None, True, _flags(matrix, full_range, transfer, msb), _code(orient), device)


def resample_frames_yuv16(frames, size, crop=None, linear=True, matrix=None, full_range=False, transfer="sdr", msb=True, device=0, orient=1):
    """nq_resample_frames_yuv16 on host arrays: frames_from_yuv16 followed by resample_frames(size, crop, linear), bit for bit, in one
    kernel.  size = (width, height) of the result (None: the crop's), crop = (x, y, width, height) inside the frames (None: the whole
    frame).  orient (1..8, orient.py): size and crop are those of the oriented frames; the frames are reduced as they lie and the small
    result is turned.  Returns a list of int32 arrays of shape (height, width)."""
    orient = _code(orient)
    frames = list(frames)
    if size is None and crop is None:
        crop = (0, 0) + oriented_size(*_host_frames(frames)[1:3], orient)
    return _yuv16_host(frames, size, crop, linear, _flags(matrix, full_range, transfer, msb), orient, device)


def frames_from_yuv16_device(d_y, d_u, d_v, width, height, y_stride, c_stride, c_step, d_dst, matrix=None, full_range=False,
                             transfer="sdr", msb=True, device=0, stream=0):
    """nq_frames_from_yuv16_device: d_y[i], d_u[i], d_v[i] are the HIP device addresses of frame i's planes (16-bit words, never
    written), d_dst[i] that of its width x height ARGB words (4-byte aligned); y_stride, c_stride and c_step count samples.  P010:
    d_v[i] = d_u[i] + 2 bytes and c_step 2.  Asynchronous on `stream` (a hipStream_t as an integer, 0 = the default stream) of
    `device`; allocates nothing."""
    if len(d_y) == 0:
        raise ValueError("no frames")
    _call(load_library(), "nq_frames_from_yuv16_device", (int(device), int(stream) or None), list(d_y), list(d_u), list(d_v), width, height,
          y_stride, c_stride, c_step, _flags(matrix, full_range, transfer, msb), list(d_dst), None, True)


def resample_frames_yuv16_device(d_y, d_u, d_v, src_width, src_height, y_stride, c_stride, c_step, d_dst, size, crop=None, linear=True,
                                 matrix=None, full_range=False, transfer="sdr", msb=True, device=0, stream=0):
    """nq_resample_frames_yuv16_device: planes as for frames_from_yuv16_device, d_dst[i] the address of frame i's size[0] x size[1]
    result; size, crop, linear as for resample_frames_yuv16.  Asynchronous on `stream` of `device`; allocates nothing."""
    if len(d_y) == 0:
        raise ValueError("no frames")
    _call(load_library(), "nq_resample_frames_yuv16_device", (int(device), int(stream) or None), list(d_y), list(d_u), list(d_v), src_width,
          src_height, y_stride, c_stride, c_step, _flags(matrix, full_range, transfer, msb), list(d_dst),
          _geometry(src_width, src_height, size, crop), linear)
