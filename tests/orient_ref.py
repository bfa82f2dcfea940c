"""The orientation codes of include/nquant_abi.h "orientation", restated with numpy slicing and .T, apart from the library and its
Python mirror: orient (one frame), orient_all, oriented_size, source_rect (the crop mapping of the reducing calls), orientation (the
code of an Android rotation and a mirror flag), compose (the code of one code applied after another) and the two definitions of the
reducing calls, on top of resample_ref / yuv_ref."""
import numpy as np

import resample_ref
import yuv_ref

CODES = (1, 2, 3, 4, 5, 6, 7, 8)

# out(x, y) = src(sx, sy): the table of the header, as functions of (x, y, W, H)
FORMULAS = {
    1: lambda x, y, W, H: (x, y),
    2: lambda x, y, W, H: (W - 1 - x, y),
    3: lambda x, y, W, H: (W - 1 - x, H - 1 - y),
    4: lambda x, y, W, H: (x, H - 1 - y),
    5: lambda x, y, W, H: (y, x),
    6: lambda x, y, W, H: (y, H - 1 - x),
    7: lambda x, y, W, H: (W - 1 - y, H - 1 - x),
    8: lambda x, y, W, H: (W - 1 - y, x),
}


def orient(frame, code):
    """One 2-D array (H, W) -> the oriented array, contiguous: (H, W) for codes 1..4, (W, H) for codes 5..8."""
    f = np.asarray(frame)
    out = {1: f, 2: f[:, ::-1], 3: f[::-1, ::-1], 4: f[::-1, :],
           5: f.T, 6: f[::-1, :].T, 7: f[::-1, ::-1].T, 8: f[:, ::-1].T}[code]
    return np.ascontiguousarray(out)


def orient_all(frames, code):
    return [orient(f, code) for f in frames]


def oriented_size(w, h, code):
    return (h, w) if code >= 5 else (w, h)


def source_rect(w, h, code, rect):
    """The (x, y, w, h) of the source that `code` carries onto rect of the oriented frame: by marking the rectangle."""
    x, y, rw, rh = rect
    ow, oh = oriented_size(w, h, code)
    assert 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= ow and y + rh <= oh
    ys, xs = np.mgrid[0:h, 0:w]
    oy, ox = orient(ys, code), orient(xs, code)                   # the source row / column of every oriented pixel
    sy, sx = oy[y:y + rh, x:x + rw], ox[y:y + rh, x:x + rw]
    x0, y0, x1, y1 = int(sx.min()), int(sy.min()), int(sx.max()), int(sy.max())
    assert (x1 - x0 + 1) * (y1 - y0 + 1) == rw * rh              # a rectangle goes onto a rectangle
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def orientation(rotation, mirror=False):
    """Turn clockwise by `rotation`, then mirror left-right: the code, found by doing it to a frame."""
    if rotation not in (0, 90, 180, 270):
        raise ValueError(rotation)
    probe = np.arange(6).reshape(2, 3)
    want = np.rot90(probe, -(rotation // 90))
    if mirror:
        want = want[:, ::-1]
    (code,) = [c for c in CODES if orient(probe, c).shape == want.shape and (orient(probe, c) == want).all()]
    return code


def compose(first, then):
    """The code that equals orienting by `first` and the result by `then`."""
    probe = np.arange(6).reshape(2, 3)
    want = orient(orient(probe, first), then)
    (code,) = [c for c in CODES if orient(probe, c).shape == want.shape and (orient(probe, c) == want).all()]
    return code


def resample_oriented(frames, code, size=None, crop=None, flags=resample_ref.LINEAR):
    """nq_resample_frames_oriented by its definition: orient, then reduce (crop and size in oriented coordinates)."""
    return resample_ref.resample(orient_all(frames, code), size, crop, flags)


def yuv_oriented(frames, code, yuv_flags=0):
    """nq_frames_from_yuv_oriented by its definition: convert, then orient."""
    return orient_all(yuv_ref.convert(frames, yuv_flags), code)


def resample_yuv_oriented(frames, code, size=None, crop=None, yuv_flags=0, flags=resample_ref.LINEAR):
    """nq_resample_frames_yuv_oriented by its definition: convert, orient, reduce."""
    return resample_ref.resample(yuv_oriented(frames, code, yuv_flags), size, crop, flags)
