"""Numpy restatement of the YUV input (include/nquant_abi.h "YUV input"), independent of the library and written from the
header's text: the coefficients as floor(65536 e + 1/2) of the exact rationals (fractions), the per-pixel integer formula with the
arithmetic shift and the clamp, sample replication of the chroma, and the fused call as the conversion followed by
resample_ref.resample.  convert() and resample() are what the GPU tests compare against, word for word."""
from fractions import Fraction

import numpy as np

import resample_ref

BT709 = 1
FULL_RANGE = 2
LINEAR = resample_ref.LINEAR
# the header's table: flag word -> (cy, crv, cgu, cgv, cbu)
HEADER_TABLE = {0: (76309, 104597, 25675, 53279, 132201), FULL_RANGE: (65536, 91881, 22553, 46802, 116130),
                BT709: (76309, 117489, 13975, 34925, 138438), BT709 | FULL_RANGE: (65536, 103206, 12276, 30679, 121609)}


def rationals(flags):
    """(cy, crv, cgu, cgv, cbu) as exact fractions, and the luma offset yo."""
    kr, kb = (Fraction(2126, 10000), Fraction(722, 10000)) if flags & BT709 else (Fraction(299, 1000), Fraction(114, 1000))
    kg = 1 - kr - kb
    sy, sc = (Fraction(1), Fraction(1)) if flags & FULL_RANGE else (Fraction(255, 219), Fraction(255, 224))
    return (sy, sc * 2 * (1 - kr), sc * 2 * (1 - kb) * kb / kg, sc * 2 * (1 - kr) * kr / kg, sc * 2 * (1 - kb)), (0 if flags & FULL_RANGE else 16)


def coefficients(flags):
    """floor(65536 e + 1/2) of the rationals, as Python ints, and yo."""
    es, yo = rationals(flags)
    return tuple(int((65536 * e + Fraction(1, 2)).__floor__()) for e in es), yo


def pixel(Y, U, V, flags):
    """The three channels of int64 arrays Y, U, V (0..255) by the integer formula: (R, G, B) int64 arrays in 0..255."""
    (cy, crv, cgu, cgv, cbu), yo = coefficients(flags)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    l = cy * (Y - yo) + 32768
    u, v = U - 128, V - 128
    r = (l + crv * v) >> 16                             # numpy's >> on signed integers is the arithmetic shift
    g = (l - cgu * u - cgv * v) >> 16
    b = (l + cbu * u) >> 16
    assert max(int(np.abs(l).max()), int(np.abs(l + crv * v).max()), int(np.abs(l - cgu * u - cgv * v).max()),
               int(np.abs(l + cbu * u).max())) < 36_000_000
    return tuple(np.clip(c, 0, 255) for c in (r, g, b))


def exact(Y, U, V, flags):
    """Round-half-up of the exact real formula, in float64: (R, G, B) int64 arrays in 0..255."""
    es, yo = rationals(flags)
    cy, crv, cgu, cgv, cbu = (float(e) for e in es)
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    l, u, v = cy * (Y - yo), U - 128.0, V - 128.0
    return tuple(np.clip(np.floor(c + 0.5), 0, 255).astype(np.int64) for c in (l + crv * v, l - cgu * u - cgv * v, l + cbu * u))


def convert_one(y, u, v, flags):
    """One frame: y (h, w), u and v ((h + 1) // 2, (w + 1) // 2) uint8 arrays (any strides) -> int32 ARGB array (h, w)."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    h, w = y.shape
    assert u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    rows, cols = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    r, g, b = pixel(y, u[rows, cols], v[rows, cols], flags)
    word = np.int64(0xFF) << 24 | r << 16 | g << 8 | b
    return word.astype(np.uint32).view(np.int32)


def convert(frames, flags=0):
    """n frames (y, u, v) -> list of int32 ARGB arrays."""
    return [convert_one(y, u, v, flags) for y, u, v in frames]


def resample(frames, size=None, crop=None, flags=0, resample_flags=LINEAR):
    """The fused call: the conversion followed by the frame reduction with the same crop, target and flags."""
    return resample_ref.resample(convert(frames, flags), size, crop, resample_flags)


def random_planes(w, h, seed):
    """(y, u, v) of random bytes, tight."""
    rng = np.random.default_rng(seed)
    ch2, cw2 = (h + 1) // 2, (w + 1) // 2
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch2, cw2), dtype=np.uint8),
            rng.integers(0, 256, (ch2, cw2), dtype=np.uint8))
