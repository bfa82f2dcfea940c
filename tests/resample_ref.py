"""Numpy restatement of the frame reduction (include/nquant_abi.h "frame reduction"), independent of the library: the two
weight matrices Wy (dh x ch) and Wx (dw x cw) of overlap lengths, the premultiplied table values summed as Wy @ P @ Wx^T in uint64 (every
sum stays below 2^56), the two kinds of division and the nearest-table-entry search.  resample() is what the GPU tests compare against,
word for word.  The linear-light table is read from include/nq_srgb_linear_16.inc, the normative copy; it is not recomputed here."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FILE = os.path.join(ROOT, "include", "nq_srgb_linear_16.inc")
LINEAR = 1


def linear_table():
    """The 256 entries of the committed table file (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(TABLE_FILE).read(), flags=re.S)
    return np.array([int(v) for v in re.findall(r"\d+", text)], np.uint64)


def table(flags):
    return linear_table() if flags & LINEAR else np.arange(256, dtype=np.uint64) * np.uint64(257)


def weights(src, dst):
    """(dst x src) uint64: [x, j] = the length of the overlap of [x src, (x + 1) src) and [j dst, (j + 1) dst)."""
    x = np.arange(dst, dtype=np.int64)[:, None]
    j = np.arange(src, dtype=np.int64)[None, :]
    w = np.minimum((x + 1) * src, (j + 1) * dst) - np.maximum(x * src, j * dst)
    return np.maximum(w, 0).astype(np.uint64)


def footprint(x, src, dst):
    """First and last source cell with a nonzero weight for output cell x."""
    return x * src // dst, ((x + 1) * src - 1) // dst


def encode(t, T):
    """The smallest v with 2 t <= T[v] + T[v + 1], 255 if there is none (t: uint64 array)."""
    mids = T[:-1] + T[1:]                               # 255 increasing thresholds
    return np.searchsorted(mids, 2 * t, side="left").astype(np.uint64)      # = the number of v with T[v] + T[v + 1] < 2 t


def resample_one(frame, crop, size, flags):
    """One frame (2-D int32/uint32 ARGB) -> int32 array of shape (dh, dw)."""
    cx, cy, cw, ch = crop
    dw, dh = size
    assert 1 <= dw <= cw and 1 <= dh <= ch
    px = np.ascontiguousarray(frame).view(np.uint32)[cy:cy + ch, cx:cx + cw].astype(np.uint64)
    assert px.shape == (ch, cw)
    T = table(flags)
    a = px >> np.uint64(24)
    Wy, Wx = weights(ch, dh), weights(cw, dw)
    W = np.uint64(cw * ch)
    S_a = Wy @ a @ Wx.T
    out = np.zeros((dh, dw), np.uint64)
    nz = S_a != 0
    den = np.where(nz, S_a, np.uint64(1))
    out |= ((np.uint64(2) * S_a + W) // (np.uint64(2) * W)) << np.uint64(24)
    for shift in (16, 8, 0):
        S_c = Wy @ (T[((px >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)] * a) @ Wx.T
        t = (np.uint64(2) * S_c + den) // (np.uint64(2) * den)
        out |= encode(t, T) << np.uint64(shift)
    return np.where(nz, out, np.uint64(0)).astype(np.uint32).view(np.int32)


def resample(frames, size=None, crop=None, flags=LINEAR):
    """n frames of one size -> list of int32 arrays; crop None: the whole frame, size None: the crop's size."""
    h, w = np.asarray(frames[0]).shape
    crop = (0, 0, w, h) if crop is None else tuple(int(v) for v in crop)
    size = crop[2:] if size is None else tuple(int(v) for v in size)
    return [resample_one(f, crop, size, flags) for f in frames]


def random_argb(w, h, seed, p_clear=0.2, p_opaque=0.3):
    """Random ARGB words with a seeded share of a = 0 and a = 255 pixels."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**32, (h, w), dtype=np.uint64).astype(np.uint32)
    u = rng.random((h, w))
    v = np.where(u < p_clear, v & np.uint32(0x00FFFFFF), v)
    v = np.where(u > 1 - p_opaque, v | np.uint32(0xFF000000), v)
    return v.astype(np.uint32).view(np.int32)
