"""Numpy restatement of the quality measurement (include/nquant_abi.h "quality measurement"), independent of the library:
the seen colour, the per-pixel squared error, the 8 x 8 block means through the premultiplied table values, and the block SSIM on
luma with its two floor divisions, all in int64.  compare() is what the GPU tests compare against, slot for slot.  The table is read
through resample_ref.table(flags): the committed include/nq_srgb_linear_16.inc, not recomputed here."""
import numpy as np

import resample_ref

LINEAR = 1
SLOTS = 16
PIXELS, BLOCKS, SSE, MAXDIFF, LF, SSIM, DEFICIT = 0, 1, 2, 6, 7, 11, 12
ONE = 32768


def _channels(frame):
    """(a, r, g, b) of a 2-D frame of ARGB words as int64 planes, with the seen colour: a = 0 makes r = g = b = 0."""
    v = np.ascontiguousarray(frame).view(np.uint32).astype(np.int64)
    a = (v >> 24) & 255
    seen = a != 0
    return [a] + [np.where(seen, (v >> s) & 255, 0) for s in (16, 8, 0)]


def _block_sums(plane):
    """Sums of a 2-D int64 plane over the 8 x 8 blocks anchored at (0, 0); edge blocks are partial."""
    h, w = plane.shape
    rows = np.add.reduceat(plane, np.arange(0, h, 8), axis=0)
    return np.add.reduceat(rows, np.arange(0, w, 8), axis=1)


def _premultiplied(ch, T):
    a = ch[0]
    return [257 * a] + [(T[c] * a + 127) // 255 for c in ch[1:]]


def _luma(ch):
    a, r, g, b = ch
    y = (77 * r + 150 * g + 29 * b + 128) >> 8
    return (y * a + 127) // 255


def compare(src, out, flags=LINEAR):
    """The 16 slots of one pair of 2-D frames (int32 or uint32 ARGB words), int64."""
    src, out = np.asarray(src), np.asarray(out)
    assert src.ndim == 2 and src.shape == out.shape
    h, w = src.shape
    T = resample_ref.table(flags).astype(np.int64)
    s, o = _channels(src), _channels(out)
    res = np.zeros(SLOTS, np.int64)
    N = _block_sums(np.ones((h, w), np.int64))
    res[PIXELS], res[BLOCKS] = h * w, N.size
    for c in range(4):
        d = s[c] - o[c]
        res[SSE + c] = (d * d).sum()
        res[MAXDIFF] = max(res[MAXDIFF], np.abs(d).max())
    for c, (p, q) in enumerate(zip(_premultiplied(s, T), _premultiplied(o, T))):
        m = (2 * _block_sums(p) + N) // (2 * N)
        m2 = (2 * _block_sums(q) + N) // (2 * N)
        res[LF + c] = ((m - m2) ** 2).sum()
    x, y = _luma(s), _luma(o)
    Sx, Sy, Sxx, Syy, Sxy = (_block_sums(v) for v in (x, y, x * x, y * y, x * y))
    C1 = (65025 * N * N + 5000) // 10000
    C2 = (585225 * N * N + 5000) // 10000
    A1 = 2 * Sx * Sy + C1
    B1 = Sx * Sx + Sy * Sy + C1
    A2 = 2 * (N * Sxy - Sx * Sy) + C2
    B2 = N * (Sxx + Syy) - Sx * Sx - Sy * Sy + C2
    assert (B1 > 0).all() and (B2 > 0).all() and max(A1.max(), B1.max(), np.abs(A2).max(), B2.max()) < 1 << 30
    l = (ONE * A1) // B1                    # numpy's // rounds toward minus infinity, as the definition does
    cs = (ONE * A2) // B2
    q = (l * cs) // ONE
    res[SSIM] = q.sum()
    res[DEFICIT] = (ONE - q).max()
    return res


def compare_frames(src_frames, out_frames, flags=LINEAR):
    """(n, 16) int64: one row of slots per pair."""
    return np.stack([compare(s, o, flags) for s, o in zip(src_frames, out_frames)])


def compare_indexed(src_frames, index_maps, palette, flags=LINEAR):
    """The indexed form: the output word is palette[index], word 0 for an index >= K."""
    pal = (np.asarray(palette).reshape(-1).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    padded = np.zeros(65536, np.uint32)
    padded[:pal.size] = pal
    return compare_frames(src_frames, [padded[np.asarray(m).astype(np.int64)] for m in index_maps], flags)
