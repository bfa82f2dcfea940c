"""The ordered dither of include/nquant_abi.h ("ordered dither") restated in numpy: a brute-force distance matrix, the two smallest
keys (d << 8) | index per pixel, the mask value at the pixel's coordinates and the inequality.  Written from the definition; the
reference project has no such step."""
import os
import re

import numpy as np

CHUNK = 1 << 14          # pixels per distance matrix
HERE = os.path.dirname(os.path.abspath(__file__))


def load_mask():
    """The committed 64 x 64 mask as int64 values -128..127, row-major."""
    text = open(os.path.join(HERE, "..", "include", "nq_blue_noise_64x64.inc")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    v = np.array([int(t) for t in text.replace("\n", " ").split(",") if t.strip()], np.int64)
    assert v.size == 4096
    return v.reshape(64, 64)


MASK = load_mask()


def _channels(v):
    v = np.asarray(v).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    return np.stack([(v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1)


def _dist(p, c):
    """d[i][j] of pixel i and entry j ((n, 4) and (m, 4) channel arrays), int64.  Expanded to |p|^2 + |c|^2 - 2 p.c so that the product
    is one float64 matrix multiplication: every term is an integer below 2^20, exact."""
    pf, cf = p.astype(np.float64), c.astype(np.float64)
    return ((pf * pf).sum(axis=1)[:, None] + (cf * cf).sum(axis=1)[None, :] - 2.0 * (pf @ cf.T)).astype(np.int64)


def first_transparent(palette):
    a = _channels(palette)[:, 0]
    z = np.flatnonzero(a == 0)
    return int(z[0]) if z.size else -1


def dither_frame(frame, palette, limit):
    """(index map as uint16, ARGB output as uint32, pixels that took i2, squared error of the counted pixels) of one 2-D frame."""
    frame = np.asarray(frame)
    h, w = frame.shape
    pal_words = (np.asarray(palette).reshape(-1).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    pal = _channels(pal_words)
    live = np.flatnonzero(pal[:, 0] != 0)
    T = first_transparent(pal_words)
    px = _channels(frame.reshape(-1).view(np.uint32) if frame.dtype == np.int32 else frame.reshape(-1))
    n = px.shape[0]
    counted = (px[:, 0] != 0) | (T < 0)
    ys, xs = np.divmod(np.arange(n, dtype=np.int64), w)
    m = MASK[ys & 63, xs & 63] + 128
    taken = np.full(n, max(T, 0), np.int64)
    mixed = 0
    if live.size:
        lp = pal[live]
        for s in range(0, n, CHUNK):
            p = px[s:s + CHUNK]
            rows = np.arange(p.shape[0])
            d = _dist(p, lp)
            key = (d << 8) | live[None, :]
            j1 = key.argmin(axis=1)
            i1, d1 = live[j1], d[rows, j1]
            pick = i1
            if live.size > 1 and limit > 0:
                key[rows, j1] = np.int64(1) << 62
                j2 = key.argmin(axis=1)
                i2, d2 = live[j2], d[rows, j2]
                delta = d2 - d1
                assert (delta >= 0).all()
                den = ((pal[i1] - pal[i2]) ** 2).sum(axis=1)
                far = np.abs(pal[i1] - pal[i2]).max(axis=1)
                mix = (far <= limit) & ((255 - 2 * m[s:s + CHUNK]) * den > 256 * delta)
                pick = np.where(mix, i2, i1)
                mixed += int((mix & counted[s:s + CHUNK]).sum())
            c = counted[s:s + CHUNK]
            taken[s:s + CHUNK][c] = pick[c]
    err = int(((px[counted] - pal[taken[counted]]) ** 2).sum())
    return taken.astype(np.uint16).reshape(h, w), pal_words[taken].reshape(h, w), mixed, err


def dither(frames, palette, limit):
    """(index maps, ARGB outputs, stats as an (n, 2) int64 array) of the definition over a sequence of 2-D frames."""
    idx, out, stats = [], [], np.zeros((len(frames), 2), np.int64)
    for i, f in enumerate(frames):
        a, b, stats[i, 0], stats[i, 1] = dither_frame(f, palette, limit)
        idx.append(a)
        out.append(b)
    return idx, out, stats
