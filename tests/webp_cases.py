"""The cases of the WebP tests (test_webp_cpu.py, test_gpu_webp.py): the smallest shapes at which the encoder can still go wrong.
Every case is (name, frames, palette, keywords of webp_ref.encode); the index maps and the restatement's file are made once."""
import functools

import numpy as np


def palette_of(K, rng, alpha=False):
    pal = (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.uint32)
    if alpha:
        pal[0] &= np.uint32(0x00FFFFFF)                                   # alpha 0, colour bits kept
        if K > 1:
            pal[K // 2] = (pal[K // 2] & np.uint32(0x00FFFFFF)) | np.uint32(0x80000000)
    return pal


def _fibonacci_map(a=3, b=17, width=128):
    """A map whose TOKENS have Fibonacci frequencies (index frequencies cannot: the parse turns every frequent index into copies).
    Runs of a and b alternate; a run of 3 + l pixels, l >= 3, parses as a copy of 3 from the last run of its value and a copy of l at
    distance 1.  So the green code sees the two literals once each, the length prefixes of l = 4, 5, 7, 9, 13, ... 257 with the
    weights 987, 610, ... 2, and the prefix of length 3 above them all: a chain 16 deep, which the limiter cuts to 15.  One band."""
    lens = [4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257]
    weights = [987, 610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2]
    runs = []
    for l, w in zip(lens, weights):
        runs += [3 + l] * w
    np.random.default_rng(7).shuffle(runs)
    runs = [4, 4] + [int(r) for r in runs]                                  # the two literals, each with a copy of 3
    rows = -(-sum(runs) // width)
    rest = rows * width - sum(runs)
    runs += [6] * (rest // 6)                                               # two copies of 3 each
    runs[runs.index(3 + 33)] += rest % 6                                    # (stays in the class 33..48)
    v = np.concatenate([np.full(r, a if k % 2 == 0 else b, np.int64) for k, r in enumerate(runs)])
    return v.reshape(rows, width)                                           # 233 x 128


def _animation(h, w, K, rng):
    """Five frames: a change with its corner at odd x and odd y, an unchanged frame, a change in the last row and column, one pixel."""
    a = rng.integers(0, K, (h, w))
    b = a.copy()
    b[5:12, 7:20] = (a[5:12, 7:20] + 1 + rng.integers(0, K - 1, (7, 13))) % K
    b[5, 7] = (a[5, 7] + 1) % K
    c = b.copy()
    d = c.copy()
    d[h - 1, w - 1] = (c[h - 1, w - 1] + 1) % K
    d[h - 3, w - 9] = (c[h - 3, w - 9] + 1) % K
    e = d.copy()
    e[0, 1] = (d[0, 1] + 1) % K
    return [a, b, c, d, e]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(2024)
    out = []
    for K in (1, 2, 4, 16, 17, 256):
        for w in (1, 7, 9, 13):
            out.append(("K%d_w%d" % (K, w), [rng.integers(0, K, (5, w))], palette_of(K, rng), {}))
    out.append(("one_pixel", [np.zeros((1, 1), np.int64)], palette_of(3, rng), {}))
    out.append(("three_bands", [rng.integers(0, 5, (9, 13)) * (rng.random((9, 13)) < 0.5)], palette_of(17, rng), {"band_bits": 2}))
    out.append(("four_bands", [rng.integers(0, 256, (250, 300))], palette_of(256, rng), {}))
    out.append(("constant", [np.full((40, 64), 9, np.int64)], palette_of(32, rng), {}))
    out.append(("noise", [np.random.default_rng(11).integers(0, 256, (48, 64))], palette_of(256, rng), {}))
    out.append(("fibonacci", [_fibonacci_map()], palette_of(21, rng), {}))
    out.append(("repeated_rows", [np.tile(rng.integers(0, 200, (1, 150)), (60, 1))], palette_of(200, rng), {}))
    out.append(("alpha_palette", [rng.integers(0, 6, (21, 33))], palette_of(6, rng, alpha=True), {}))
    for (h, w), K, alpha, delays, loop in (((40, 48), 17, False, [0, 65535, 3, 1, 2], 0), ((37, 45), 4, True, [7, 0, 65535, 5, 1], 3),
                                           ((37, 45), 200, False, None, 3)):
        frames = _animation(h, w, K, rng)
        for delta in (True, False):
            out.append(("anim_%dx%d_K%d_%s" % (w, h, K, "delta" if delta else "whole"), frames if delta else frames[:3],
                        palette_of(K, rng, alpha), {"delays_cs": delays if delta or delays is None else delays[:3], "loop": loop, "delta": delta}))
    return out


def names():
    return [c[0] for c in cases()]


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(file, per frame [(literals, copies)] per band) of the restatement."""
    import webp_ref
    _, frames, pal, kw = case(name)
    stats = []
    return webp_ref.encode(frames, pal, stats=stats, **kw), stats
