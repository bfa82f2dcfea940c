"""The cases of the WebP tests (test_webp_cpu.py, test_gpu_webp.py): cases(), the smallest shapes at which the encoder can still go
wrong, and limit_cases(), the smallest at which it reaches its chain, grid and bit-writer limits.  Every case is (name, frames,
palette, keywords of webp_ref.encode); the index maps and the restatement's file are made once."""
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


# ---- the limit cases: each reaches one of the encoder's limits (DESIGN.md "WebP encoder", the limit cases); test_webp_cpu.py asserts
# from the restatement's statistics that it does ----
def _with_repeats(a, rng, count, longest):
    """Noise `a` with `count` stretches of up to `longest` pixels repeated from earlier in the same row-major order."""
    flat = a.reshape(-1)
    for _ in range(count):
        n = int(rng.integers(3, longest + 1))
        dst = int(rng.integers(n, flat.size - n))
        src = int(rng.integers(0, dst - n + 1))
        flat[dst:dst + n] = flat[src:src + n]
    return a


def _far_copy_map():
    """One band of 32768 packed pixels whose last three repeat its first three; the constant between them keeps to one hash bucket,
    so the head table still names position 0 at position 32765."""
    v = np.full(512 * 64, 7, np.int64)
    v[:3] = v[-3:] = (201, 33, 118)
    return v.reshape(64, 512)


# distance prefix symbols 15 .. 28 of the markers of _wide_items_map: (smallest distance, largest distance, copies, markers)
_MARKER_CLASSES = [(73, 136, 987, 4), (137, 264, 610, 4), (265, 392, 377, 5), (393, 648, 233, 5), (649, 904, 144, 4), (905, 1416, 89, 3),
                   (1417, 1928, 55, 3), (1929, 2952, 34, 3), (2953, 3976, 21, 3), (3977, 6024, 13, 3), (6025, 8072, 8, 2),
                   (8073, 12168, 5, 3), (12169, 16264, 3, 2), (16265, 24456, 2, 2)]


def _wide_items_map(seed=15, lead=1, filler=760, a=3, b=17, width=256, rows=128):
    """One band of 32768 packed pixels in which both codes of a copy are deep and the extra bits many.  As in _fibonacci_map, runs of
    a and b alternate and their lengths give the green code Fibonacci weights.  Between the runs stand markers: three literals that
    come back at a chosen distance (before a run of the other value than last time, so that the copy stays 3 long); marker classes
    with Fibonacci counts fill the distance prefixes 15 .. 28.  Three blocks (a marker, then two runs) come back whole: 258 pixels
    (the length prefix with 7 extra bits) at a distance of prefix 29 (13 extra bits), 203 and 153 pixels at prefixes 27 and 28; and
    one marker of the first pixels comes back in the last ones: prefix 30 (14 extra bits).  `lead` literals in front shift the items
    against the words, `filler` runs of 6 fill the band.  What the parse makes of all this is measured, not planned: the defaults are
    the best of a search over seeds, and test_webp_cpu.py asserts what they reach."""
    rng = np.random.default_rng(seed)
    L = width * rows
    lens = [4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193]
    weights = [610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2]
    runs = []
    for l, w in zip(lens, weights):
        runs += [3 + l] * w
    runs += [6] * filler                                                    # two copies of 3 each: they fill the band
    rng.shuffle(runs)
    runs = [4, 4] + [int(r) for r in runs]
    values = [int(v) for v in rng.permutation(np.arange(50, 250))]          # every marker has three pixel values of its own
    triples = [tuple(values[3 * k:3 * k + 3]) for k in range(len(values) // 3)]
    markers = []                                                            # [lo, hi, period, copies left, last position, triple, what followed]
    for lo, hi, copies, count in _MARKER_CLASSES:
        for k in range(count):
            n = copies // count + (1 if k < copies % count else 0)
            markers.append([lo, hi, lo + (hi - lo) // 4, n, None, triples.pop(), None])
    far = triples.pop()
    blocks = []                                                             # [pixels, smallest distance, first position, done]
    out = [250] * lead + list(far)
    for na, nb, lo in ((70, 80, 16265), (90, 110, 12169), (120, 135, 24457)):   # 153, 203 and 258 pixels: 6, 6 and 7 extra bits of length
        blocks.append([list(triples.pop()) + [a] * na + [b] * nb, lo, len(out), False])
        out += blocks[-1][0]
    last = b

    def marker(m, follower):
        m[4], m[6] = len(out), follower
        out.extend(m[5])

    for r in runs:
        nxt = a if last == b else b
        for m in reversed(markers):                                         # at most one between two runs (a copy ends with its marker), the rare first
            if m[4] is None:
                marker(m, nxt)
                break
            if m[3] and m[6] != nxt and (len(out) - m[4] >= m[2] or len(out) + r - m[4] > m[1] - 8) and len(out) - m[4] >= m[0]:
                m[3] -= 1
                marker(m, nxt)
                break
        for k in blocks:
            if not k[3] and len(out) - k[2] >= k[1] + 600:
                out += k[0]
                k[3] = True
                last = b
                break
        last = a if last == b else b
        out += [last] * r
    room = L - 3 - len(out)
    assert room >= 0 and all(k[3] for k in blocks), room
    while room >= 6:
        last = a if last == b else b
        out += [last] * 6
        room -= 6
    out += [49] * room + list(far)
    return np.array(out, np.int64).reshape(rows, width)


def _rows_from_a_pool(h, w, K, rng, pool=5):
    """Every row is one of `pool` noise rows: bands repeat rows (copies one packed row back) and repeat each other (the chains one
    workgroup takes in turn hold the same triples at other places)."""
    return rng.integers(0, K, (pool, w))[rng.integers(0, pool, h)]


def _delta_frames(n, h, w, K, rng):
    """Frames of which each changes one rectangle of the one before: narrow, medium and wide ones in turn, a few as tall as the frame,
    so that the images of one call have different band heights and band counts."""
    frames = [rng.integers(0, K, (h, w))]
    for i in range(1, n):
        rw = int(rng.integers(*((2, 21), (65, 81), (129, w))[i % 3]))
        rh = h if i % 50 == 7 else int(rng.integers(1, 5))
        x, y = int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))
        f = frames[-1].copy()
        new = rng.integers(0, K, (rh, rw)) if i % 2 else np.tile(rng.integers(0, K, (1, 5)), (rh, rw // 5 + 1))[:, :rw]
        f[y:y + rh, x:x + rw] = new
        f[y, x] = (frames[-1][y, x] + 1) % K                                # the corners do change
        f[y + rh - 1, x + rw - 1] = (frames[-1][y + rh - 1, x + rw - 1] + 1) % K
        frames.append(f)
    return frames


@functools.lru_cache(maxsize=None)
def limit_cases():
    rng = np.random.default_rng(4242)
    out = []
    out.append(("full_chain_K17", [_with_repeats(rng.integers(0, 17, (5, 8192)), rng, 300, 300)], palette_of(17, rng), {"band_bits": 2}))
    out.append(("full_chain_K16", [_with_repeats(rng.integers(0, 16, (9, 16384)), rng, 600, 600)], palette_of(16, rng), {}))
    out.append(("far_copy", [_far_copy_map()], palette_of(256, rng), {}))
    out.append(("wide_items", [_wide_items_map()], palette_of(256, rng), {}))
    out.append(("many_bands_K2", [_rows_from_a_pool(4100, 64, 2, rng)], palette_of(2, rng), {"band_bits": 2}))
    out.append(("many_bands_K256", [_rows_from_a_pool(4100, 8, 256, rng)], palette_of(256, rng), {"band_bits": 2}))
    pool = [rng.integers(0, 256, (64, 64)) for _ in range(6)]
    out.append(("many_frames", [pool[i] for i in rng.integers(0, 6, 1100)], palette_of(256, rng),
                {"delays_cs": [int(d) for d in rng.choice([0, 1, 4, 10, 65535], 1100)], "loop": 2, "band_bits": 4, "delta": False}))
    out.append(("many_frames_delta", _delta_frames(300, 132, 136, 256, rng), palette_of(256, rng, alpha=True),
                {"delays_cs": [int(d) for d in rng.choice([0, 2, 7], 300)], "loop": 0, "delta": True}))
    return out


def limit_names():
    return [c[0] for c in limit_cases()]


def names():
    return [c[0] for c in cases()] + limit_names()


def case(name):
    return next(c for c in cases() + limit_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(file, per frame [webp_ref.Band, which equals (literals, copies)] per band) of the restatement."""
    import webp_ref
    _, frames, pal, kw = case(name)
    stats = []
    return webp_ref.encode(frames, pal, stats=stats, **kw), stats
