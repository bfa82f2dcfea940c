"""Restatement of the retiming (include/nquant_abi.h "retiming"), independent of the library: plan() is nq_retime_plan in
Python integers (which do not overflow), mix() is nq_retime_frames in numpy uint64 (every sum stays below 2^55; the numerators of the
divisions below 2^57).  mix() is what the GPU tests compare against, word for word.  The linear-light table is read from
include/nq_srgb_linear_16.inc, the normative copy; it is not recomputed here."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FILE = os.path.join(ROOT, "include", "nq_srgb_linear_16.inc")
LINEAR = 1
MAX_WINDOW = 64


def linear_table():
    """The 256 entries of the committed table file (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(TABLE_FILE).read(), flags=re.S)
    return np.array([int(v) for v in re.findall(r"\d+", text)], np.uint64)


def table(flags):
    return linear_table() if flags & LINEAR else np.arange(256, dtype=np.uint64) * np.uint64(257)


def cs(x):
    """R(x): microseconds to the nearest centisecond, halves up."""
    return (x + 5000) // 10000


def plan(t_us, period, shutter):
    """(m, offset, source, weight, delays_cs) as lists of Python ints.  Every output's window is intersected with EVERY source interval:
    no walk, no state."""
    t = [int(v) for v in t_us]
    n = len(t) - 1
    assert n >= 1 and all(b > a for a, b in zip(t[:-1], t[1:])) and 1 <= shutter <= period
    D = t[n] - t[0]
    m = max(1, (2 * D + period) // (2 * period))
    offset, source, weight, delays = [0], [], [], []
    for j in range(m):
        lo = t[0] + j * period
        hi = min(lo + shutter, t[n])
        for i in range(n):
            w = min(t[i + 1], hi) - max(t[i], lo)
            if w > 0:
                source.append(i)
                weight.append(w)
        offset.append(len(source))
        delays.append(cs(D if j + 1 == m else (j + 1) * period) - cs(j * period))
    return m, offset, source, weight, delays


def encode(t, T):
    """The smallest v with 2 t <= T[v] + T[v + 1], 255 if there is none (t: uint64 array)."""
    mids = T[:-1] + T[1:]
    return np.searchsorted(mids, 2 * t, side="left").astype(np.uint64)


def mix(frames, m, offset, source, weight, flags=LINEAR):
    """n frames of one size (2-D int32/uint32 ARGB) and any plan -> list of m int32 arrays."""
    T = table(flags)
    px = [np.ascontiguousarray(f).view(np.uint32).astype(np.uint64) for f in frames]
    two = np.uint64(2)
    outs = []
    for j in range(m):
        pairs = range(int(offset[j]), int(offset[j + 1]))
        assert 1 <= len(pairs) <= MAX_WINDOW
        W = sum(int(weight[k]) for k in pairs)
        assert 1 <= W <= 2**31 - 1
        S = [np.zeros(px[0].shape, np.uint64) for _ in range(4)]
        for k in pairs:
            p, w = px[int(source[k])], np.uint64(int(weight[k]))
            a = p >> np.uint64(24)
            S[0] += w * a
            for q, shift in enumerate((16, 8, 0)):
                S[1 + q] += w * (a * T[((p >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)])
        nz = S[0] != 0
        den = np.where(nz, S[0], np.uint64(1))
        out = ((two * S[0] + np.uint64(W)) // (two * np.uint64(W))) << np.uint64(24)
        for q, shift in enumerate((16, 8, 0)):
            out |= encode((two * S[1 + q] + den) // (two * den), T) << np.uint64(shift)
        outs.append(np.where(nz, out, np.uint64(0)).astype(np.uint32).view(np.int32))
    return outs


def random_argb(w, h, seed, p_clear=0.2, p_opaque=0.3):
    """Random ARGB words with a seeded share of a = 0 and a = 255 pixels."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**32, (h, w), dtype=np.uint64).astype(np.uint32)
    u = rng.random((h, w))
    v = np.where(u < p_clear, v & np.uint32(0x00FFFFFF), v)
    v = np.where(u > 1 - p_opaque, v | np.uint32(0xFF000000), v)
    return v.astype(np.uint32).view(np.int32)


def variable_timestamps(n, seed, lo=1, hi=10_000_000, start=None):
    """n + 1 timestamps with log-uniform durations in lo..hi microseconds and a seeded (possibly negative) start."""
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(np.log(lo), np.log(hi + 1), n)).astype(np.int64).clip(lo, hi)
    t0 = int(rng.integers(-10**9, 10**12)) if start is None else int(start)
    return [t0] + [t0 + int(v) for v in np.cumsum(d)]
