"""The limit cases of the PNG and APNG tests (test_png_cpu.py, test_gpu_png.py, test_gpu_apng.py): the smallest index maps at which the
deflate chain of png_deflate_kernel reaches its limiters, its bit writer's third word, the edges of its distance window, match lengths
and run-length coder, the extremes of the block header, every kind of in-step hash group and a workgroup's later segments (DESIGN.md
5c, "limit cases").  Every case is (name, index map, palette, segment_bytes); the maps and the restatement's files are made once.
What a case reaches is measured, not planned: test_png_cpu.py asserts it from the statistics of png_ref.encode(stats=...)."""
import functools

import numpy as np

import png_ref

LENS = [4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 255]             # one match length in each of 14 length symbols, 261 .. 284
FIB3 = [1830, 1131, 699, 432, 267, 165, 102, 63, 39, 24, 15, 9, 6, 3]      # 3 x Fibonacci


def palette_of(K, rng, alpha=False):
    pal = (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.uint32)
    if alpha:
        pal[0] &= np.uint32(0x00FFFFFF)
        pal[K // 2] = (pal[K // 2] & np.uint32(0x00FFFFFF)) | np.uint32(0x80000000)
    return pal


def _runs_map(runs, a=0, b=17):
    """One row in which runs of a and of b alternate."""
    return np.concatenate([np.full(r, a if k % 2 == 0 else b, np.int64) for k, r in enumerate(runs)]).reshape(1, -1)


def _len_limit_map(seed=7, lens=LENS, counts=FIB3):
    """Runs of index 0 and index 17 alternate (the row's filter byte joins the first run).  A run of 3 + l pixels parses as a match of 3
    from the last run of its value and a match of l at distance 1, so the length symbols of l = 4, 5, 7, ... 255 get the counts 3 x
    Fibonacci and the symbol of length 3 the sum of them all: one chain over 257 .. 284, 17 deep without the limit.  (With plain
    Fibonacci counts the three symbols of count 1 split the tree into two chains and the depth stays at 10.)"""
    runs = []
    for l, c in zip(lens, counts):
        runs += [3 + l] * c
    np.random.default_rng(seed).shuffle(runs)
    return _runs_map([4, 4] + [int(r) for r in runs])


def _far_edge_map(D, n=40000):
    """One row of 7s; pixels 0..2 come back at pixel D.  The constant between keeps to one hash bucket, so the head table still names
    the first triple when the second arrives: D = 32768 is a match of 258 at the window's edge, D = 32769 is none."""
    v = np.full(n, 7, np.int64)
    v[:3] = v[D:D + 3] = (201, 33, 118)
    return v.reshape(1, n)


MATCH_EDGES_S = 5000


def _match_edges_map():
    """Three segments of 5000, 5000 and 40 bytes of one row.  Segment 0: a run of 258 (a literal and a match of exactly 257: symbol
    284, extra value 30), a run of 260 (a match of 258: symbol 285), noise, and a run of 9s that goes on for 100 bytes on either side
    of the segment's end, so that L - m cuts the match below its natural length and the compare meets the zero padding.  Segments 1 and
    2 end in three pixels seen before, after other pixels: a match of 3 that ends on the segment's last byte."""
    rng = np.random.default_rng(21)
    S = MATCH_EDGES_S
    raw = rng.integers(100, 200, 2 * S + 40)                                # the raw stream; byte 0 becomes the filter byte
    raw[10:268] = 200
    raw[300:560] = 201
    raw[S - 100:S + 100] = 9
    raw[2 * S - 40:2 * S - 37] = (1, 2, 3)
    raw[2 * S - 3:2 * S] = (1, 2, 3)
    raw[2 * S + 5:2 * S + 8] = (4, 5, 6)
    raw[2 * S + 37:2 * S + 40] = (4, 5, 6)
    return raw[1:].reshape(1, -1)


# ---- blocks of literals with planned code lengths ----
def _dyadic_map(lens, seed_from=0):
    """One row whose block has no match and gives literal s the code length lens[s] (lens[256]: the end-of-block symbol's, the
    longest; lens[0] > 0: the filter byte).  The Kraft sum of lens is 1, and symbol s stands 2^(longest - lens[s]) times in the
    stream, so Huffman's tree has exactly these depths.  The pixels are shuffled until no three bytes come back."""
    top = max(lens)
    assert len(lens) == 257 and lens[256] == top and lens[0] and sum(1 << (top - l) for l in lens if l) == 1 << top
    vals = np.concatenate([np.full((1 << (top - l)) - (s == 0), s, np.int64) for s, l in enumerate(lens[:256]) if l])
    for seed in range(seed_from, seed_from + 2000):
        v = vals.copy()
        np.random.default_rng(seed).shuffle(v)
        idx = v.reshape(1, -1)
        if not any(isinstance(t, tuple) for t in png_ref.tokens_of(png_ref.raw_stream(idx, 256))):
            return idx
    raise AssertionError("no shuffle without a match")


def _clc_limit_lens(seed):
    """Code lengths whose run-length coding has the symbol counts 1, 1, 2, 3, 5, 8, 13, 21, 34, 55 (symbols 18 and 1 -- the distance
    code's one length --, 17, 16, 0 and the lengths 5 .. 9): a chain 9 deep, which the limit of 7 cuts.  Lengths 5, 8 and 9 hold a
    run of 5, 4 and 4 (one plain symbol and a 16), so that 12, 13, 21, 37 and 58 symbols have the lengths 5 .. 9: Kraft sum 1."""
    rng = np.random.default_rng(seed)
    singles = [5] * 7 + [6] * 13 + [7] * 21 + [8] * 33 + [9] * 53            # + the heads of the three runs + the end-of-block 9
    pieces = [[l] for l in singles] + [[5] * 5, [8] * 4, [9] * 4] + [[0]] * 5 + [[0] * 3, [0] * 10, [0] * 98]
    order = rng.permutation(len(pieces))
    lens = [l for i in order for l in pieces[i]] + [9]
    return lens


@functools.lru_cache(maxsize=None)
def _clc_limit_map():
    want = {18: 1, 1: 1, 17: 2, 16: 3, 0: 5, 5: 8, 6: 13, 7: 21, 8: 34, 9: 55}
    for seed in range(100000):
        lens = _clc_limit_lens(seed)
        if not lens[0]:
            continue
        cf = {}
        for s, _, _ in png_ref.run_lengths(lens + [1]):
            cf[s] = cf.get(s, 0) + 1
        if cf == want:
            return _dyadic_map(lens)
    raise AssertionError("no layout")


def _run_edges_a_lens():
    """Zero runs of 11 and 138 (symbol 18 at both ends of its range), 3 and 10 (symbol 17), equal lengths 1 + 3 and 1 + 6 (symbol 16)."""
    lens = [5] + [0] * 11 + [2] + [0] * 138 + [3] + [0] * 3 + [4] + [0] * 10 + [5] + [4] * 4 + [5] * 7
    return lens + [0] * (256 - len(lens)) + [5]


def _run_edges_b_lens():
    """A zero run of 139: 138 and one plain zero.  Sixteen symbols of length 4, among them runs of 3 (plain) and 11 (16 with 6 and 4);
    no match, so HLIT = 257 and HDIST = 1."""
    lens = [4] + [0] * 139 + [4] * 3 + [0] * 2 + [4] * 11
    return lens + [0] * (256 - len(lens)) + [4]


def _run_edges_c_lens():
    """A zero run of 148: 138 and 10."""
    lens = [3] + [0] * 148 + [3] * 6
    return lens + [0] * (256 - len(lens)) + [3]


# ---- copies with planned lengths and distances ----
COPY_LENGTHS = [5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 257]   # one length in each of 17 length symbols, 259 .. 284


def _chain_counts(n, ratio):
    """n counts, falling: 1, 1, 2, 3, 5, 8 from the rare end, then each `ratio` times the one before.  Huffman's tree over counts
    c1 <= c2 <= ... is one chain while c1 + ... + ck <= c(k+2); Fibonacci numbers meet that with nothing to spare, a ratio of 1.7
    leaves 1 - 1 / (1.7 x 0.7) = 16 % for what the parse does to the counts."""
    c = [1, 1, 2, 3, 5, 8]
    while len(c) < n:
        c.append(int(c[-1] * ratio + 0.999))
    return c[:n][::-1]


def _copies_map(n, first_sym, ratio, lengths, seed=0, lead=0, soft=0.25, sep=7, top=255):
    """One row made of markers that come back at planned distances.  A marker is three pixels of its own and a tail of `sep` pixels
    (at least two: between two markers stand only the triples (y, z, sep), (z, sep, sep), (sep, sep, x'), (sep, x', y'), a few per
    marker, so that almost no other triple takes a marker's place in the 8192-entry head table before the marker comes back).
    Class k = 0 .. n-1 is the distance symbol first_sym + k; its markers are lengths[k] long and come back _chain_counts(n, ratio)[k]
    times in all, each time after other pixels than the time before, so that the copy ends with the marker.  The scheduler walks
    the row: of the markers that are at least their class's smallest distance back it takes the one whose largest distance runs out
    first; a marker that it missed gets three new pixels; where none is due it writes three pixels never seen.  `lead` literals in
    front shift the items against the words.  What the parse makes of this is measured: test_png_cpu.py asserts what it reaches."""
    rng = np.random.default_rng(seed)
    counts = _chain_counts(n, ratio)
    total = sum(c * l for c, l in zip(counts, lengths))
    alphabet = list(range(20, top + 1))
    seen = set()

    def triple():
        while True:
            t = tuple(alphabet[i] for i in rng.integers(0, len(alphabet), 3))
            if t not in seen and len(set(t)) == 3:
                seen.add(t)
                return list(t)

    markers = []                     # [smallest distance, largest, wanted distance, copies left, last position, pixels, what followed, not before]
    for k, (c, l) in enumerate(zip(counts, lengths)):
        lo, eb = png_ref.DIST_CODES[first_sym + k]
        hi = lo + (1 << eb) - 1
        lo = max(lo, l)
        nm = max(1, round((lo + soft * (hi - lo)) * c / total))
        while nm * ((total - l) // lo) < c:                                  # a marker can come back only so often
            nm += 1
        d = min(max(nm * total / c, lo + 2), hi - l - 2)
        for j in range(nm):
            markers.append([lo, hi, d, c // nm + (1 if j < c % nm else 0), None, triple() + [sep] * (l - 3), None, int(j / nm * min(d, 3000))])
    out = [250] * lead
    prev = None                                                              # the marker written last: what follows it is decided now
    while any(m[3] for m in markers) and len(out) < 65534 - 3:
        pos = len(out)
        best = early = None
        for m in markers:
            if not m[3] or pos + len(m[5]) > 65534 or (prev is not None and prev[6] == m[5][0]):
                continue
            if m[4] is None:
                if pos < m[7]:
                    continue
                key = m[7] + 30 + 0.3 * m[0]
            else:
                dist = pos - m[4]
                if dist > m[1]:                                              # missed: it starts again as a new marker
                    m[4], m[7], m[5][:3] = None, pos, triple()
                    continue
                if dist < m[0]:
                    continue
                if dist < 0.97 * m[2]:
                    if early is None or m[4] + m[2] < early[0]:
                        early = (m[4] + m[2], m)
                    continue
                key = m[4] + m[1]
            if best is None or key < best[0]:
                best = (key, m)
        best = best or early
        if best is None:
            t = triple()
            if prev is not None:
                prev[6] = t[0]
            prev = None
            out += t
            continue
        m = best[1]
        if prev is not None:
            prev[6] = m[5][0]
        if m[4] is not None:
            m[3] -= 1
        m[4] = pos
        out += m[5]
        prev = m
    out += [251, 252][:65534 - len(out)]
    return np.array(out, np.int64).reshape(1, -1)


def _dist_limit_map():
    """Eighteen distance symbols, 12 .. 29, every marker five pixels: the distance code's tree is 16 deep without the limit.  No index
    above 254, so the map also fits a palette of 255 (APNG's mark mode)."""
    return _copies_map(18, 12, 1.7, [5] * 18, top=254)


def _wide_items_map(seed=2, lead=4):
    """Seventeen distance symbols, 13 .. 29, and with them seventeen length symbols: the rarest copy is 257 pixels (5 extra bits) from
    24577 or more pixels back (13 extra bits).  seed and lead are the best of a search over four seeds and six leads: a longest item
    of 43 bits, three items that reach the third word of the emit window (test_png_cpu.py asserts it)."""
    return _copies_map(17, 13, 1.7, COPY_LENGTHS, seed, lead, top=255)


def _header_max_map(seed=0, m=7):
    """HLIT = 286, HDIST = 30 and HCLEN = 19 in one block: the chain of _len_limit_map with one length in each of the symbols 258 .. 270
    and 285 (a run of 3 + 258) and counts m x Fibonacci -- the literals 0 and 17 and the end-of-block symbol weigh 4 together, and a
    chain whose two rarest counts are m stays one chain while what lies below weighs no more than m --, so that a length of 15 is in
    use; and the three bytes (17, 0, 17), which stand nowhere else, twice and more than 24576 bytes apart: distance symbol 29."""
    fib = [377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1, 1]
    lens = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 258]
    runs = []
    for l, f in zip(lens, fib):
        runs += [3 + l] * (m * f)
    np.random.default_rng(seed).shuffle(runs)
    runs = [4, 4] + [int(r) for r in runs]
    at, total = [], 0
    for k, r in enumerate(runs):
        if k % 2 == 0 and k >= 2 and len(at) < 2 and (not at or total - at[0][1] >= 24700):
            at.append((k, total))
        total += r
    for k, _ in reversed(at):
        runs[k:k] = [1, 1, 2]                                               # 17, 0, 17 17 after a run of 0
    return _runs_map(runs)


# ---- a workgroup's later segments ----
POOL_W, POOL_ROWS, POOL_S = 1023, 4, 4096                                    # a row is 1024 bytes, a segment four rows


def _pool_blocks():
    rng = np.random.default_rng(99)
    n = POOL_W * POOL_ROWS
    noise = rng.integers(0, 256, n)
    flat = np.full(n, 5, np.int64)
    runs = []
    for l, c in zip(LENS[:8], (55, 34, 21, 13, 8, 5, 3, 2)):
        runs += [3 + l] * c
    rng.shuffle(runs)
    fib = _runs_map([4, 4] + [int(r) for r in runs], 3, 17).reshape(-1)
    fib = np.concatenate([fib, np.full(n - fib.size, 3, np.int64)])[:n]
    row = rng.integers(0, 256, POOL_W)
    long_ = np.tile(row, POOL_ROWS)                                          # matches of 258 one row back
    short = rng.integers(0, 3, n) * 100                                      # three values: short matches everywhere
    mixed = np.concatenate([noise[:n // 2], np.zeros(n - n // 2, np.int64)])
    return [b.reshape(POOL_ROWS, POOL_W) for b in (noise, flat, fib, long_, short, mixed)]


def _pooled_map(segments=1100):
    """`segments` segments of four rows, each one of six blocks in random order, and a last segment of two rows: more chains than 4
    workgroups per compute unit, so every workgroup starts later chains on the LDS tables and the token scratch another block left."""
    rng = np.random.default_rng(5)
    blocks = _pool_blocks()
    order = rng.integers(0, len(blocks), segments)
    return np.concatenate([blocks[i] for i in order] + [blocks[0][:2]])


def device_maps(maps):
    """One device buffer holding every map at an odd uint16 offset (2-byte but not 4-byte aligned), sentinels in between."""
    import torch
    offs, off = [], 1
    for f in maps:
        offs.append(off)
        off += f.size + 2
        off += 1 - off % 2
    host = np.full(off + 8, 0xFFFF, np.uint16)
    for f, o in zip(maps, offs):
        host[o:o + f.size] = np.asarray(f).reshape(-1)
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    ptrs = [buf.data_ptr() + 2 * o for o in offs]
    assert all(p % 4 == 2 for p in ptrs)
    return buf, host, ptrs


@functools.lru_cache(maxsize=None)
def limit_cases():
    rng = np.random.default_rng(4242)
    full = lambda: palette_of(256, rng)
    out = []
    out.append(("len_limit", _len_limit_map(), full(), 65535))
    for D in (32767, 32768, 32769):
        out.append(("far_edge_%d" % D, _far_edge_map(D), full(), 65535))
    out.append(("match_edges", _match_edges_map(), full(), MATCH_EDGES_S))
    out.append(("all_zero", np.zeros((3, 3000), np.int64), full(), 4096))
    out.append(("dist_limit", _dist_limit_map(), full(), 65535))
    out.append(("wide_items", _wide_items_map(), full(), 65535))
    out.append(("header_max", _header_max_map(), full(), 65535))
    out.append(("clc_limit", _clc_limit_map(), full(), 65535))
    out.append(("run_edges_a", _dyadic_map(_run_edges_a_lens()), full(), 65535))
    out.append(("run_edges_b", _dyadic_map(_run_edges_b_lens()), full(), 65535))
    out.append(("run_edges_c", _dyadic_map(_run_edges_c_lens()), full(), 65535))
    out.append(("pooled", _pooled_map(), full(), POOL_S))
    return out


def names():
    return [c[0] for c in limit_cases()]


def case(name):
    return next(c for c in limit_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(file, [png_ref.Block per segment]) of the restatement."""
    _, idx, pal, S = case(name)
    stats = []
    return png_ref.encode(idx, pal, S, stats=stats), stats
