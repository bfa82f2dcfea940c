"""Python restatement of the indexed PNG files the library writes (include/nquant_abi.h "PNG encoding"), independent
of the library: scanline packing, the per-segment LZ77 parse, the code-length construction, the dynamic-Huffman block layout and the
chunks.  Checksums come from Python's zlib (the library computes its own).  encode() is what the GPU tests compare bytes against;
parse() / unpack() read a file back for the round-trip checks."""
import functools
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
DEFAULT_SEGMENT = 32768
HASH_BITS = 13
MIN_MATCH, MAX_MATCH, MAX_DIST = 3, 258, 32768
# RFC 1951 3.2.5: (first length, extra bits) of length codes 257..285, (first distance, extra bits) of distance codes 0..29
LENGTH_CODES = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2),
                (27, 2), (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5),
                (227, 5), (258, 0)]
DIST_CODES = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1), (9, 2), (13, 2), (17, 3), (25, 3), (33, 4), (49, 4), (65, 5), (97, 5),
              (129, 6), (193, 6), (257, 7), (385, 7), (513, 8), (769, 8), (1025, 9), (1537, 9), (2049, 10), (3073, 10), (4097, 11),
              (6145, 11), (8193, 12), (12289, 12), (16385, 13), (24577, 13)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def bit_depth(K):
    return next(d for d in (1, 2, 4, 8) if (1 << d) >= max(K, 2))


def raw_stream(index, K):
    """Filter byte 0 + the row's indices packed MSB-first at the bit depth of K, padded to a byte, for every row."""
    index = np.asarray(index)
    h, w = index.shape
    d = bit_depth(K)
    per = 8 // d
    rb = (w * d + 7) // 8
    padded = np.zeros((h, rb * per), np.uint8)
    padded[:, :w] = index
    packed = np.zeros((h, rb), np.uint8)
    for j in range(per):
        packed |= padded[:, j::per] << (8 - d * (j + 1))
    return np.concatenate([np.zeros((h, 1), np.uint8), packed], axis=1).tobytes()


def unpack(raw, h, w, K):
    d = bit_depth(K)
    per = 8 // d
    rb = (w * d + 7) // 8
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + rb)
    assert (rows[:, 0] == 0).all()
    out = np.zeros((h, rb * per), np.uint8)
    for j in range(per):
        out[:, j::per] = (rows[:, 1:] >> (8 - d * (j + 1))) & ((1 << d) - 1)
    return out[:, :w]


def tokens_of(seg):
    """The greedy parse of one segment: a list of literals (int) and matches ((length, distance))."""
    L = len(seg)
    a = np.frombuffer(seg, np.uint8)
    cand = np.full(L, -1, np.int64)
    if L >= MIN_MATCH:
        key = a[:-2].astype(np.uint64) | a[1:-1].astype(np.uint64) << np.uint64(8) | a[2:].astype(np.uint64) << np.uint64(16)
        hsh = ((key * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)
        order = np.argsort(hsh, kind="stable")
        same = hsh[order[1:]] == hsh[order[:-1]]
        cand[order[1:][same]] = order[:-1][same]
    cand = cand.tolist()
    out = []
    p = 0
    while p < L:
        q = cand[p]
        n = 0
        if q >= 0 and p - q <= MAX_DIST and seg[q] == seg[p] and seg[q + 1] == seg[p + 1] and seg[q + 2] == seg[p + 2]:
            cap = min(MAX_MATCH, L - p)
            diff = a[q:q + cap] != a[p:p + cap]
            n = int(diff.argmax()) if diff.any() else cap
        if n >= MIN_MATCH:
            out.append((n, p - q))
            p += n
        else:
            out.append(seg[p])
            p += 1
    return out


def code_lengths(freq, limit):
    """Code lengths <= limit of the used symbols: Huffman's construction on the symbols sorted by (count, symbol) -- two queues, the
    leaf is taken on a tie --, depths above `limit` cut to it and the Kraft sum repaired, then the multiset of lengths is dealt out
    longest first in the sorted order.  No used symbol: symbol 0 gets length 1; one: it gets length 1."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    n = len(used)
    lens = [0] * len(freq)
    if n <= 1:
        lens[used[0][1] if n else 0] = 1
        return lens
    W = [f for f, _ in used] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n
    for k in range(n, 2 * n - 1):
        for _ in range(2):
            if i < n and (j >= k or W[i] <= W[j]):
                t = i
                i += 1
            else:
                t = j
                j += 1
            W[k] += W[t]
            parent[t] = k
    depth = [0] * (2 * n - 1)
    for t in range(2 * n - 3, -1, -1):
        depth[t] = depth[parent[t]] + 1
    count = [0] * (limit + 1)
    for t in range(n):
        count[min(depth[t], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        l = max(x for x in range(1, limit) if count[x])
        count[l] -= 1
        count[l + 1] += 2
        total -= 1
    t = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lens[used[t][1]] = l
            t += 1
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2; returned bit-reversed (a Huffman code goes into the stream most significant bit first)."""
    maxl = max(lens)
    bl = [0] * (maxl + 2)
    for l in lens:
        if l:
            bl[l] += 1
    nxt = [0] * (maxl + 2)
    code = 0
    for b in range(1, maxl + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return out


def run_lengths(seq):
    """The code-length sequence in code-length-code symbols: [(symbol, extra value, extra bits)].  A run of r equal lengths v:
    v = 0: 18 (11..138 zeros) while r >= 11, then 17 (3..10) if r >= 3, else r plain zeros; v > 0: v once, then 16 (3..6 repeats)
    while r >= 3 remain, the rest plain."""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        r = 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                c = min(r, 138)
                out.append((18, c - 11, 7))
                r -= c
            if r >= 3:
                out.append((17, r - 3, 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                c = min(r, 6)
                out.append((16, c - 3, 2))
                r -= c
        out.extend([(v, 0, 0)] * r)
    return out


def _length_symbol(n):
    for c in range(len(LENGTH_CODES) - 1, -1, -1):
        if n >= LENGTH_CODES[c][0]:
            return 257 + c, n - LENGTH_CODES[c][0], LENGTH_CODES[c][1]


def _dist_symbol(d):
    for c in range(len(DIST_CODES) - 1, -1, -1):
        if d >= DIST_CODES[c][0]:
            return c, d - DIST_CODES[c][0], DIST_CODES[c][1]


def unlimited_depth(freq):
    """The largest depth of Huffman's tree over the used symbols when no limit cuts it (code_lengths with a limit no tree reaches)."""
    return max(code_lengths(freq, max(len(freq), 2)))


def step_groups(seg):
    """What the parse's 64-position steps see of the hash, one entry per step that holds a position with three bytes:
    (valid positions, groups of two or more positions that share a hash, size of the largest group, neighbours in a group -- a
    position and the one it takes as its candidate -- whose three bytes differ: a collision of the 13-bit hash inside the step)."""
    L = len(seg)
    a = np.frombuffer(seg, np.uint8)
    out = []
    if L < MIN_MATCH:
        return out
    key = a[:-2].astype(np.uint64) | a[1:-1].astype(np.uint64) << np.uint64(8) | a[2:].astype(np.uint64) << np.uint64(16)
    hsh = ((key * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)
    for base in range(0, L - 2, 64):
        h, k = hsh[base:base + 64], key[base:base + 64]
        order = np.argsort(h, kind="stable")
        same = h[order[1:]] == h[order[:-1]]
        _, counts = np.unique(h, return_counts=True)
        out.append((len(h), int((counts >= 2).sum()), int(counts.max()), int((same & (k[order[1:]] != k[order[:-1]])).sum())))
    return out


class Block:
    """One segment's dynamic-Huffman block and how it came about (the `stats` of deflate() and encode()):
    value, bits     the block: bit i of value is its i-th bit
    tokens          the greedy parse: literals (int) and matches ((length, distance))
    lit_hist, dist_hist, cl_hist      the three symbol histograms (286, 30 and 19 counts)
    lit_lens, dist_lens, cl_lens      the code lengths with the limits 15, 15 and 7
    lit_depth, dist_depth, cl_depth   the largest depth of each tree without a limit
    hlit, hdist, hclen                the header's three counts
    runs            the code-length sequence: [(code-length-code symbol, extra value, extra bits)]
    items           per token (bit position in the block, bit count, value): what the bit writer takes as one item
    steps           step_groups() of the segment"""
    __slots__ = ("value", "bits", "tokens", "lit_hist", "dist_hist", "cl_hist", "lit_lens", "dist_lens", "cl_lens", "lit_depth", "dist_depth",
                 "cl_depth", "hlit", "hdist", "hclen", "runs", "items", "steps", "length")


def _block(seg, final, full):
    """The Block of a segment; `full`: with the fields that only the statistics need (the depths, items and steps)."""
    B = Block()
    B.length = len(seg)
    toks = B.tokens = tokens_of(seg)
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in toks:
        if isinstance(t, tuple):
            lf[_length_symbol(t[0])[0]] += 1
            df[_dist_symbol(t[1])[0]] += 1
        else:
            lf[t] += 1
    ll, dl = code_lengths(lf, 15), code_lengths(df, 15)
    lc, dc = canonical_codes(ll), canonical_codes(dl)
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    hdist = max(1, max(s for s in range(30) if dl[s]) + 1)
    rl = run_lengths(ll[:hlit] + dl[:hdist])
    cf = [0] * 19
    for s, _, _ in rl:
        cf[s] += 1
    cl = code_lengths(cf, 7)
    cc = canonical_codes(cl)
    hclen = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    B.lit_hist, B.dist_hist, B.cl_hist = lf, df, cf
    B.lit_lens, B.dist_lens, B.cl_lens = ll, dl, cl
    if full:
        B.lit_depth, B.dist_depth, B.cl_depth = unlimited_depth(lf), unlimited_depth(df), unlimited_depth(cf)
    B.hlit, B.hdist, B.hclen, B.runs = hlit, hdist, hclen, rl
    val, nb = 0, 0

    def put(v, b):
        nonlocal val, nb
        val |= v << nb
        nb += b

    put(1 if final else 0, 1)
    put(2, 2)
    put(hlit - 257, 5)
    put(hdist - 1, 5)
    put(hclen - 4, 4)
    for i in range(hclen):
        put(cl[CL_ORDER[i]], 3)
    for s, e, eb in rl:
        put(cc[s], cl[s])
        put(e, eb)
    items = B.items = []
    for t in toks:
        at = nb
        if isinstance(t, tuple):
            s, e, eb = _length_symbol(t[0])
            put(lc[s], ll[s])
            put(e, eb)
            s, e, eb = _dist_symbol(t[1])
            put(dc[s], dl[s])
            put(e, eb)
        else:
            put(lc[t], ll[t])
        if full:
            items.append((at, nb - at, val >> at))
    put(lc[256], ll[256])
    B.value, B.bits = val, nb
    if full:
        B.steps = step_groups(seg)
    return B


@functools.lru_cache(maxsize=1 << 16)
def block_of(seg, final):
    """(value, bit count) of the one dynamic-Huffman block of a segment; bit i of the value is the i-th bit of the block."""
    B = _block(seg, final, False)
    return B.value, B.bits


@functools.lru_cache(maxsize=64)
def block_stats(seg, final):
    """The Block of a segment with every field."""
    return _block(seg, final, True)


def segment_length(raw_len, segment_bytes):
    return min(segment_bytes if segment_bytes else DEFAULT_SEGMENT, raw_len)


def deflate(raw, segment_bytes=0, stats=None):
    """The segments' blocks one after another, the last byte zero-padded.  `stats`: a list that receives every segment's Block."""
    S = segment_length(len(raw), segment_bytes)
    val, nb = 0, 0
    parts = []
    for o in range(0, len(raw), S):
        if stats is None:
            v, b = block_of(raw[o:o + S], o + S >= len(raw))
        else:
            stats.append(block_stats(raw[o:o + S], o + S >= len(raw)))
            v, b = stats[-1].value, stats[-1].bits
        val |= v << nb
        nb += b
        if nb >= 1 << 16:                            # keep the big integer short
            k = nb // 8
            parts.append((val & ((1 << (8 * k)) - 1)).to_bytes(k, "little"))
            val >>= 8 * k
            nb -= 8 * k
    parts.append(val.to_bytes((nb + 7) // 8, "little"))
    return b"".join(parts)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(index, palette, segment_bytes=0, stats=None):
    """The file.  `stats`: a list that receives the Block of every segment, in order."""
    index = np.asarray(index)
    h, w = index.shape
    pal = [int(c) & 0xFFFFFFFF for c in np.asarray(palette).reshape(-1)]
    K = len(pal)
    raw = raw_stream(index, K)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth(K), 3, 0, 0, 0))
    out += chunk(b"PLTE", b"".join(bytes(((c >> 16) & 255, (c >> 8) & 255, c & 255)) for c in pal))
    nt = max((i + 1 for i, c in enumerate(pal) if (c >> 24) != 255), default=0)
    if nt:
        out += chunk(b"tRNS", bytes(c >> 24 for c in pal[:nt]))
    out += chunk(b"IDAT", b"\x78\x01" + deflate(raw, segment_bytes, stats) + struct.pack(">I", zlib.adler32(raw)))
    return out + chunk(b"IEND", b"")


def parse(png):
    """[(type, data)] of a file's chunks; every CRC is verified."""
    assert png[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        kind, data = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + data), kind
        out.append((kind, data))
        pos += 12 + n
    assert pos == len(png) and out[-1] == (b"IEND", b"")
    return out


def decode(png):
    """(index map, K, palette RGB bytes, tRNS bytes or None) of an indexed PNG with one IDAT, inflated by Python's zlib."""
    chunks = parse(png)
    kinds = [k for k, _ in chunks]
    assert kinds in ([b"IHDR", b"PLTE", b"IDAT", b"IEND"], [b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"]), kinds
    d = dict(chunks)
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", d[b"IHDR"])
    assert (ctype, comp, flt, lace) == (3, 0, 0, 0)
    K = len(d[b"PLTE"]) // 3
    assert depth == bit_depth(K)
    raw = zlib.decompress(d[b"IDAT"])
    return unpack(raw, h, w, K), K, d[b"PLTE"], d.get(b"tRNS")
