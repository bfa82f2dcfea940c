"""Python restatement of the lossless WebP files the library writes (include/nquant_abi.h "WebP encoding", DESIGN.md "WebP encoder"),
independent of the library, and an independent reader of such files.
  encode()    the encoder bit for bit: bundling, bands, the per-band parse (png_ref.tokens_of: the PNG encoder's), the code lengths
              (png_ref.code_lengths), the code headers, the entropy image, the colour table, the RIFF container
              with stats=[]: per image and band a Band -- (literals, copies), and what the band reaches of the encoder's limits
  read()      RIFF / VP8X / ANIM / ANMF / VP8L as far as the encoder uses them, with a Huffman decoder of its own (it shares nothing
              with the writer but the bit order); per frame also how many literals and copies every band held
  compose()   the n displayed RGBA canvases of a file
max_bytes() is nq_webp_max_bytes' formula."""
import struct

import numpy as np

import png_ref

# order in which the lengths of the code-length code are stored
CL_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
GREEN_SYMBOLS, DIST_SYMBOLS = 256 + 24, 40
MAX_CHAIN = 32768


def per_of(K):
    """Indices per packed pixel."""
    return 8 if K <= 2 else 4 if K <= 4 else 2 if K <= 16 else 1


def band_bits_of(pw, band_bits=0):
    """p: a band is 2^p packed rows.  0 selects the largest p in 2..9 with pw * 2^p <= 32768."""
    if band_bits == 0:
        ok = [p for p in range(2, 10) if pw << p <= MAX_CHAIN]
        if not ok:
            raise ValueError("packed width %d: no band fits a chain" % pw)
        return ok[-1]
    if not 2 <= band_bits <= 9 or pw << band_bits > MAX_CHAIN:
        raise ValueError("band_bits = %d at packed width %d" % (band_bits, pw))
    return band_bits


def pack(index, K):
    """(h, pw) uint8: index x of a row in bits (x mod per) * (8 / per) of packed pixel x / per."""
    index = np.asarray(index)
    h, w = index.shape
    per = per_of(K)
    d = 8 // per
    pw = (w + per - 1) // per
    padded = np.zeros((h, pw * per), np.uint8)
    padded[:, :w] = index
    out = np.zeros((h, pw), np.uint8)
    for j in range(per):
        out |= padded[:, j::per] << (d * j)
    return out


def prefix_of(v):
    """(prefix symbol, extra value, extra bits) of a length or distance code v >= 1."""
    d = v - 1
    if d < 2:
        return d, 0, 0
    hb = d.bit_length() - 1
    eb = hb - 1
    return 2 * hb + ((d >> eb) & 1), d & ((1 << eb) - 1), eb


class Bits:
    """A bit string: bit i of val is the i-th bit."""

    def __init__(self):
        self.val, self.nb = 0, 0

    def put(self, v, b):
        assert 0 <= v < (1 << b) or (b == 0 and v == 0)
        self.val |= v << self.nb
        self.nb += b

    def extend(self, other):
        self.val |= other.val << self.nb
        self.nb += other.nb

    def tobytes(self):
        return self.val.to_bytes((self.nb + 7) // 8, "little")


def put_code(w, freq):
    """Writes the prefix code of the symbols counted in freq; returns (lengths, codes) for the data: a code with at most one used
    symbol is a simple code whose symbol costs no bits."""
    n = len(freq)
    used = [s for s in range(n) if freq[s]]
    if len(used) <= 1:
        s = used[0] if used else 0
        assert s < 256
        w.put(1, 1)
        w.put(0, 1)
        if s < 2:
            w.put(0, 1)
            w.put(s, 1)
        else:
            w.put(1, 1)
            w.put(s, 8)
        return [0] * n, [0] * n
    lens = png_ref.code_lengths(freq, 15)
    codes = png_ref.canonical_codes(lens)
    rl = png_ref.run_lengths(lens)
    cf = [0] * 19
    for s, _, _ in rl:
        cf[s] += 1
    assert sum(1 for f in cf if f) >= 2
    cl = png_ref.code_lengths(cf, 7)
    cc = png_ref.canonical_codes(cl)
    ncl = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    w.put(0, 1)
    w.put(ncl - 4, 4)
    for i in range(ncl):
        w.put(cl[CL_ORDER[i]], 3)
    w.put(0, 1)
    for s, e, eb in rl:
        w.put(cc[s], cl[s])
        w.put(e, eb)
    return lens, codes


def put_simple_zero(w, symbol):
    put_code(w, [1 if s == symbol else 0 for s in range(256)])


def color_table_bits(w, pal):
    """The colour table as a K x 1 image of differences: cache bit, five codes, K pixels of literals."""
    prev = 0
    px = []
    for c in pal:
        px.append(tuple((((c >> s) & 255) - ((prev >> s) & 255)) & 255 for s in (8, 16, 0, 24)))      # green, red, blue, alpha
        prev = c
    w.put(0, 1)
    tabs = []
    for ch in range(4):
        f = [0] * (GREEN_SYMBOLS if ch == 0 else 256)
        for p in px:
            f[p[ch]] += 1
        tabs.append(put_code(w, f))
    put_code(w, [0] * DIST_SYMBOLS)
    for p in px:
        for ch in range(4):
            w.put(tabs[ch][1][p[ch]], tabs[ch][0][p[ch]])


def entropy_image_bits(w, ew, eh):
    """Pixel (x, y) names group y.  Per row a literal, then, when the row is wider than 1, one copy of length ew - 1 at distance 1."""
    w.put(0, 1)
    fg, fr, fd = [0] * GREEN_SYMBOLS, [0] * 256, [0] * DIST_SYMBOLS
    ls, le, lb = prefix_of(max(ew - 1, 1))
    ds, de, db = prefix_of(1 + 120)
    for y in range(eh):
        fg[y & 255] += 1
        fr[y >> 8] += 1
        if ew > 1:
            fg[256 + ls] += 1
            fd[ds] += 1
    (gl, gc), (rl, rc) = put_code(w, fg), put_code(w, fr)
    put_simple_zero(w, 0)
    put_simple_zero(w, 255)
    dl, dc = put_code(w, fd)
    for y in range(eh):
        w.put(gc[y & 255], gl[y & 255])
        w.put(rc[y >> 8], rl[y >> 8])
        if ew > 1:
            w.put(gc[256 + ls], gl[256 + ls])
            w.put(le, lb)
            w.put(dc[ds], dl[ds])
            w.put(de, db)


class Band(tuple):
    """What `stats` holds per band: the pair (literals, copies), which it compares equal to, and as attributes what the band reaches:
      length           L, the band's packed pixels (the chain length)
      item_bits        the largest data item (one token: green code + length extra bits + distance code + distance extra bits)
      third_word       items with (bit offset in the band's data string) % 32 + bits > 64: they reach a third 32-bit word
      third_word_set   those of them that have a 1 among the bits in that third word
      wide_items       items of more than 32 bits
      green_depth, dist_depth   the longest code of the band's green and distance code (0: the one-symbol form)
      distance, copy   the largest copy distance and copy length (0: no copy)"""
    FIELDS = ("length", "item_bits", "third_word", "third_word_set", "wide_items", "green_depth", "dist_depth", "distance", "copy")

    def __new__(cls, literals, copies, **reach):
        self = super().__new__(cls, (literals, copies))
        assert sorted(reach) == sorted(cls.FIELDS)
        self.__dict__.update(reach)
        return self


def band_bits_strings(seg):
    """(code header, data) bit strings of one band, and its Band."""
    toks = png_ref.tokens_of(seg)
    fg, fd = [0] * GREEN_SYMBOLS, [0] * DIST_SYMBOLS
    for t in toks:
        if isinstance(t, tuple):
            fg[256 + prefix_of(t[0])[0]] += 1
            fd[prefix_of(t[1] + 120)[0]] += 1
        else:
            fg[t] += 1
    head, data = Bits(), Bits()
    gl, gc = put_code(head, fg)
    put_simple_zero(head, 0)
    put_simple_zero(head, 0)
    put_simple_zero(head, 255)
    dl, dc = put_code(head, fd)
    item_bits = third_word = third_word_set = wide_items = 0
    for t in toks:
        at = data.nb
        if isinstance(t, tuple):
            s, e, eb = prefix_of(t[0])
            data.put(gc[256 + s], gl[256 + s])
            data.put(e, eb)
            s, e, eb = prefix_of(t[1] + 120)
            data.put(dc[s], dl[s])
            data.put(e, eb)
        else:
            data.put(gc[t], gl[t])
        bits = data.nb - at
        item_bits = max(item_bits, bits)
        wide_items += bits > 32
        if at % 32 + bits > 64:
            third_word += 1
            third_word_set += (data.val >> (at - at % 32 + 64)) != 0
    copies = [t for t in toks if isinstance(t, tuple)]
    return head, data, Band(len(toks) - len(copies), len(copies), length=len(seg), item_bits=item_bits, third_word=third_word,
                            third_word_set=third_word_set, wide_items=wide_items, green_depth=max(gl), dist_depth=max(dl),
                            distance=max((d for _, d in copies), default=0), copy=max((n for n, _ in copies), default=0))


_VP8L = {}                # vp8l's results by content: an animation that repeats frames restates each distinct one once


def vp8l(index, pal, band_bits=0, stats=None):
    """The payload of a VP8L chunk for one index map (or rectangle of one)."""
    index = np.asarray(index)
    h, w = index.shape
    K = len(pal)
    assert index.min() >= 0 and index.max() < K
    key = (index.astype(np.uint8).tobytes(), h, w, tuple(pal), band_bits)
    if key not in _VP8L:
        _VP8L[key] = _vp8l(index, pal, band_bits)
    data, bands = _VP8L[key]
    if stats is not None:
        stats.append(list(bands))
    return data


def _vp8l(index, pal, band_bits):
    h, w = index.shape
    K = len(pal)
    alpha = any((c >> 24) != 255 for c in pal)
    packed = pack(index, K)
    pw = packed.shape[1]
    p = band_bits_of(pw, band_bits)
    rows = 1 << p
    nb = (h + rows - 1) // rows
    o = Bits()
    o.put(0x2F, 8)
    o.put(w - 1, 14)
    o.put(h - 1, 14)
    o.put(1 if alpha else 0, 1)
    o.put(0, 3)
    o.put(1, 1)
    o.put(3, 2)
    o.put(K - 1, 8)
    color_table_bits(o, pal)
    o.put(0, 1)
    o.put(0, 1)
    if nb > 1:
        o.put(1, 1)
        o.put(p - 2, 3)
        entropy_image_bits(o, (pw + rows - 1) // rows, nb)
    else:
        o.put(0, 1)
    parts = [band_bits_strings(packed[b * rows:(b + 1) * rows].tobytes()) for b in range(nb)]
    for head, _, _ in parts:
        o.extend(head)
    for _, data, _ in parts:
        o.extend(data)
    return o.tobytes(), [band for _, _, band in parts]


def chunk(kind, data):
    return kind + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def u24(v):
    return struct.pack("<I", v)[:3]


def rectangles(frames, delta=True):
    """Frame 0 whole; frame i the bounding box of the pixels that differ from frame i - 1, left and top rounded down to even; 1 x 1 at
    (0, 0) when nothing differs.  delta=False: every frame whole."""
    h, w = np.asarray(frames[0]).shape
    out = [(0, 0, w, h)]
    for i in range(1, len(frames)):
        if not delta:
            out.append((0, 0, w, h))
            continue
        ys, xs = np.nonzero(np.asarray(frames[i]) != np.asarray(frames[i - 1]))
        if len(ys) == 0:
            out.append((0, 0, 1, 1))
            continue
        x0, y0 = int(xs.min()) & ~1, int(ys.min()) & ~1
        out.append((x0, y0, int(xs.max()) + 1 - x0, int(ys.max()) + 1 - y0))
    return out


def encode(frames, palette, delays_cs=None, loop=0, band_bits=0, delta=True, stats=None):
    """The file nq_encode_webp writes for these index maps."""
    frames = [np.asarray(f) for f in frames]
    pal = [int(c) & 0xFFFFFFFF for c in np.asarray(palette).reshape(-1)]
    n = len(frames)
    h, w = frames[0].shape
    if n == 1:
        body = chunk(b"VP8L", vp8l(frames[0], pal, band_bits, stats))
        return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body
    alpha = any((c >> 24) != 255 for c in pal)
    body = chunk(b"VP8X", bytes([0x02 | (0x10 if alpha else 0), 0, 0, 0]) + u24(w - 1) + u24(h - 1))
    body += chunk(b"ANIM", struct.pack("<IH", 0, loop))
    for i, (x, y, rw, rh) in enumerate(rectangles(frames, delta)):
        sub = frames[i][y:y + rh, x:x + rw]
        dur = 10 * (delays_cs[i] if delays_cs is not None else 0)
        body += chunk(b"ANMF", u24(x // 2) + u24(y // 2) + u24(rw - 1) + u24(rh - 1) + u24(dur) + b"\x02" + chunk(b"VP8L", vp8l(sub, pal, band_bits, stats)))
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


# ---- nq_webp_max_bytes ----
HEAD_BITS_MAX = 4640      # five code headers of a band (DESIGN.md "WebP encoder", the bound)
TABLE_BITS_MAX = 30400    # header, transform, colour table and the fixed bits of the main image
ENTROPY_BITS_MAX = 7700   # the entropy image's codes; its rows take at most 64 bits each


def frame_max(w, h, band_bits=0):
    """Most bytes of one frame's ANMF and VP8L chunk, for any content and every K whose bundling the geometry allows."""
    worst = 0
    for per in (1, 2, 4, 8):
        pw = (w + per - 1) // per
        try:
            p = band_bits_of(pw, band_bits)
        except ValueError:
            continue
        nb = (h + (1 << p) - 1) >> p
        bits = TABLE_BITS_MAX + (ENTROPY_BITS_MAX + 64 * nb if nb > 1 else 0) + nb * HEAD_BITS_MAX + 15 * pw * h
        worst = max(worst, (bits + 7) // 8)
    if not worst:
        raise ValueError("%d x %d at band_bits = %d: no bundling fits a chain" % (w, h, band_bits))
    return 24 + 8 + worst + 1


def max_bytes(n, w, h, band_bits=0):
    return 12 + 18 + 14 + n * frame_max(w, h, band_bits)


# ---- an independent reader ----
class Reader:
    def __init__(self, data):
        self.b = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little").tolist()
        self.pos = 0

    def bits(self, n):
        assert self.pos + n <= len(self.b), "read past the chunk"
        r = 0
        for i in range(n):
            r |= self.b[self.pos + i] << i
        self.pos += n
        return r


class Code:
    """A prefix code from its lengths: read bit by bit, most significant bit of a code first."""

    def __init__(self, lens):
        used = [(l, s) for s, l in enumerate(lens) if l]
        assert used, "a code without symbols"
        self.single = used[0][1] if len(used) == 1 else None
        self.table = {}
        if self.single is None:
            code, prev = 0, 0
            for l, s in sorted(used):
                code <<= l - prev
                prev = l
                self.table[(l, code)] = s
                code += 1
            assert code == 1 << prev, "the code is not complete"

    def read(self, r):
        if self.single is not None:
            return self.single
        code = 0
        for l in range(1, 16):
            code = code << 1 | r.bits(1)
            s = self.table.get((l, code))
            if s is not None:
                return s
        raise AssertionError("no such code")


def read_code(r, n):
    lens = [0] * n
    if r.bits(1):
        count = r.bits(1) + 1
        s = r.bits(8 if r.bits(1) else 1)
        lens[s] = 1
        if count == 2:
            lens[r.bits(8)] = 1
        return Code(lens)
    cl = [0] * 19
    for i in range(r.bits(4) + 4):
        cl[CL_ORDER[i]] = r.bits(3)
    clc = Code(cl)
    budget = n
    if r.bits(1):
        budget = 2 + r.bits(2 + 2 * r.bits(3))
        assert budget <= n
    i, prev = 0, 8
    while i < n and budget > 0:
        budget -= 1
        s = clc.read(r)
        if s < 16:
            lens[i] = s
            i += 1
            if s:
                prev = s
            continue
        rep = {16: lambda: 3 + r.bits(2), 17: lambda: 3 + r.bits(3), 18: lambda: 11 + r.bits(7)}[s]()
        assert i + rep <= n
        if s == 16:
            lens[i:i + rep] = [prev] * rep
        i += rep
    return Code(lens)


def read_prefix(r, sym):
    if sym < 4:
        return sym + 1
    extra = (sym - 2) >> 1
    return ((2 + (sym & 1)) << extra) + r.bits(extra) + 1


def read_pixels(r, w, h, groups, group_of, counts=None):
    """ARGB words of a w x h image coded with `groups` (lists of five Codes); group_of(x, y)."""
    out = [0] * (w * h)
    i = 0
    while i < w * h:
        gi = group_of(i % w, i // w)
        g = groups[gi]
        s = g[0].read(r)
        if s < 256:
            red, blue, alpha = g[1].read(r), g[2].read(r), g[3].read(r)
            out[i] = alpha << 24 | red << 16 | s << 8 | blue
            i += 1
            if counts is not None:
                counts[gi][0] += 1
        else:
            assert s < GREEN_SYMBOLS
            length = read_prefix(r, s - 256)
            code = read_prefix(r, g[4].read(r))
            assert code > 120, "a distance code of the 2-D map"
            dist = code - 120
            assert dist <= i and i + length <= w * h
            for _ in range(length):
                out[i] = out[i - dist]
                i += 1
            if counts is not None:
                counts[gi][1] += 1
    return out


def read_groups(r, count):
    return [[read_code(r, GREEN_SYMBOLS)] + [read_code(r, 256) for _ in range(3)] + [read_code(r, DIST_SYMBOLS)] for _ in range(count)]


_READ = {}                # read_vp8l's results by payload


def read_vp8l(data):
    """(index map (h, w), palette words, alpha bit, [(literals, copies)] per band) of a VP8L payload as the encoder writes it."""
    if data not in _READ:
        _READ[data] = _read_vp8l(data)
    index, pal, alpha, bands = _READ[data]
    return index.copy(), list(pal), alpha, list(bands)


def _read_vp8l(data):
    r = Reader(data)
    assert r.bits(8) == 0x2F
    w, h = r.bits(14) + 1, r.bits(14) + 1
    alpha = r.bits(1)
    assert r.bits(3) == 0
    assert r.bits(1) == 1 and r.bits(2) == 3, "one colour-indexing transform"
    K = r.bits(8) + 1
    assert r.bits(1) == 0, "no colour cache"
    pal, prev = [], 0
    for d in read_pixels(r, K, 1, read_groups(r, 1), lambda x, y: 0):
        prev = sum((((d >> s) + (prev >> s)) & 255) << s for s in (0, 8, 16, 24))
        pal.append(prev)
    assert r.bits(1) == 0, "no second transform"
    per = per_of(K)
    pw = (w + per - 1) // per
    assert r.bits(1) == 0, "no colour cache"
    if r.bits(1):
        p = r.bits(3) + 2
        ew, eh = (pw + (1 << p) - 1) >> p, (h + (1 << p) - 1) >> p
        assert r.bits(1) == 0
        ent = [(v >> 8) & 0xFFFF for v in read_pixels(r, ew, eh, read_groups(r, 1), lambda x, y: 0)]
        ngroups = max(ent) + 1
        group_of = lambda x, y: ent[(y >> p) * ew + (x >> p)]
    else:
        ngroups, group_of = 1, lambda x, y: 0
    groups = read_groups(r, ngroups)
    counts = [[0, 0] for _ in range(ngroups)]
    px = read_pixels(r, pw, h, groups, group_of, counts)
    assert (r.pos + 7) // 8 == len(data), "bytes after the image"
    assert not any(r.b[r.pos:]), "padding bits are zero"
    packed = np.array(px, np.uint32).reshape(h, pw)
    assert ((packed & 0xFFFF00FF) == 0xFF000000).all()
    green = ((packed >> 8) & 255).astype(np.uint8)
    d = 8 // per
    index = np.zeros((h, pw * per), np.uint8)
    for j in range(per):
        index[:, j::per] = (green >> (d * j)) & ((1 << d) - 1)
    return index[:, :w], pal, alpha, [tuple(c) for c in counts]


def chunks(data):
    out, pos = [], 0
    while pos < len(data):
        kind = data[pos:pos + 4]
        n, = struct.unpack("<I", data[pos + 4:pos + 8])
        assert pos + 8 + n <= len(data)
        out.append((kind, data[pos + 8:pos + 8 + n]))
        pos += 8 + n + (n & 1)
        if n & 1:
            assert data[pos - 1] == 0
    assert pos == len(data)
    return out


def read(data):
    """{"size": (w, h), "loop", "alpha", "frames": [{"rect", "duration_ms", "index", "palette", "bands"}]}."""
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8 and len(data) % 2 == 0
    top = chunks(data[12:])
    if top[0][0] == b"VP8L":
        assert len(top) == 1
        index, pal, alpha, bands = read_vp8l(top[0][1])
        h, w = index.shape
        return {"size": (w, h), "loop": None, "alpha": alpha,
                "frames": [{"rect": (0, 0, w, h), "duration_ms": 0, "index": index, "palette": pal, "bands": bands}]}
    assert [k for k, _ in top[:2]] == [b"VP8X", b"ANIM"] and all(k == b"ANMF" for k, _ in top[2:]) and len(top) > 2
    x = top[0][1]
    assert len(x) == 10 and x[0] & ~0x10 == 0x02 and x[1:4] == b"\0\0\0"
    w, h = int.from_bytes(x[4:7], "little") + 1, int.from_bytes(x[7:10], "little") + 1
    bg, loop = struct.unpack("<IH", top[1][1])
    assert bg == 0
    frames = []
    for _, a in top[2:]:
        fx, fy, fw, fh, dur = (int.from_bytes(a[3 * i:3 * i + 3], "little") for i in range(5))
        assert a[15] == 0x02, "do not blend, dispose none"
        sub = chunks(a[16:])
        assert len(sub) == 1 and sub[0][0] == b"VP8L"
        index, pal, alpha, bands = read_vp8l(sub[0][1])
        assert index.shape == (fh + 1, fw + 1) and 2 * fx + fw + 1 <= w and 2 * fy + fh + 1 <= h
        assert alpha == (x[0] >> 4) & 1
        frames.append({"rect": (2 * fx, 2 * fy, fw + 1, fh + 1), "duration_ms": dur, "index": index, "palette": pal, "bands": bands})
    assert frames[0]["rect"] == (0, 0, w, h)
    return {"size": (w, h), "loop": loop, "alpha": (x[0] >> 4) & 1, "frames": frames}


def rgba_of(index, pal):
    p = np.array([int(c) & 0xFFFFFFFF for c in pal], np.uint32)[np.asarray(index)]
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255, p >> 24], -1).astype(np.uint8)


def compose(data):
    """The displayed RGBA canvases, one per frame: every rectangle replaces what was there."""
    f = read(data)
    w, h = f["size"]
    canvas = np.zeros((h, w, 4), np.uint8)
    out = []
    for fr in f["frames"]:
        x, y, rw, rh = fr["rect"]
        canvas[y:y + rh, x:x + rw] = rgba_of(fr["index"], fr["palette"])
        out.append(canvas.copy())
    return out
