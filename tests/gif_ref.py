"""Python restatement of the GIF bitstream the library writes (include/nquant_abi.h, "GIF encoding"), plus a plain LZW decoder.
The tests compare the library's bytes with encode() byte for byte, and decode() / Pillow read the files back.  This is a test
helper, not the oracle: it restates the normative listing of the encoding and nothing else."""
import struct

import numpy as np

DEFAULT_SEGMENT = 16384


def color_bits(K):
    """N: smallest value in 0..7 with 2^(N+1) >= max(K, 2)."""
    N = 0
    while (1 << (N + 1)) < max(K, 2):
        N += 1
    return N


def min_code_size(K):
    return max(2, color_bits(K) + 1)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def emit(self, code, width):
        """`width` bits of `code`, least significant bit first; whole bytes leave the accumulator eight at a time."""
        self.acc |= code << self.n
        self.n += width
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def finish(self):
        self.out += self.acc.to_bytes((self.n + 7) // 8, "little")      # (the last byte's upper bits are 0)
        self.acc, self.n = 0, 0
        return bytes(self.out)


def _segment(bits, p, m, first, last):
    clear, eoi = 1 << m, (1 << m) + 1
    w, nxt, table = m + 1, eoi + 1, {}              # table: (pre << 16 | c) -> code, for the string `pre` followed by index c < 65536
    if first:
        bits.emit(clear, w)
    pre = int(p[0])
    for c in p[1:]:
        c = int(c)
        code = table.get(pre << 16 | c)
        if code is not None:
            pre = code
            continue
        bits.emit(pre, w)
        if nxt == 4096:
            bits.emit(clear, w)
            table, nxt, w = {}, eoi + 1, m + 1
        else:
            table[pre << 16 | c] = nxt
            if nxt == (1 << w) and w < 12:
                w += 1
            nxt += 1
        pre = c
    bits.emit(pre, w)
    if nxt == (1 << w) and w < 12:
        w += 1
    bits.emit(eoi if last else clear, w)


def frame_data(index, K, segment_pixels=0):
    """The LZW data of one frame (before the sub-block framing): segments of S pixels, row-major."""
    p = np.ascontiguousarray(index).reshape(-1).astype(np.int64)
    S = segment_pixels or DEFAULT_SEGMENT
    m = min_code_size(K)
    bits = _Bits()
    starts = list(range(0, p.size, S))
    for k, b in enumerate(starts):
        _segment(bits, p[b:b + S].tolist(), m, k == 0, k == len(starts) - 1)     # (a list of ints: the loop is twice as fast over one)
    return bits.finish()


def sub_blocks(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        blk = data[i:i + 255]
        out.append(len(blk))
        out += blk
    out.append(0)
    return bytes(out)


def transparent_index(palette):
    pal = np.asarray(palette).astype(np.int64) & 0xFFFFFFFF
    for i, c in enumerate(pal):
        if (c >> 24) == 0:
            return i
    return -1


def encode(frames, palette, delays_cs=None, loop=0, segment_pixels=0):
    """frames: 2-D index maps (height, width); palette: ARGB_8888 entries (K = len(palette)).  Returns the whole file."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    pal = np.asarray(palette).astype(np.int64) & 0xFFFFFFFF
    K, n = len(pal), len(frames)
    N = color_bits(K)
    m = min_code_size(K)
    t = transparent_index(pal)
    W = max(f.shape[1] for f in frames)
    H = max(f.shape[0] for f in frames)
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", W, H, 0xF0 | N, t if t >= 0 else 0, 0)
    for i in range(1 << (N + 1)):
        c = int(pal[i]) if i < K else 0
        out += bytes(((c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF))
    if n > 1 and loop >= 0:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    for i, f in enumerate(frames):
        if n > 1 or t >= 0:
            packed = (2 << 2 if n > 1 else 0) | (1 if t >= 0 else 0)
            d = int(delays_cs[i]) if delays_cs is not None else 0
            out += b"\x21\xF9\x04" + struct.pack("<BHB", packed, d, t if t >= 0 else 0) + b"\x00"
        out += b"\x2C" + struct.pack("<HHHHB", 0, 0, f.shape[1], f.shape[0], 0)
        out.append(m)
        out += sub_blocks(frame_data(f, K, segment_pixels))
    out.append(0x3B)
    return bytes(out)


def max_bytes(shapes, segment_pixels=0):
    """An upper bound of the file size for frames of these (height, width) shapes, any K and any content (the library's
    nq_gif_max_bytes is another bound; the tests only hold both above encode())."""
    S = segment_pixels or DEFAULT_SEGMENT
    total = 6 + 7 + 3 * 256 + 19 + 1
    for h, w in shapes:
        px = h * w
        bits, left = 0, px
        while left > 0:
            L = min(S, left)
            bits += 12 * (L + 3 + L // 3838)
            left -= L
        d = (bits + 7) // 8
        total += 8 + 10 + 1 + d + (d + 254) // 255 + 1
    return total


# ---- reading back ----
def lzw_decode(data, m, count):
    """Plain GIF LZW decoder: `count` indices from the concatenated sub-block data of one frame."""
    clear, eoi = 1 << m, (1 << m) + 1
    out = []
    pos, nbits = 0, len(data) * 8
    w = m + 1
    table = [[i] for i in range(clear)] + [None, None]
    prev = None
    while pos + w <= nbits:
        code = 0
        for k in range(w):
            b = pos + k
            code |= ((data[b >> 3] >> (b & 7)) & 1) << k
        pos += w
        if code == clear:
            table = table[:eoi + 1]
            w, prev = m + 1, None
            continue
        if code == eoi:
            break
        if prev is None:
            entry = table[code]
            out.extend(entry)
            prev = entry
            continue
        if code < len(table):
            entry = table[code]
            new = prev + entry[:1]
        elif code == len(table):
            entry = prev + prev[:1]
            new = entry
        else:
            raise ValueError("bad LZW code %d (table %d)" % (code, len(table)))
        if len(table) < 4096:
            table.append(new)
            if len(table) == (1 << w) and w < 12:
                w += 1
        out.extend(entry)
        prev = entry
    return np.array(out[:count], np.int64)


def parse(gif):
    """(screen, global table bytes, frames): frames are dicts with w, h, delay, transparency, disposal, index (h, w)."""
    assert gif[:6] == b"GIF89a"
    W, H, packed, bg, _ = struct.unpack("<HHBBB", gif[6:13])
    pos = 13
    gct = b""
    if packed & 0x80:
        size = 3 << ((packed & 7) + 1)
        gct = gif[pos:pos + size]
        pos += size
    frames, gce, loop = [], {}, None
    while True:
        b = gif[pos]
        if b == 0x3B:
            break
        if b == 0x21:
            label = gif[pos + 1]
            pos += 2
            blocks = []
            while gif[pos]:
                blocks.append(gif[pos + 1:pos + 1 + gif[pos]])
                pos += 1 + gif[pos]
            pos += 1
            if label == 0xF9:
                p, d, t = struct.unpack("<BHB", blocks[0])
                gce = {"delay": d, "transparency": t if p & 1 else None, "disposal": (p >> 2) & 7}
            elif label == 0xFF and blocks[0] == b"NETSCAPE2.0":
                loop = struct.unpack("<H", blocks[1][1:3])[0]
            continue
        assert b == 0x2C, "unexpected block 0x%02x at %d" % (b, pos)
        x, y, w, h, ip = struct.unpack("<HHHHB", gif[pos + 1:pos + 10])
        pos += 10
        m = gif[pos]
        pos += 1
        data = bytearray()
        while gif[pos]:
            data += gif[pos + 1:pos + 1 + gif[pos]]
            pos += 1 + gif[pos]
        pos += 1
        idx = lzw_decode(bytes(data), m, w * h).reshape(h, w)
        frames.append(dict(gce, w=w, h=h, index=idx))
        gce = {}
    return {"width": W, "height": H, "packed": packed, "background": bg, "loop": loop}, gct, frames
