"""Python restatement of the GIF files with one colour table per frame (include/nquant_abi.h, "GIF encoding, local colour tables"),
a parser that keeps every frame's position and local table, and a composer that plays a file back onto an RGB canvas.  A test helper on
top of gif_ref.py (bit writer, code sizes, sub-blocks, LZW decoder), gif_delta_ref.py (the unchanged index) and gif_lossy_ref.py (the
lossy chains): it restates the normative listing and nothing else.  encode() and encode_delta() return (file bytes, substituted pixels)."""
import struct

import numpy as np

import gif_delta_ref
import gif_lossy_ref
import gif_ref
from gif_ref import color_bits, min_code_size, sub_blocks


def rgb24(palette):
    """rgb_i: the 24-bit RGB of every entry (alpha is not part of it)."""
    return np.asarray(palette).astype(np.int64) & 0xFFFFFF


def _table(pal, Kt):
    """The 2^(N+1) RGB entries of a frame's local table: zeros after entry K - 1 (entry u of delta mode included)."""
    N = color_bits(Kt)
    out = bytearray()
    for i in range(1 << (N + 1)):
        c = int(pal[i]) if i < len(pal) else 0
        out += bytes(((c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF))
    return N, bytes(out)


def _data(body, pal, Kt, T, segment_pixels, lossy):
    if lossy == 0:
        return gif_ref.frame_data(body, Kt, segment_pixels), 0
    return gif_lossy_ref.frame_data(body, Kt, segment_pixels, gif_lossy_ref.Table(pal, Kt, T), lossy)


def _head(W, H, n, loop):
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", W, H, 0x70, 0, 0)
    if n > 1 and loop >= 0:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    return out


def _frames(frames):
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    return [np.asarray(f) for f in frames]


def encode(frames, palettes, delays_cs=None, loop=0, segment_pixels=0, lossy=0):
    """frames: 2-D index maps (sizes may differ); palettes: one sequence of ARGB_8888 entries per frame.  (file, substituted pixels)."""
    frames = _frames(frames)
    n = len(frames)
    assert len(palettes) == n
    out = _head(max(f.shape[1] for f in frames), max(f.shape[0] for f in frames), n, loop)
    subs = 0
    for i, (f, p) in enumerate(zip(frames, palettes)):
        pal = np.asarray(p).astype(np.int64) & 0xFFFFFFFF
        K = len(pal)
        t = gif_ref.transparent_index(pal)
        if n > 1 or t >= 0:
            d = int(delays_cs[i]) if delays_cs is not None else 0
            out += b"\x21\xF9\x04" + struct.pack("<BHB", (2 << 2 if n > 1 else 0) | (t >= 0), d, t if t >= 0 else 0) + b"\x00"
        N, table = _table(pal, K)
        out += b"\x2C" + struct.pack("<HHHHB", 0, 0, f.shape[1], f.shape[0], 0x80 | N) + table
        out.append(min_code_size(K))
        data, s = _data(f, pal, K, t, segment_pixels, lossy)
        subs += s
        out += sub_blocks(data)
    out.append(0x3B)
    return bytes(out), subs


def changed(frames, palettes, i):
    """D of frame i >= 1: where the colour shown differs from the colour frame i - 1 showed."""
    return rgb24(palettes[i])[frames[i]] != rgb24(palettes[i - 1])[frames[i - 1]]


def rectangles(frames, palettes):
    """(x, y, w, h) per frame: the whole map for frame 0, then D's bounding box (1 x 1 at (0, 0) when D is empty)."""
    frames = _frames(frames)
    h, w = frames[0].shape
    out = [(0, 0, w, h)]
    for i in range(1, len(frames)):
        ys, xs = np.nonzero(changed(frames, palettes, i))
        if ys.size == 0:
            out.append((0, 0, 1, 1))
        else:
            out.append((int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)))
    return out


def bodies(frames, palettes, rects=None):
    """What each frame's chains encode: frame 0 whole; frame i its rectangle of index_i, pixels outside D replaced by u_i if there is one.
    rects: rectangles(frames, palettes) where the caller has them already."""
    frames = _frames(frames)
    out = [frames[0].astype(np.int64)]
    for i, (x, y, w, h) in enumerate((rects or rectangles(frames, palettes))[1:], 1):
        u = gif_delta_ref.unchanged_index(len(palettes[i]))
        cur = frames[i].astype(np.int64)[y:y + h, x:x + w]
        out.append(cur if u is None else np.where(changed(frames, palettes, i)[y:y + h, x:x + w], cur, u))
    return out


def encode_delta(frames, palettes, delays_cs=None, loop=0, segment_pixels=0, lossy=0):
    """Frames of one size; (file, substituted pixels).  One frame is the full-frame file."""
    frames = _frames(frames)
    n = len(frames)
    assert len(palettes) == n
    if n == 1:
        return encode(frames, palettes, delays_cs, loop, segment_pixels, lossy)
    assert len({f.shape for f in frames}) == 1
    H, W = frames[0].shape
    out = _head(W, H, n, loop)
    subs = 0
    rects = rectangles(frames, palettes)
    for i, ((x, y, w, h), body) in enumerate(zip(rects, bodies(frames, palettes, rects))):
        pal = np.asarray(palettes[i]).astype(np.int64) & 0xFFFFFFFF
        assert all((int(c) >> 24) != 0 for c in pal), "alpha 0 entries are refused for n > 1"
        K = len(pal)
        u = gif_delta_ref.unchanged_index(K)
        Kt = K + (u is not None)
        d = int(delays_cs[i]) if delays_cs is not None else 0
        out += b"\x21\xF9\x04" + struct.pack("<BHB", 1 << 2 | (u is not None), d, u if u is not None else 0) + b"\x00"
        N, table = _table(pal, Kt)
        out += b"\x2C" + struct.pack("<HHHHB", x, y, w, h, 0x80 | N) + table
        out.append(min_code_size(Kt))
        data, s = _data(body, pal, Kt, u if u is not None else -1, segment_pixels, lossy)
        subs += s
        out += sub_blocks(data)
    out.append(0x3B)
    return bytes(out), subs


def max_bytes(shapes, segment_pixels=0):
    """gif_ref.max_bytes of the same frames + one 768-byte table per frame (the library's nq_gif_local_max_bytes is the same sum)."""
    return gif_ref.max_bytes(shapes, segment_pixels) + 768 * len(shapes)


# ---- reading back ----
def parse(gif):
    """(screen, frames): every frame carries x, y, w, h, m, its extension's fields, index (h, w) and table, an (entries, 3) array (its
    local table; the global one where it has none)."""
    assert gif[:6] == b"GIF89a"
    W, H, packed, bg, _ = struct.unpack("<HHBBB", gif[6:13])
    pos = 13
    gct = None
    if packed & 0x80:
        size = 3 << ((packed & 7) + 1)
        gct = np.frombuffer(gif[pos:pos + size], np.uint8).reshape(-1, 3)
        pos += size
    frames, gce, loop = [], {}, None
    while gif[pos] != 0x3B:
        b = gif[pos]
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
        table = gct
        if ip & 0x80:
            size = 3 << ((ip & 7) + 1)
            table = np.frombuffer(gif[pos:pos + size], np.uint8).reshape(-1, 3)
            pos += size
        m = gif[pos]
        pos += 1
        data = bytearray()
        while gif[pos]:
            data += gif[pos + 1:pos + 1 + gif[pos]]
            pos += 1 + gif[pos]
        pos += 1
        idx = gif_ref.lzw_decode(bytes(data), m, w * h)
        assert idx.size == w * h, "frame %d: %d of %d pixels" % (len(frames), idx.size, w * h)
        assert table is not None and idx.max() < len(table), "frame %d: an index beyond its table" % len(frames)
        frames.append(dict(gce, x=x, y=y, w=w, h=h, m=m, local=bool(ip & 0x80), table=table, index=idx.reshape(h, w)))
        gce = {}
    assert pos == len(gif) - 1, "bytes after the trailer"
    return {"width": W, "height": H, "packed": packed, "background": bg, "loop": loop}, frames


def compose(gif):
    """The RGB canvas (H, W, 3 uint8) after every frame.  A frame's pixels other than its transparent index are painted at its position
    in its own table's colours; disposal 2 clears the frame's area to black before the next frame, 0 and 1 keep the canvas."""
    return compose_parsed(*parse(gif))


def compose_parsed(screen, frames):
    """compose() of what parse() returned."""
    canvas = np.zeros((screen["height"], screen["width"], 3), np.uint8)
    out = []
    for f in frames:
        assert f["x"] + f["w"] <= screen["width"] and f["y"] + f["h"] <= screen["height"]
        view = canvas[f["y"]:f["y"] + f["h"], f["x"]:f["x"] + f["w"]]
        t = f.get("transparency")
        paint = np.ones(f["index"].shape, bool) if t is None else f["index"] != t
        view[paint] = f["table"][f["index"][paint]]
        out.append(canvas.copy())
        if f.get("disposal", 0) == 2:
            view[:] = 0
    return out
