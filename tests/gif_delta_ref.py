"""Python restatement of the delta-mode GIF bitstream (include/nquant_abi.h, "GIF encoding, delta mode"; DESIGN.md "GIF encoder, delta
mode"), a parser that keeps every frame's position, and a composer that plays a file back onto a canvas.  A test helper like
gif_ref.py, whose LZW, sub-block and code-size rules it imports: it restates the normative listing and nothing else."""
import struct

import numpy as np

import gif_ref
from gif_ref import color_bits, frame_data, min_code_size, sub_blocks


def unchanged_index(K):
    """u: the index that stands for "same as the frame before"; None when the colour table has no room for it."""
    return K if K <= 255 else None


def rectangles(frames):
    """(x, y, w, h) per frame: the whole map for frame 0, then the bounding box of the pixels that differ from the frame before
    (1 x 1 at (0, 0) when none does)."""
    h, w = frames[0].shape
    out = [(0, 0, w, h)]
    for a, b in zip(frames[:-1], frames[1:]):
        ys, xs = np.nonzero(np.asarray(a) != np.asarray(b))
        if ys.size == 0:
            out.append((0, 0, 1, 1))
        else:
            out.append((int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)))
    return out


def bodies(frames, K, rects=None):
    """What each frame's LZW chains encode: frame 0 whole; frame i its rectangle of frame i, unchanged pixels replaced by u.
    rects: rectangles(frames) where the caller has them already."""
    u = unchanged_index(K)
    out = [np.asarray(frames[0]).astype(np.int64)]
    for i, (x, y, w, h) in enumerate((rects or rectangles(frames))[1:], 1):
        cur = np.asarray(frames[i]).astype(np.int64)[y:y + h, x:x + w]
        prev = np.asarray(frames[i - 1]).astype(np.int64)[y:y + h, x:x + w]
        out.append(cur if u is None else np.where(cur != prev, cur, u))
    return out


def encode(frames, palette, delays_cs=None, loop=0, segment_pixels=0):
    """frames: 2-D index maps of one (height, width); palette: ARGB_8888 entries (K = len(palette)).  Returns the whole file."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    frames = [np.asarray(f) for f in frames]
    if len(frames) == 1:
        return gif_ref.encode(frames, palette, delays_cs, loop, segment_pixels)
    assert len({f.shape for f in frames}) == 1
    pal = np.asarray(palette).astype(np.int64) & 0xFFFFFFFF
    assert all((int(c) >> 24) != 0 for c in pal), "alpha 0 entries are refused for n > 1"
    K = len(pal)
    u = unchanged_index(K)
    Kt = K + (u is not None)
    N, m = color_bits(Kt), min_code_size(Kt)
    H, W = frames[0].shape
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", W, H, 0xF0 | N, 0, 0)
    for i in range(1 << (N + 1)):
        c = int(pal[i]) if i < K else 0
        out += bytes(((c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF))
    if loop >= 0:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    rects = rectangles(frames)
    for i, ((x, y, w, h), body) in enumerate(zip(rects, bodies(frames, K, rects))):
        d = int(delays_cs[i]) if delays_cs is not None else 0
        out += b"\x21\xF9\x04" + struct.pack("<BHB", 1 << 2 | (u is not None), d, u if u is not None else 0) + b"\x00"
        out += b"\x2C" + struct.pack("<HHHHB", x, y, w, h, 0)
        out.append(m)
        out += sub_blocks(frame_data(body, Kt, segment_pixels))
    out.append(0x3B)
    return bytes(out)


# ---- reading back ----
def parse(gif):
    """(screen, global table bytes, frames): as gif_ref.parse, and every frame also carries its x and y."""
    assert gif[:6] == b"GIF89a"
    W, H, packed, bg, _ = struct.unpack("<HHBBB", gif[6:13])
    pos = 13
    gct = b""
    if packed & 0x80:
        size = 3 << ((packed & 7) + 1)
        gct = gif[pos:pos + size]
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
        x, y, w, h, _ = struct.unpack("<HHHHB", gif[pos + 1:pos + 10])
        pos += 10
        m = gif[pos]
        pos += 1
        data = bytearray()
        while gif[pos]:
            data += gif[pos + 1:pos + 1 + gif[pos]]
            pos += 1 + gif[pos]
        pos += 1
        idx = gif_ref.lzw_decode(bytes(data), m, w * h)
        assert idx.size == w * h, "frame %d: %d of %d pixels" % (len(frames), idx.size, w * h)
        frames.append(dict(gce, x=x, y=y, w=w, h=h, index=idx.reshape(h, w)))
        gce = {}
    assert pos == len(gif) - 1, "bytes after the trailer"
    return {"width": W, "height": H, "packed": packed, "background": bg, "loop": loop}, gct, frames


def compose(gif):
    """The index canvas after every frame, for files whose frames all keep the canvas (disposal 0 or 1): a frame's pixels other than
    its transparent index are painted at its position.  The canvas starts as -1 (nothing painted)."""
    screen, _, frames = parse(gif)
    canvas = np.full((screen["height"], screen["width"]), -1, np.int64)
    out = []
    for f in frames:
        assert f.get("disposal", 0) in (0, 1), "compose() handles disposal keep only"
        assert f["x"] + f["w"] <= screen["width"] and f["y"] + f["h"] <= screen["height"]
        view = canvas[f["y"]:f["y"] + f["h"], f["x"]:f["x"] + f["w"]]
        t = f.get("transparency")
        paint = np.ones(f["index"].shape, bool) if t is None else f["index"] != t
        view[paint] = f["index"][paint]
        out.append(canvas.copy())
    return out
