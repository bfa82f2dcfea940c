"""Python restatement of the animated PNG files the library writes (include/nquant_abi.h "APNG encoding", DESIGN.md "PNG encoder,
animated (APNG)"), independent of the library.  A test helper like png_ref.py, whose scanline packing, deflate chains and chunk
writer it uses, and gif_delta_ref.py, whose rectangles it uses: this module restates the mode rule, the bodies and the chunk layout
and nothing else.  encode() is what the GPU tests compare bytes against; parse() / compose() play a file back by the APNG rules, with
Python's zlib and every CRC verified."""
import struct
import zlib

import numpy as np

import png_ref
from gif_delta_ref import rectangles


def _argb(palette):
    return [int(c) & 0xFFFFFFFF for c in np.asarray(palette).reshape(-1)]


def unchanged_index(palette):
    """u of mark mode (every alpha 255 and K <= 255), None in crop mode."""
    pal = _argb(palette)
    return len(pal) if len(pal) <= 255 and all(c >> 24 == 255 for c in pal) else None


def palette_t(palette):
    """The Kt entries of the file's palette: in mark mode entry u = (0, 0, 0) with alpha 0 follows the K entries."""
    pal = _argb(palette)
    return pal + [0] if unchanged_index(pal) is not None else pal


def bodies(frames, palette):
    """What each frame's chains encode: frame 0 whole; frame i its rectangle of frame i, in mark mode unchanged pixels replaced by u."""
    u = unchanged_index(palette)
    out = [np.asarray(frames[0]).astype(np.int64)]
    for i, (x, y, w, h) in enumerate(rectangles(frames)[1:], 1):
        cur = np.asarray(frames[i]).astype(np.int64)[y:y + h, x:x + w]
        prev = np.asarray(frames[i - 1]).astype(np.int64)[y:y + h, x:x + w]
        out.append(cur if u is None else np.where(cur != prev, cur, u))
    return out


def zlib_stream(body, Kt, segment_bytes=0):
    """The IDAT payload of png_ref.encode(body, a palette of Kt entries, segment_bytes)."""
    raw = png_ref.raw_stream(body, Kt)
    return b"\x78\x01" + png_ref.deflate(raw, segment_bytes) + struct.pack(">I", zlib.adler32(raw))


def encode(frames, palette, delays_cs=None, loop=0, segment_bytes=0):
    """frames: 2-D index maps of one (height, width); palette: ARGB_8888 entries (K = len(palette)).  Returns the whole file."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    frames = [np.asarray(f) for f in frames]
    if len(frames) == 1:
        return png_ref.encode(frames[0], palette, segment_bytes)
    assert len({f.shape for f in frames}) == 1
    H, W = frames[0].shape
    pal = palette_t(palette)
    Kt = len(pal)
    over = unchanged_index(palette) is not None
    out = png_ref.SIGNATURE + png_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, png_ref.bit_depth(Kt), 3, 0, 0, 0))
    out += png_ref.chunk(b"PLTE", b"".join(bytes(((c >> 16) & 255, (c >> 8) & 255, c & 255)) for c in pal))
    nt = max((i + 1 for i, c in enumerate(pal) if (c >> 24) != 255), default=0)
    if nt:
        out += png_ref.chunk(b"tRNS", bytes(c >> 24 for c in pal[:nt]))
    out += png_ref.chunk(b"acTL", struct.pack(">II", len(frames), loop))
    seq = 0
    for i, ((x, y, w, h), body) in enumerate(zip(rectangles(frames), bodies(frames, palette))):
        d = int(delays_cs[i]) if delays_cs is not None else 0
        out += png_ref.chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, x, y, d, 100, 0, 1 if over and i else 0))
        seq += 1
        z = zlib_stream(body, Kt, segment_bytes)
        if i == 0:
            out += png_ref.chunk(b"IDAT", z)
        else:
            out += png_ref.chunk(b"fdAT", struct.pack(">I", seq) + z)
            seq += 1
    return out + png_ref.chunk(b"IEND", b"")


def max_bytes(n, width, height, segment_bytes=0):
    """nq_apng_max_bytes restated: n still images of that size at K = 256 (their deflate bound: 4544 + 16 L bits per segment of L
    bytes; 1091 bytes in front of the data, 20 after it), plus acTL and frame 0's fcTL."""
    raw = height * (1 + width)
    S = png_ref.segment_length(raw, segment_bytes)
    full, rest = divmod(raw, S)
    bits = full * (4544 + 16 * S) + ((4544 + 16 * rest) if rest else 0)
    return n * (1091 + (bits + 7) // 8 + 20) + 58


# ---- reading back ----
def parse(apng):
    """(header, frames) of a file whose chunks png_ref.parse has verified.  header: width, height, depth, palette (ARGB per entry),
    num_frames (None: a still image), num_plays.  A frame: x, y, w, h, delay_num, delay_den, dispose, blend, index (h x w, inflated
    with Python's zlib and unpacked).  The sequence numbers must count 0, 1, 2, ... over fcTL and fdAT, and IDAT belongs to frame 0."""
    chunks = png_ref.parse(apng)
    assert chunks[0][0] == b"IHDR" and chunks[1][0] == b"PLTE"
    W, H, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (ctype, comp, flt, lace) == (3, 0, 0, 0)
    plte = chunks[1][1]
    Kt = len(plte) // 3
    assert depth == png_ref.bit_depth(Kt)
    alpha = [255] * Kt
    head = {"width": W, "height": H, "depth": depth, "num_frames": None, "num_plays": None}
    frames, seq, cur = [], 0, None
    for kind, data in chunks[2:-1]:
        if kind == b"tRNS":
            assert not frames and cur is None and len(data) <= Kt
            alpha[:len(data)] = list(data)
        elif kind == b"acTL":
            assert cur is None and head["num_frames"] is None
            head["num_frames"], head["num_plays"] = struct.unpack(">II", data)
        elif kind == b"fcTL":
            s, w, h, x, y, dn, dd, dispose, blend = struct.unpack(">IIIIIHHBB", data)
            assert s == seq and cur is None and x + w <= W and y + h <= H and w >= 1 and h >= 1
            seq += 1
            cur = {"x": x, "y": y, "w": w, "h": h, "delay_num": dn, "delay_den": dd, "dispose": dispose, "blend": blend}
        elif kind in (b"IDAT", b"fdAT"):
            if head["num_frames"] is None:          # a still image
                assert kind == b"IDAT" and not frames
                cur = {"x": 0, "y": 0, "w": W, "h": H, "delay_num": 0, "delay_den": 100, "dispose": 0, "blend": 0}
            assert cur is not None and (kind == b"IDAT") == (not frames)
            if kind == b"fdAT":
                assert struct.unpack(">I", data[:4])[0] == seq
                seq += 1
                data = data[4:]
            else:
                assert (cur["x"], cur["y"], cur["w"], cur["h"]) == (0, 0, W, H)
            raw = zlib.decompress(data)
            assert len(raw) == cur["h"] * (1 + (cur["w"] * depth + 7) // 8)
            cur["index"] = png_ref.unpack(raw, cur["h"], cur["w"], Kt).astype(np.int64)
            frames.append(cur)
            cur = None
        else:
            raise AssertionError("unexpected chunk %r" % kind)
    assert cur is None and (head["num_frames"] is None or head["num_frames"] == len(frames))
    head["palette"] = [a << 24 | plte[3 * i] << 16 | plte[3 * i + 1] << 8 | plte[3 * i + 2] for i, a in enumerate(alpha)]
    return head, frames


def compose(apng):
    """The RGBA canvas (H x W x 4 uint8) after every frame, by the APNG rules for the files written here (dispose_op NONE): the canvas
    starts fully transparent black; blend SOURCE replaces the region's four channels; blend OVER composites the frame onto it, and
    the OVER frames written here hold only the alphas 255 (the pixel replaces) and 0 (the canvas stays), which is asserted."""
    head, frames = parse(apng)
    pal = np.array(head["palette"], np.int64)
    canvas = np.zeros((head["height"], head["width"], 4), np.uint8)
    out = []
    for f in frames:
        assert f["dispose"] == 0 and f["blend"] in (0, 1)
        c = pal[f["index"]]
        src = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255, c >> 24], -1).astype(np.uint8)
        view = canvas[f["y"]:f["y"] + f["h"], f["x"]:f["x"] + f["w"]]
        if f["blend"] == 0:
            view[...] = src
        else:
            a = src[..., 3]
            assert ((a == 0) | (a == 255)).all(), "the OVER frames written here hold alpha 0 and 255 only"
            view[a == 255] = src[a == 255]
        out.append(canvas.copy())
    return out


def rgba_of(frame, palette):
    """The RGBA picture of an index map."""
    c = np.array(_argb(palette), np.int64)[np.asarray(frame)]
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255, c >> 24], -1).astype(np.uint8)


def pillow_canvases(apng):
    """The RGBA canvas Pillow shows for every frame."""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(apng))
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append(np.array(im.convert("RGBA")))
    return out
