"""Python restatement of the lossy mode of the GIF encoders (include/nquant_abi.h, "GIF encoding, lossy mode").  A test helper like
gif_ref.py and gif_delta_ref.py, from which it takes everything that the mode leaves alone (bit writer, code sizes, sub-blocks,
rectangles and bodies): it restates the normative listing of the one step that changes, and nothing else.  encode() and encode_delta()
return (file bytes, number of substituted pixels)."""
import struct

import numpy as np

import gif_delta_ref
import gif_ref
from gif_ref import _Bits, color_bits, min_code_size, sub_blocks


class Table:
    """What the search needs of the Kt-entry colour table as the file holds it: the largest channel difference and the squared distance
    of every pair of entries, and the transparent index T (-1: none)."""

    def __init__(self, palette, Kt, T):
        pal = np.asarray(palette).astype(np.int64) & 0xFFFFFF
        rgb = np.zeros((Kt, 3), np.int64)
        n = min(len(pal), Kt)
        rgb[:n] = np.stack([(pal[:n] >> 16) & 255, (pal[:n] >> 8) & 255, pal[:n] & 255], -1)
        d = rgb[:, None, :] - rgb[None, :, :]
        self.rgb, self.T = rgb, T
        self.apart = np.abs(d).max(-1).tolist()
        self.d2 = (d * d).sum(-1).tolist()


_TABLES = {}


def table_of(pal, Kt, T):
    """Table(pal, Kt, T), kept for the next call with the same palette (the suites encode many maps over few palettes)."""
    key = (np.asarray(pal).astype(np.int64).tobytes(), Kt, T)
    if key not in _TABLES:
        if len(_TABLES) >= 8:
            _TABLES.clear()
        _TABLES[key] = Table(pal, Kt, T)
    return _TABLES[key]


def _segment(bits, p, m, first, last, tab, lossy):
    """gif_ref._segment with the lossy step; returns the number of pixels that were substituted."""
    clear, eoi = 1 << m, (1 << m) + 1
    w, nxt, table = m + 1, eoi + 1, {}
    kids = {}                                        # pre -> the c with (pre, c) in the dictionary (what the candidates are drawn from)
    subs = 0
    if first:
        bits.emit(clear, w)
    pre = int(p[0])
    for c in p[1:]:
        c = int(c)
        code = table.get((pre, c))
        if code is not None:
            pre = code
            continue
        if lossy > 0 and c != tab.T:
            apart, d2 = tab.apart[c], tab.d2[c]
            cand = [(d2[k], k) for k in kids.get(pre, ()) if k != c and k != tab.T and apart[k] <= lossy]
            if cand:
                pre = table[(pre, min(cand)[1])]
                subs += 1
                continue
        bits.emit(pre, w)
        if nxt == 4096:
            bits.emit(clear, w)
            table, kids, nxt, w = {}, {}, eoi + 1, m + 1
        else:
            table[(pre, c)] = nxt
            kids.setdefault(pre, []).append(c)
            if nxt == (1 << w) and w < 12:
                w += 1
            nxt += 1
        pre = c
    bits.emit(pre, w)
    if nxt == (1 << w) and w < 12:
        w += 1
    bits.emit(eoi if last else clear, w)
    return subs


def frame_data(index, Kt, segment_pixels, tab, lossy):
    """(the LZW data of one frame or body, substituted pixels): gif_ref.frame_data with the lossy chains."""
    p = np.ascontiguousarray(index).reshape(-1).astype(np.int64)
    S = segment_pixels or gif_ref.DEFAULT_SEGMENT
    m = min_code_size(Kt)
    bits = _Bits()
    starts = list(range(0, p.size, S))
    subs = 0
    for k, b in enumerate(starts):
        subs += _segment(bits, p[b:b + S], m, k == 0, k == len(starts) - 1, tab, lossy)
    return bits.finish(), subs


def encode(frames, palette, delays_cs=None, loop=0, segment_pixels=0, lossy=0):
    """gif_ref.encode with lossy chains: (file, substituted pixels)."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    pal = np.asarray(palette).astype(np.int64) & 0xFFFFFFFF
    K, n = len(pal), len(frames)
    N = color_bits(K)
    m = min_code_size(K)
    t = gif_ref.transparent_index(pal)
    tab = table_of(pal, K, t)
    W = max(f.shape[1] for f in frames)
    H = max(f.shape[0] for f in frames)
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", W, H, 0xF0 | N, t if t >= 0 else 0, 0)
    for i in range(1 << (N + 1)):
        c = int(pal[i]) if i < K else 0
        out += bytes(((c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF))
    if n > 1 and loop >= 0:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    subs = 0
    for i, f in enumerate(frames):
        if n > 1 or t >= 0:
            packed = (2 << 2 if n > 1 else 0) | (1 if t >= 0 else 0)
            d = int(delays_cs[i]) if delays_cs is not None else 0
            out += b"\x21\xF9\x04" + struct.pack("<BHB", packed, d, t if t >= 0 else 0) + b"\x00"
        out += b"\x2C" + struct.pack("<HHHHB", 0, 0, f.shape[1], f.shape[0], 0)
        out.append(m)
        data, s = frame_data(f, K, segment_pixels, tab, lossy)
        subs += s
        out += sub_blocks(data)
    out.append(0x3B)
    return bytes(out), subs


def encode_delta(frames, palette, delays_cs=None, loop=0, segment_pixels=0, lossy=0):
    """gif_delta_ref.encode with lossy chains: (file, substituted pixels).  Rectangles and bodies come from the index maps as given."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    frames = [np.asarray(f) for f in frames]
    if len(frames) == 1:
        return encode(frames, palette, delays_cs, loop, segment_pixels, lossy)
    assert len({f.shape for f in frames}) == 1
    pal = np.asarray(palette).astype(np.int64) & 0xFFFFFFFF
    assert all((int(c) >> 24) != 0 for c in pal), "alpha 0 entries are refused for n > 1"
    K = len(pal)
    u = gif_delta_ref.unchanged_index(K)
    Kt = K + (u is not None)
    N, m = color_bits(Kt), min_code_size(Kt)
    tab = table_of(pal, Kt, u if u is not None else -1)
    H, W = frames[0].shape
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", W, H, 0xF0 | N, 0, 0)
    for i in range(1 << (N + 1)):
        c = int(pal[i]) if i < K else 0
        out += bytes(((c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF))
    if loop >= 0:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    subs = 0
    for i, ((x, y, w, h), body) in enumerate(zip(gif_delta_ref.rectangles(frames), gif_delta_ref.bodies(frames, K))):
        d = int(delays_cs[i]) if delays_cs is not None else 0
        out += b"\x21\xF9\x04" + struct.pack("<BHB", 1 << 2 | (u is not None), d, u if u is not None else 0) + b"\x00"
        out += b"\x2C" + struct.pack("<HHHHB", x, y, w, h, 0)
        out.append(m)
        data, s = frame_data(body, Kt, segment_pixels, tab, lossy)
        subs += s
        out += sub_blocks(data)
    out.append(0x3B)
    return bytes(out), subs


# ---- checking a decoded file against its source ----
def within(decoded, source, palette, lossy):
    """True where the decoded index shows a colour within `lossy` per channel of the source index's colour (index maps of one shape)."""
    pal = np.asarray(palette).astype(np.int64) & 0xFFFFFF
    rgb = np.stack([(pal >> 16) & 255, (pal >> 8) & 255, pal & 255], -1)
    return np.abs(rgb[np.asarray(decoded)] - rgb[np.asarray(source)]).max(-1) <= lossy


# ---- content the suites share ----
def ramp_palette(K):
    """An opaque grey ramp: neighbouring entries are 255 // (K - 1) apart, so a small `lossy` already finds candidates."""
    v = (np.arange(K) * 255 // max(K - 1, 1)).astype(np.int64)
    return 0xFF000000 | v << 16 | v << 8 | v


def noisy_gradient_map(h, w, K, seed):
    """(index map, palette): a noisy RGB gradient, K of its pixels sampled as the palette, every pixel given the nearest palette colour
    of its own colour plus random noise -- a random dither.  Deterministic in its arguments."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(w + h - 2, 1)], -1)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).round().astype(np.int64).reshape(-1, 3)
    pal = img[rng.choice(img.shape[0], K, replace=False)]
    noisy = img + rng.integers(-12, 13, img.shape)
    idx = ((noisy[:, None, :] - pal[None, :, :]) ** 2).sum(-1).argmin(-1)
    return idx.reshape(h, w), 0xFF000000 | pal[:, 0] << 16 | pal[:, 1] << 8 | pal[:, 2]


def dithered(h, w, K, rng):
    """What a dither leaves of a smooth gradient: every pixel one of the two ramp entries around its value, chosen at random."""
    g = (np.arange(h)[:, None] * 0.37 + np.arange(w)[None, :]) / (0.37 * h + w) * (K - 1)
    return np.minimum(np.floor(g + rng.random((h, w))).astype(np.int64), K - 1)
