"""Indexed PNG files from the quantizer's index maps, encoded on the GPU (nq_encode_png / nq_encode_png_device, include/nquant_abi.h
"PNG encoding").  One call encodes n independent images, each with its own palette of K <= 256 ARGB entries; the bit depth follows
K, all 8 bits of a palette entry's alpha are kept (tRNS).  There is no CPU fallback: without a HIP device every call raises NqError
with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C

import numpy as np

from .gif import _Handle, _index_maps
from .host import MODE_PARALLEL_TILED, NQ_KIND_LAB, NqError, PnnLABQuantizer, PnnQuantizer, _frame_sizes, load_library


def _palettes(palettes, n):
    """(uint32 [n, stride] table, int32 K[n]) of one palette (n = 1), a sequence of n palettes or an (n, stride) array (K = stride)."""
    if isinstance(palettes, np.ndarray) and palettes.ndim == 1 or (n == 1 and np.ndim(palettes[0]) == 0):
        palettes = [palettes]
    if len(palettes) != n:
        raise ValueError("one palette per image")
    rows = [np.asarray(p).astype(np.int64).reshape(-1) & 0xFFFFFFFF for p in palettes]
    K = np.array([r.size for r in rows], np.int32)
    table = np.zeros((n, max(int(K.max()), 1)), np.uint32)
    for i, r in enumerate(rows):
        table[i, :r.size] = r
    return table, K


def png_max_bytes(widths, heights, K=None, segment_bytes=0):
    """nq_png_max_bytes: an upper bound of the total size of the files for images of these sizes (any content; no device needed).
    K: one value for all images, one per image, or None (256)."""
    L = load_library()
    w = np.ascontiguousarray(widths, np.int32).reshape(-1)
    h = np.ascontiguousarray(heights, np.int32).reshape(-1)
    if w.size != h.size:
        raise ValueError("one width and one height per image")
    k = None
    if K is not None:
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.int32).reshape(-1), w.shape) if np.size(K) == 1 else K, np.int32).reshape(-1)
        if k.size != w.size:
            raise ValueError("one K per image")
    out = C.c_int64(0)
    rc = L.nq_png_max_bytes(int(w.size), w.ctypes.data, h.ctypes.data, k.ctypes.data if k is not None else None, int(segment_bytes), C.byref(out))
    if rc != 0:
        raise NqError(rc, "invalid PNG shape arguments")
    return out.value


def _encode(L, handle, entry, ptrs, w, h, palettes, segment_bytes, check):
    n = len(ptrs)
    table, K = _palettes(palettes, n)
    try:
        cap = png_max_bytes(w, h, K, segment_bytes)
    except NqError:
        cap = 0                                     # (bad sizes: the encode call below says which)
    buf = np.empty(max(cap, 1), np.uint8)
    offs = np.zeros(n + 1, np.int64)
    src = (C.c_void_p * n)(*[int(p) for p in ptrs])
    check(getattr(L, entry)(handle, n, src, w.ctypes.data, h.ctypes.data, table.ctypes.data, int(table.shape[1]), K.ctypes.data,
                            int(segment_bytes), buf.ctypes.data, int(cap), offs.ctypes.data))
    return [buf[offs[i]:offs[i + 1]].tobytes() for i in range(n)]


def encode_png(indices, palettes, segment_bytes=0, device=0):
    """nq_encode_png: `indices` is one 2-D index map -- then `palettes` is its palette (ARGB_8888 entries, K = len <= 256) and the file
    is returned -- or a sequence of n maps with a sequence of n palettes, and a list of n files is returned.  segment_bytes: bytes
    of the raw stream per deflate chain (0 = 32768, at most 65535)."""
    single = isinstance(indices, np.ndarray) and indices.ndim == 2
    maps = _index_maps(indices)
    w = np.array([a.shape[1] for a in maps], np.int32)
    h = np.array([a.shape[0] for a in maps], np.int32)
    if single:
        palettes = [palettes]
    hd = _Handle(device)
    try:
        files = _encode(hd._L, hd._h, "nq_encode_png", [a.ctypes.data for a in maps], w, h, palettes, segment_bytes, hd._check)
    finally:
        hd.close()
    return files[0] if single else files


def encode_png_device(q, d_index_ptrs, widths, heights, palettes, segment_bytes=0):
    """nq_encode_png_device on the handle of quantizer `q`: d_index_ptrs[i] is the HIP device address of image i's uint16 index map
    (widths[i] x heights[i], 2-byte aligned), palettes[i] its palette.  Returns the list of files."""
    n = len(d_index_ptrs)
    w, h = _frame_sizes(widths, heights, n)
    return _encode(q._L, q._h, "nq_encode_png_device", list(d_index_ptrs), w, h, palettes, segment_bytes, q._check)


def write_png(path, index, palette, segment_bytes=0, device=0):
    """encode_png of one image, written to `path`.  Returns the number of bytes written."""
    data = encode_png(np.asarray(index), palette, segment_bytes, device)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def convert_to_png(kind, image, nMaxColors, dither, segment_bytes=0, device=0, mode=MODE_PARALLEL_TILED, seed=0, tile=None):
    """convert(nMaxColors, dither) of the RGB (kind 0) or LAB (kind 1) quantizer followed by the PNG encoding of its index map on the
    same handle.  nMaxColors <= 256.  Returns (file bytes, palette)."""
    if not 1 <= int(nMaxColors) <= 256:
        raise ValueError("a PNG palette holds at most 256 entries")
    q = (PnnLABQuantizer if kind == NQ_KIND_LAB else PnnQuantizer)(image, device=device, mode=mode, seed=seed, tile=tile)
    try:
        out = q.convert(nMaxColors, dither)
        maps = _index_maps(out.index)
        w, h = np.array([maps[0].shape[1]], np.int32), np.array([maps[0].shape[0]], np.int32)
        files = _encode(q._L, q._h, "nq_encode_png", [maps[0].ctypes.data], w, h, [out.palette], segment_bytes, q._check)
    finally:
        q.close()
    return files[0], out.palette
