"""Quality measurement: what a conversion did to the picture, measured on the GPU (nq_compare_frames / nq_compare_indexed and their
_device forms, include/nquant_abi.h "quality measurement").  One streaming pass over a source frame and its output gives 16 integer
slots: the per-pixel squared error per channel (dither raises it), the squared error of the 8 x 8 block means in linear light (dither
is there to lower it), and SSIM on luma over the same blocks.  All sums are integers: the results are deterministic.
choose_colors() drives the converters with it: the smallest palette size of a ladder that meets a quality target.
The calls take no handle.  There is no CPU fallback: without a HIP device every call raises NqError with status -5 (NQ_ERR_NO_DEVICE)."""
import ctypes as C
import math

import numpy as np

from .host import NqError, _as_i32, _frame_sizes, load_library

COMPARE_LINEAR = 1
SLOTS = 16


class Quality:
    """The 16 raw slots of one pair of frames (or of a sum of pairs, Quality.total), and the figures derived from them on the host."""
    __slots__ = ("slots",)

    def __init__(self, slots):
        s = np.array(slots, np.int64).reshape(-1)
        if s.size != SLOTS:
            raise ValueError("a Quality record holds %d slots" % SLOTS)
        self.slots = s

    pixels = property(lambda self: int(self.slots[0]))
    blocks = property(lambda self: int(self.slots[1]))
    sse = property(lambda self: tuple(int(v) for v in self.slots[2:6]), doc="squared error of a, r, g, b")
    max_diff = property(lambda self: int(self.slots[6]))
    lf = property(lambda self: tuple(int(v) for v in self.slots[7:11]), doc="squared error of the block means of a, r, g, b")
    deficit = property(lambda self: int(self.slots[12]))

    @property
    def psnr(self):
        """10 log10(65025 * 3 * pixels / (sse_r + sse_g + sse_b)); inf when the colours are equal."""
        e = int(self.slots[3:6].sum())
        return math.inf if e == 0 else 10.0 * math.log10(65025.0 * 3.0 * self.pixels / e)

    @property
    def lf_psnr(self):
        """The same of the 16-bit block means: 10 log10(65535^2 * 3 * blocks / (lf_r + lf_g + lf_b))."""
        e = int(self.slots[8:11].sum())
        return math.inf if e == 0 else 10.0 * math.log10(65535.0 ** 2 * 3.0 * self.blocks / e)

    @property
    def ssim(self):
        """Mean block SSIM on luma, 1 for identical frames."""
        return int(self.slots[11]) / (32768.0 * self.blocks)

    @property
    def worst_block(self):
        """The smallest block SSIM."""
        return 1.0 - self.deficit / 32768.0

    @staticmethod
    def total(records):
        """The record of a sequence: the slots add, slots 6 and 12 take the maximum."""
        rows = np.stack([r.slots for r in records])
        s = rows.sum(axis=0)
        s[6], s[12] = rows[:, 6].max(), rows[:, 12].max()
        return Quality(s)

    def meets(self, min_ssim=None, min_psnr=None, min_lf_psnr=None):
        return ((min_ssim is None or self.ssim >= min_ssim) and (min_psnr is None or self.psnr >= min_psnr)
                and (min_lf_psnr is None or self.lf_psnr >= min_lf_psnr))

    def __repr__(self):
        return "Quality(psnr=%.2f, lf_psnr=%.2f, ssim=%.4f, worst_block=%.4f, max_diff=%d)" % (self.psnr, self.lf_psnr, self.ssim,
                                                                                             self.worst_block, self.max_diff)


def _check(L, rc, what):
    if rc != 0:
        raise NqError(rc, (L.nq_last_error(None) or b"").decode() or what)


def _table(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[int(p) for p in ptrs])


def _palette(palette):
    pal = np.array(np.asarray(palette).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32).reshape(-1)
    if pal.size < 1:
        raise ValueError("an empty palette")
    return pal


def _host_pairs(src_frames, outs, out_dtype):
    src = [np.ascontiguousarray(_as_i32(f)) for f in src_frames]
    out = [np.ascontiguousarray(np.asarray(o).astype(out_dtype, copy=False)) if out_dtype is not None else np.ascontiguousarray(_as_i32(o))
           for o in outs]
    if len(src) == 0 or len(src) != len(out):
        raise ValueError("one output per source frame, at least one")
    for s, o in zip(src, out):
        if s.ndim != 2 or s.shape != o.shape:
            raise ValueError("every frame must be a 2-D (height, width) array, and its output of the same shape")
    return src, out


def compare_frames(src_frames, out_frames, linear=True, device=0):
    """nq_compare_frames on host arrays: sequences of 2-D int32/uint32 ARGB_8888 arrays, pair i of one shape (shapes may differ between
    pairs).  linear: block means in linear light (NQ_COMPARE_LINEAR), else in stored values.  Returns one Quality per pair."""
    L = load_library()
    src, out = _host_pairs(src_frames, out_frames, None)
    n = len(src)
    w, h = _frame_sizes([f.shape[1] for f in src], [f.shape[0] for f in src], n)
    res = np.zeros((n, SLOTS), np.int64)
    _check(L, L.nq_compare_frames(int(device), n, _table([f.ctypes.data for f in src]), _table([f.ctypes.data for f in out]), w.ctypes.data,
                                  h.ctypes.data, COMPARE_LINEAR if linear else 0, res.ctypes.data), "nq_compare_frames")
    return [Quality(r) for r in res]


def compare_indexed(src_frames, index_maps, palette, linear=True, device=0):
    """nq_compare_indexed on host arrays: the output of pair i is palette[index_maps[i]] (uint16 maps, 1..256 entries).  An index past
    the palette raises NqError (status -1).  Returns one Quality per pair."""
    L = load_library()
    src, idx = _host_pairs(src_frames, index_maps, np.uint16)
    pal = _palette(palette)
    n = len(src)
    w, h = _frame_sizes([f.shape[1] for f in src], [f.shape[0] for f in src], n)
    res = np.zeros((n, SLOTS), np.int64)
    _check(L, L.nq_compare_indexed(int(device), n, _table([f.ctypes.data for f in src]), _table([f.ctypes.data for f in idx]), pal.ctypes.data,
                                   int(pal.size), w.ctypes.data, h.ctypes.data, COMPARE_LINEAR if linear else 0, res.ctypes.data),
           "nq_compare_indexed")
    return [Quality(r) for r in res]


def compare_frames_device(d_src, d_out, widths, heights, d_result, linear=True, device=0, stream=0):
    """nq_compare_frames_device: d_src[i] / d_out[i] are the HIP device addresses of pair i (widths[i] x heights[i] ARGB pixels, 4-byte
    aligned, never written), d_result that of 16 * n int64 slots (8-byte aligned).  Asynchronous on `stream` (a hipStream_t as an
    integer, 0 = the default stream) of `device`; allocates nothing.  16-byte aligned frames of widths that are multiples of 4 take the
    fast path."""
    L = load_library()
    n = len(d_src)
    if n == 0 or len(d_out) != n:
        raise ValueError("one output per source frame, at least one")
    w, h = _frame_sizes(widths, heights, n)
    _check(L, L.nq_compare_frames_device(int(device), int(stream) or None, n, _table(d_src), _table(d_out), w.ctypes.data, h.ctypes.data,
                                         COMPARE_LINEAR if linear else 0, int(d_result)), "nq_compare_frames_device")


def compare_indexed_device(d_src, d_index, palette, widths, heights, d_result, linear=True, device=0, stream=0):
    """nq_compare_indexed_device: as compare_frames_device with d_index[i] the device address of pair i's uint16 index map (2-byte
    aligned; 8-byte for the fast path) and `palette` 1..256 entries on the host.  An index past the palette reads as the word 0 and is
    not reported by this form, which waits for nothing."""
    L = load_library()
    n = len(d_src)
    if n == 0 or len(d_index) != n:
        raise ValueError("one index map per source frame, at least one")
    pal = _palette(palette)
    w, h = _frame_sizes(widths, heights, n)
    _check(L, L.nq_compare_indexed_device(int(device), int(stream) or None, n, _table(d_src), _table(d_index), pal.ctypes.data, int(pal.size),
                                          w.ctypes.data, h.ctypes.data, COMPARE_LINEAR if linear else 0, int(d_result)),
           "nq_compare_indexed_device")


def choose_colors(kind, frames, dither=True, ladder=(16, 32, 64, 128, 256), min_ssim=None, min_psnr=None, min_lf_psnr=None, ordered=None,
                  refine=0, device=0, linear=True, **convert_args):
    """The smallest palette size of `ladder` whose conversion of `frames` meets every given target (pngquant / gifski --quality).
    Every K of the ladder is tried in ascending order: the frames are converted with convert_frames -- convert_frames_ordered when
    `ordered` (the limit 0..255) is given, convert_frames_refined when `refine` > 0 -- and the outputs measured against the frames on the
    device; the Quality records of the frames are summed (Quality.total) and compared with min_ssim / min_psnr / min_lf_psnr.  The
    search stops at the first K that meets them.  EVERY STEP IS A FULL PALETTE BUILD: the reference's bin weights depend on nMaxColors,
    so the palettes of two sizes are not nested and nothing of one step can serve the next.
    convert_args go to the converter (mode=, seeds=, tile= ...).
    Returns (K, palette, images, report, met): the ladder value chosen, what the converter returned for it, report = {K tried: Quality}
    and met = whether the targets were reached; if no K reaches them, the largest K with met=False.  With no target the first K."""
    from .host import convert_frames
    ladder = sorted(int(k) for k in ladder)
    if not ladder:
        raise ValueError("an empty ladder")
    frames = [_as_i32(f) for f in frames]
    report = {}
    for K in ladder:
        if ordered is not None:
            from .ordered import convert_frames_ordered
            palette, images = convert_frames_ordered(kind, frames, K, ordered, refine=refine, device=device, **convert_args)
        elif refine:
            from .refine import convert_frames_refined
            palette, images = convert_frames_refined(kind, frames, K, dither, refine, device=device, **convert_args)
        else:
            palette, images = convert_frames(kind, frames, K, dither, device=device, **convert_args)
        report[K] = Quality.total(compare_frames(frames, [im.argb for im in images], linear=linear, device=device))
        if report[K].meets(min_ssim, min_psnr, min_lf_psnr):
            return K, palette, images, report, True
    return ladder[-1], palette, images, report, False
