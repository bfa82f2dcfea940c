"""Host-side mirror of the reference's quantizer objects over the C ABI (include/nquant_abi.h).

Reference interface mirrored (NQ/ = nQuant.master/src/main/java/com/android/nQuant/):
  new PnnQuantizer(fname) / new PnnLABQuantizer(fname)   NQ/PnnQuantizer.java:35, NQ/PnnLABQuantizer.java:24
  Bitmap convert(int nMaxColors, boolean dither)          NQ/PnnQuantizer.java:409
  boolean hasAlpha()                                       NQ/PnnQuantizer.java:458
  protected pnnquan / nearestColorIndex / closestColorIndex / dither hooks
The file name argument is replaced by the decoded ARGB_8888 pixels (BitmapFactory is Android platform I/O and out
of scope); a non-zero status raises NqError just as the reference's convert() `throws Exception`."""
import ctypes as C
import gc
import os

import numpy as np

NQ_KIND_RGB, NQ_KIND_LAB = 0, 1
MODE_REFERENCE_SEQUENTIAL, MODE_PARALLEL_TILED, MODE_LOOKUP_ONLY = 0, 1, 2

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

OPT_CELL_LISTS, OPT_FAST_DITHER, OPT_MERGE_WALL_SECONDS, OPT_DITHER_CHAIN = 1, 2, 3, 4
# nq_selftest_fast modes (NQ_FAST_ST_*): name -> (code, output words per element; 0 = a counting form)
FAST_ST = {"TANH": (0, 2), "CLOSEST_ERR": (1, 3), "CLOSEST_ERR_PAIRS": (2, 3), "NEXTINT": (3, 1), "NEXTINT_COUNT": (4, 0), "REM": (5, 1),
           "REM_COUNT": (6, 0), "YDIFF": (7, 3), "YDIFF_RANGE": (8, 3), "LAB32": (9, 3), "LAB64": (10, 3), "NEAR_D32": (11, 1),
           "NEAR_D32_PAIRS": (12, 1), "TANH_BITS": (13, 2), "NEXTINT_LIST": (14, 1),
           "NEAR_SAFE": (15, 1), "JUMP": (16, 66)}
YDIFF_RECORD = np.dtype([("c1", np.int32), ("c2", np.int32), ("gt", np.int32), ("pad", np.int32), ("thr", np.float64)])


class NqError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("nquant status %d: %s" % (status, message))
        self.status = status


class Params(C.Structure):
    """nq_params (include/nquant_abi.h)."""
    _fields_ = [("kind", C.c_int32), ("nMaxColors", C.c_int32), ("hasSemiTransparency", C.c_int32),
                ("transparentPixelIndex", C.c_int32), ("transparentColor", C.c_int32), ("isNano", C.c_int32),
                ("texicab", C.c_int32), ("quan_rt", C.c_int32), ("maxbins", C.c_int32), ("paletteLength", C.c_int32),
                ("PR", C.c_double), ("PG", C.c_double), ("PB", C.c_double), ("PA", C.c_double),
                ("ratio", C.c_double), ("weight", C.c_double), ("distinctColors", C.c_int64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_vp, _i32, _i64 = C.c_void_p, C.c_int, C.c_int64
_pi32, _pi64, _pf32 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
# The C ABI (include/nquant_abi.h): name -> (restype, argtypes).  load_library applies it; abi_symbols() lists it.
_ABI = {
    "nq_abi_version": (_i32, []),
    "nq_create": (_i32, [_i32, _i32, C.POINTER(_vp)]),
    "nq_destroy": (None, [_vp]),
    "nq_last_error": (C.c_char_p, [_vp]),
    "nq_set_stream": (_i32, [_vp, _vp]),
    "nq_set_tile": (_i32, [_vp, _i32, _i32]),
    "nq_set_option": (_i32, [_vp, _i32, _i32]),
    "nq_get_list_counts": (_i32, [_vp, _vp, _vp]),
    "nq_get_params": (_i32, [_vp, C.POINTER(Params)]),
    "nq_set_params": (_i32, [_vp, C.POINTER(Params)]),
    "nq_convert": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i64, _i32, _vp, _vp, _vp, _pi32]),
    "nq_convert_device": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i64, _i32, _vp, _vp, _vp, _pi32]),
    "nq_convert_batch_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "nq_convert_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "nq_pnnquan": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _pi32]),
    "nq_pnnquan_device": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _pi32]),
    "nq_dither": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _i64, _i32, _vp, _vp]),
    "nq_dither_device": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _i64, _i32, _vp, _vp]),
    "nq_nearest_index": (_i32, [_vp, _vp, _i32, _vp, _i64, _vp]),
    "nq_closest_tuple": (_i32, [_vp, _vp, _i32, _vp, _i64, _vp]),
    "nq_band_scan_device": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp]),
    "nq_set_scan": (_i32, [_vp, _i32, _i64, C.c_uint32, _i64]),
    "nq_band_histogram_device": (_i32, [_vp, _vp, _i64, _vp]),
    "nq_palette_from_histograms_device": (_i32, [_vp, _vp, _i32, _i32, _vp, _pi32]),
    "nq_band_distinct_device": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "nq_set_distinct": (_i32, [_vp, _i64, _vp]),
    "nq_get_stage_ms": (_i32, [_vp, _pf32]),
    "nq_get_merge_stats": (_i32, [_vp, _pi64]),
    "nq_get_batch_phase_ms": (_i32, [_vp, _pf32]),
    "nq_get_team_stats": (_i32, [_vp, _pi64]),
    "nq_get_merge_variant": (_i32, [_vp, _pi32, _pi32]),
    "nq_get_dither_path": (_i32, [_vp, _pi32, _pi32]),
    "nq_get_dither_split_stats": (_i32, [_pi64]),
    "nq_get_device_bytes": (_i32, [_pi64]),
    "nq_set_band": (_i32, [_vp, _i32, _i32]),
    "nq_selftest_ciede": (_i32, [_vp, _vp, _i64, _vp]),
    "nq_selftest_fast": (_i32, [_vp, _i32, _vp, _i64, _vp]),
    "nq_gilbert_dither": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _vp, C.c_double, _i32, _i64, _i32, _vp, _vp]),
    "nq_bluenoise_dither": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _vp, C.c_float, _i64, _i32, _vp]),
    "nq_band_color_presence_device": (_i32, [_vp, _vp, _i64, _vp, _i32, _pi64, _vp]),
    "nq_pnnquan_frames_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _pi32]),
    "nq_convert_frames_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _pi32]),
    "nq_convert_frames": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _pi32]),
    "nq_gif_max_bytes": (_i32, [_i32, _vp, _vp, _i32, _i32, _pi64]),
    "nq_encode_gif_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _pi64]),
    "nq_encode_gif": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _pi64]),
    "nq_encode_gif_delta_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_encode_gif_delta": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_encode_gif_lossy_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _pi64]),
    "nq_encode_gif_lossy": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _pi64]),
    "nq_encode_gif_delta_lossy_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_encode_gif_delta_lossy": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_gif_local_max_bytes": (_i32, [_i32, _vp, _vp, _i32, _pi64]),
    "nq_encode_gif_local_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _pi64]),
    "nq_encode_gif_local": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _pi64]),
    "nq_encode_gif_local_delta_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_encode_gif_local_delta": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_png_max_bytes": (_i32, [_i32, _vp, _vp, _vp, _i32, _pi64]),
    "nq_encode_png_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "nq_encode_png": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "nq_apng_max_bytes": (_i32, [_i32, _i32, _i32, _i32, _pi64]),
    "nq_encode_apng_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_encode_apng": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_hold_frames_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "nq_hold_frames": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "nq_frame_signatures_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp]),
    "nq_frame_signatures": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp]),
    "nq_shots_from_signatures": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp]),
    "nq_detect_shots_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "nq_detect_shots": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "nq_refine_palette_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _pi32]),
    "nq_refine_palette": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _pi32]),
    "nq_convert_frames_refined_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _pi32]),
    "nq_convert_frames_refined": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _pi32]),
    "nq_resample_frames_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32]),
    "nq_resample_frames": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32]),
    "nq_frames_from_yuv_device": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "nq_frames_from_yuv": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "nq_resample_frames_yuv_device": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 10 + [_vp, _i32, _i32, _i32]),
    "nq_resample_frames_yuv": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 10 + [_vp, _i32, _i32, _i32]),
    "nq_orient_frames_device": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp]),
    "nq_orient_frames": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp]),
    "nq_frames_from_yuv_oriented_device": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 7 + [_vp]),
    "nq_frames_from_yuv_oriented": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 7 + [_vp]),
    "nq_resample_frames_oriented_device": (_i32, [_vp, _i32, _vp] + [_i32] * 7 + [_vp, _i32, _i32, _i32]),
    "nq_resample_frames_oriented": (_i32, [_vp, _i32, _vp] + [_i32] * 7 + [_vp, _i32, _i32, _i32]),
    "nq_resample_frames_yuv_oriented_device": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 11 + [_vp, _i32, _i32, _i32]),
    "nq_resample_frames_yuv_oriented": (_i32, [_vp, _i32, _vp, _vp, _vp] + [_i32] * 11 + [_vp, _i32, _i32, _i32]),
    "nq_dither_ordered_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "nq_dither_ordered": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "nq_convert_frames_ordered_device": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _pi32]),
    "nq_convert_frames_ordered": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _pi32]),
    "nq_compare_frames_device": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "nq_compare_indexed_device": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "nq_compare_frames": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "nq_compare_indexed": (_i32, [_i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "nq_frames_from_yuv16_device": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "nq_frames_from_yuv16": (_i32, [_i32, _i32, _vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "nq_resample_frames_yuv16_device": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp] + [_i32] * 10 + [_vp, _i32, _i32, _i32]),
    "nq_resample_frames_yuv16": (_i32, [_i32, _i32, _vp, _vp, _vp] + [_i32] * 10 + [_vp, _i32, _i32, _i32]),
    "nq_retime_plan": (_i32, [_i32, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nq_retime_frames_device": (_i32, [_i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32]),
    "nq_retime_frames": (_i32, [_i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32]),
    "nq_webp_max_bytes": (_i32, [_i32, _i32, _i32, _i32, _pi64]),
    "nq_encode_webp_device": (_i32, [_i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _pi64, _vp]),
    "nq_encode_webp": (_i32, [_i32, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _pi64, _vp]),
}


def abi_symbols():
    return list(_ABI)


def device_bytes():
    """Bytes of device memory the library holds in this process, over all handles (nq_get_device_bytes).  Quantizers that are unreachable
    but still wait for the garbage collector (a caught NqError's traceback holds its frame's locals in a cycle) are destroyed first, so
    two readings differ only by what the calls between them did, not by when the collector happens to run."""
    gc.collect()
    out = C.c_int64(0)
    rc = load_library().nq_get_device_bytes(C.byref(out))
    if rc != 0:
        raise NqError(rc, "nq_get_device_bytes")
    return out.value


def library_path():
    """libnquant_hip.so next to this file; NQ_LIB=<path> loads another build of it (kernel experiments: build.py NQ_BUILD_TAG)."""
    return os.environ.get("NQ_LIB") or os.path.join(_HERE, "libnquant_hip.so")


def _preload_hip_runtime():
    """One HIP runtime per process.  libnquant_hip.so needs `libamdhip64.so.7`; a PyTorch-ROCm wheel bundles its own copy
    (same SONAME) and always loads it by file name, so if the system runtime got in first the process would hold two
    runtimes and the second one sees no GPU.  When torch is installed, load ITS runtime first (cheap: no torch import);
    the dynamic loader then resolves our NEEDED entry and torch's to that one copy, and torch tensors / streams are
    valid in our launches.  NQ_HIP_RUNTIME=<path> overrides, NQ_HIP_RUNTIME=system skips."""
    choice = os.environ.get("NQ_HIP_RUNTIME", "")
    if choice == "system":
        return
    cand = choice
    if not cand:
        try:
            import importlib.util
            spec = importlib.util.find_spec("torch")
            if spec is not None and spec.submodule_search_locations:
                cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        except Exception:
            cand = ""
    if cand and os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library():
    """Loads libnquant_hip.so (built in-tree by build.py).  Raises if it is missing: there is no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    _preload_hip_runtime()
    L = C.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


def _as_i32(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype != np.int32:
        raise TypeError("pixels must be int32/uint32 ARGB_8888, got %s" % a.dtype)
    return a


class QuantizedImage:
    """What convert() returns: the ARGB pixels of the reference's Bitmap plus the index map and palette."""

    def __init__(self, argb, index, palette):
        self.argb, self.index, self.palette = argb, index, palette


STAGES = ["prescan", "histogram", "nn_init", "merge", "palette_fill", "dither", "bluenoise", "total"]


class PnnQuantizer:
    """RGB PNN quantizer (NQ/PnnQuantizer.java) on one MI355X."""
    KIND = NQ_KIND_RGB

    def __init__(self, pixels, width=None, height=None, device=0, mode=MODE_PARALLEL_TILED, seed=0, tile=None):
        pixels = _as_i32(pixels)
        if width is None:
            height, width = pixels.shape
        self.width, self.height = int(width), int(height)
        self.pixels = pixels.reshape(-1)
        if self.pixels.size != self.width * self.height:
            raise ValueError("pixel count does not match width*height")
        self.mode, self.seed = mode, seed
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.nq_create(self.KIND, device, C.byref(h))
        if rc != 0:
            raise NqError(rc, (self._L.nq_last_error(None) or b"").decode())
        self._h = h
        if tile is not None:
            self._L.nq_set_tile(self._h, int(tile[0]), int(tile[1]))

    # -- plumbing --
    def close(self):
        if getattr(self, "_h", None):
            self._L.nq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise NqError(rc, (self._L.nq_last_error(self._h) or b"").decode())

    def set_stream(self, hip_stream):
        self._check(self._L.nq_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_tile(self, tile_w, tile_h):
        self._check(self._L.nq_set_tile(self._h, tile_w, tile_h))

    def set_band(self, y0, image_height):
        """The following dither calls treat their buffer as rows [y0, ...) of an image of image_height rows (0, 0 = whole image)."""
        self._check(self._L.nq_set_band(self._h, int(y0), int(image_height)))

    def list_counts(self):
        c = np.zeros(65536, np.uint8)
        n = np.zeros(65536, np.uint8)
        self._check(self._L.nq_get_list_counts(self._h, c.ctypes.data, n.ctypes.data))
        return c, n

    def set_option(self, option, value):
        self._check(self._L.nq_set_option(self._h, int(option), int(value)))

    def dither_path(self):
        """(ran the specialised dither kernel?, tiles it handed back to the generic kernel) of the last dither pass."""
        fast, failed = C.c_int32(0), C.c_int32(0)
        self._check(self._L.nq_get_dither_path(self._h, C.byref(fast), C.byref(failed)))
        return fast.value, failed.value

    @property
    def params(self):
        p = Params()
        self._check(self._L.nq_get_params(self._h, C.byref(p)))
        return p

    def set_params(self, p):
        self._check(self._L.nq_set_params(self._h, C.byref(p)))

    def stage_ms(self):
        a = (C.c_float * 8)()
        self._check(self._L.nq_get_stage_ms(self._h, a))
        return dict(zip(STAGES, list(a)))

    def team_stats(self):
        """Counters of the last merge loop's team of helper workgroups (nq_get_team_stats)."""
        a = (C.c_int64 * 16)()
        self._check(self._L.nq_get_team_stats(self._h, a))
        return dict(zip(["published", "used", "timeouts", "wait_ticks_100MHz", "helpers", "speculating_at_end", "cache_hits_top", "virtual_merges_used",
                         "sift_ticks", "merge_ticks", "top_fetch_ticks", "pops", "epilogue_ticks", "select_ticks", "declined", "gave_up"], list(a)))

    def merge_variant(self):
        """(workgroup-size code, helpers per loop) of the merge kernel the last merge launch ran for this quantizer's job
        (nq_get_merge_variant): 512 / 256 / 128, or 127 for the dense variant; (0, 0) when the last palette needed no merge loop."""
        threads, helpers = C.c_int32(0), C.c_int32(0)
        self._check(self._L.nq_get_merge_variant(self._h, C.byref(threads), C.byref(helpers)))
        return threads.value, helpers.value

    def batch_phase_ms(self):
        """Phases of the last batch call this quantizer was the FIRST handle of: {prepare, merge, finish, total} in ms (nq_get_batch_phase_ms)."""
        a = (C.c_float * 4)()
        self._check(self._L.nq_get_batch_phase_ms(self._h, a))
        return dict(zip(["prepare", "merge", "finish", "total"], list(a)))

    def merge_stats(self):
        a = (C.c_int64 * 16)()
        self._check(self._L.nq_get_merge_stats(self._h, a))
        return dict(zip(["find_nn_calls", "merges", "find_ticks_100MHz", "ctrl_ticks_100MHz", "rebuilds", "overflows", "exact_evals",
                         "bound_ticks", "exact_ticks", "replay_ticks", "chunks", "chunks_l1", "chunks_l2", "chunks_listed", "aborted", "seed_round_ticks"], list(a)[:16]))

    # -- the reference interface --
    def hasAlpha(self):
        """NQ/PnnQuantizer.java:458-460"""
        return self.params.transparentPixelIndex > -1

    def convert(self, nMaxColors, dither, mode=None, seed=None):
        """Bitmap convert(int nMaxColors, boolean dither) (NQ/PnnQuantizer.java:409-456)."""
        n = self.width * self.height
        out = np.empty(n, np.int32)
        idx = np.empty(n, np.uint16)
        pal = np.zeros(max(int(nMaxColors), 2), np.int32)
        K = C.c_int32(0)
        self._check(self._L.nq_convert(self._h, self.pixels.ctypes.data, self.width, self.height, int(nMaxColors), int(bool(dither)),
                                       int(self.seed if seed is None else seed), int(self.mode if mode is None else mode),
                                       out.ctypes.data, idx.ctypes.data, pal.ctypes.data, C.byref(K)))
        return QuantizedImage(out.reshape(self.height, self.width), idx.reshape(self.height, self.width), pal[:K.value].copy())

    def pnnquan(self, nMaxColors):
        """Integer[] pnnquan(int[] pixels, int nMaxColors) preceded by convert()'s alpha pre-scan."""
        pal = np.zeros(max(int(nMaxColors), 2), np.int32)
        K = C.c_int32(0)
        self._check(self._L.nq_pnnquan(self._h, self.pixels.ctypes.data, self.width, self.height, int(nMaxColors),
                                       pal.ctypes.data, C.byref(K)))
        return pal[:K.value].copy()

    def dither(self, palette, dither, mode=None, seed=None):
        """int[] dither(cPixels, palette, width, height, dither) (RGB :393-407, LAB NQ/PnnLABQuantizer.java:493-522)."""
        palette = _as_i32(palette)
        n = self.width * self.height
        out = np.empty(n, np.int32)
        idx = np.empty(n, np.uint16)
        self._check(self._L.nq_dither(self._h, self.pixels.ctypes.data, self.width, self.height, palette.ctypes.data, len(palette),
                                      int(bool(dither)), int(self.seed if seed is None else seed),
                                      int(self.mode if mode is None else mode), out.ctypes.data, idx.ctypes.data))
        return out.reshape(self.height, self.width), idx.reshape(self.height, self.width)

    def gilbert_dither(self, palette, saliencies, weight, dither, mode=None, seed=None):
        """static int[] GilbertCurve.dither(width, height, pixels, palette, this, saliencies, weight, dither) (NQ/GilbertCurve.java:367):
        returns (qPixels as the reference leaves them, palette indices)."""
        palette = _as_i32(palette)
        n = self.width * self.height
        sal = None if saliencies is None else np.ascontiguousarray(saliencies, np.float32).reshape(-1)
        out = np.empty(n, np.int32)
        idx = np.empty(n, np.uint16)
        self._check(self._L.nq_gilbert_dither(self._h, self.width, self.height, self.pixels.ctypes.data, palette.ctypes.data, len(palette),
                                              None if sal is None else sal.ctypes.data, float(weight), int(bool(dither)),
                                              int(self.seed if seed is None else seed), int(self.mode if mode is None else mode),
                                              out.ctypes.data, idx.ctypes.data))
        return out.reshape(self.height, self.width), idx.reshape(self.height, self.width)

    def bluenoise_dither(self, palette, qpixels, weight, mode=None, seed=None):
        """static int[] BlueNoise.dither(width, height, pixels, palette, this, qPixels, weight) (NQ/BlueNoise.java:207): qPixels =
        palette indices in, returns (ARGB, final indices)."""
        palette = _as_i32(palette)
        n = self.width * self.height
        io = np.ascontiguousarray(qpixels, np.int32).reshape(-1).copy()
        idx = np.empty(n, np.uint16)
        self._check(self._L.nq_bluenoise_dither(self._h, self.width, self.height, self.pixels.ctypes.data, palette.ctypes.data, len(palette),
                                                io.ctypes.data, float(weight), int(self.seed if seed is None else seed),
                                                int(self.mode if mode is None else mode), idx.ctypes.data))
        return io.reshape(self.height, self.width), idx.reshape(self.height, self.width)

    def selftest_ciede(self, lab_pairs):
        """(n, 6) float32 {L1,A1,B1,L2,A2,B2} -> (n, 4) fast floats, (n, 4) literal floats (as uint32 bit patterns), (n,) decided flags."""
        a = np.ascontiguousarray(lab_pairs, np.float32).reshape(-1, 6)
        out = np.zeros((a.shape[0], 9), np.uint32)
        self._check(self._L.nq_selftest_ciede(self._h, a.ctypes.data, a.shape[0], out.ctypes.data))
        self.ciede_quad_identical = (out[:, 8] >> 1) & 1     # the quad-parallel pass (merge loop) gave the same floats and flag
        return out[:, 0:4], out[:, 4:8], out[:, 8] & 1

    def selftest_fast(self, mode, first=None, count=None, a0=0, thresholds=None, gt=False, records=None):
        """One filter of the specialised dither kernel on its own (nq_selftest_fast).  Range modes: first, count (+ a0; YDIFF_RANGE: up to
        32 float64 thresholds and gt); explicit modes: records (int32 (n, 2); TANH_BITS uint32 (n,); NEXTINT_LIST int32 (n,); JUMP int64 (n,); YDIFF: YDIFF_RECORD).  Returns the (n, words) uint32 output, or
        (disagreements, first disagreeing input or None) for the counting forms."""
        which, words = FAST_ST[mode]
        if records is None:
            thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, np.float64).reshape(-1)
            a1 = (thr.size << 1 | int(bool(gt))) if mode == "YDIFF_RANGE" else 0
            src = np.concatenate([np.array([first, count, a0, a1], np.int64), thr.view(np.int64)])
            n = int(count)
        else:
            src = np.ascontiguousarray(records, YDIFF_RECORD if mode == "YDIFF" else np.uint32 if mode == "TANH_BITS" else np.int64 if mode == "JUMP" else np.int32)
            n = src.shape[0]
        out = np.zeros((n, words) if words else 4, np.uint32)
        self._check(self._L.nq_selftest_fast(self._h, which, src.ctypes.data, n, out.ctypes.data))
        if words:
            return out
        bad, where = (int(v) for v in out.view(np.uint64))
        return bad, (None if where == 2 ** 64 - 1 else where)

    def nearestColorIndex(self, palette, colors):
        """short nearestColorIndex(palette, c, pos) on a cache miss, vectorised over `colors`."""
        palette, colors = _as_i32(palette), _as_i32(colors).reshape(-1)
        out = np.empty(colors.size, np.int16)
        self._check(self._L.nq_nearest_index(self._h, palette.ctypes.data, len(palette), colors.ctypes.data, colors.size, out.ctypes.data))
        return out

    def closestTuple(self, palette, colors):
        """The closest[4] tuple closestColorIndex builds for every colour."""
        palette, colors = _as_i32(palette), _as_i32(colors).reshape(-1)
        out = np.empty((colors.size, 4), np.int32)
        self._check(self._L.nq_closest_tuple(self._h, palette.ctypes.data, len(palette), colors.ctypes.data, colors.size, out.ctypes.data))
        return out

    # -- device-pointer entry points (bench / resident pipelines): ints are HIP device addresses --
    def convert_device(self, d_pixels, nMaxColors, dither, d_out_argb, d_out_index=0, mode=None, seed=None):
        pal = np.zeros(max(int(nMaxColors), 2), np.int32)
        K = C.c_int32(0)
        self._check(self._L.nq_convert_device(self._h, C.c_void_p(d_pixels), self.width, self.height, int(nMaxColors), int(bool(dither)),
                                              int(self.seed if seed is None else seed), int(self.mode if mode is None else mode),
                                              C.c_void_p(d_out_argb), C.c_void_p(d_out_index or None), pal.ctypes.data, C.byref(K)))
        return pal[:K.value].copy()

    def pnnquan_device(self, d_pixels, nMaxColors):
        pal = np.zeros(max(int(nMaxColors), 2), np.int32)
        K = C.c_int32(0)
        self._check(self._L.nq_pnnquan_device(self._h, C.c_void_p(d_pixels), self.width, self.height, int(nMaxColors),
                                              pal.ctypes.data, C.byref(K)))
        return pal[:K.value].copy()

    def dither_device(self, d_pixels, palette, dither, d_out_argb, d_out_index=0, mode=None, seed=None):
        palette = _as_i32(palette)
        self._check(self._L.nq_dither_device(self._h, C.c_void_p(d_pixels), self.width, self.height, palette.ctypes.data, len(palette),
                                             int(bool(dither)), int(self.seed if seed is None else seed),
                                             int(self.mode if mode is None else mode), C.c_void_p(d_out_argb),
                                             C.c_void_p(d_out_index or None)))


def dither_split_stats():
    """nq_get_dither_split_stats, cumulative over the process: (dither passes in the split form of OPT_DITHER_CHAIN, those with the chain
    pass on a batch's side stream, tiles their light kernels listed -- of the passes whose dither_path() has been asked)."""
    out = (C.c_int64 * 3)()
    if load_library().nq_get_dither_split_stats(out) != 0:
        raise RuntimeError("nq_get_dither_split_stats failed")
    return int(out[0]), int(out[1]), int(out[2])


def convert_batch_host(quantizers, pixels, nMaxColors, dither, out_argb, out_index=None, mode=None, seeds=None):
    """nq_convert_batch: like convert_batch_device with HOST addresses (ints) of the pixel / output buffers -- uploads and
    read-backs overlap the per-image stages (fully when the buffers are page-locked)."""
    return convert_batch_device(quantizers, pixels, nMaxColors, dither, out_argb, out_index, mode, seeds, _entry="nq_convert_batch")


def convert_batch_device(quantizers, d_pixels, nMaxColors, dither, d_out_argb, d_out_index=None, mode=None, seeds=None,
                         _entry="nq_convert_batch_device"):
    """nq_convert_batch_device: convert() of several quantizer objects in one call -- their merge loops run side by side in one
    launch.  `quantizers[i].width/height` describe image i, `d_pixels[i]`, `d_out_argb[i]`, `d_out_index[i]` are HIP device
    addresses.  Returns the list of palettes; results equal len(quantizers) separate convert_device calls."""
    n = len(quantizers)
    if n == 0:
        return []
    q0 = quantizers[0]
    hs = (C.c_void_p * n)(*[q._h for q in quantizers])
    src = (C.c_void_p * n)(*[int(a) for a in d_pixels])
    dst = (C.c_void_p * n)(*[int(a) for a in d_out_argb])
    idx = (C.c_void_p * n)(*[int(a) for a in d_out_index]) if d_out_index is not None else None
    widths = np.array([q.width for q in quantizers], np.int32)
    heights = np.array([q.height for q in quantizers], np.int32)
    sd = np.array([q.seed for q in quantizers] if seeds is None else list(seeds), np.int64)
    stride = max(int(nMaxColors), 2)
    pal = np.zeros((n, stride), np.int32)
    K = np.zeros(n, np.int32)
    q0._check(getattr(q0._L, _entry)(hs, n, src, widths.ctypes.data, heights.ctypes.data, int(nMaxColors), int(bool(dither)),
                                            sd.ctypes.data, int(q0.mode if mode is None else mode), dst, idx, pal.ctypes.data,
                                            stride, K.ctypes.data))
    return [pal[i, :K[i]].copy() for i in range(n)]


def _frame_sizes(widths, heights, n):
    w = np.ascontiguousarray(widths, np.int32).reshape(-1)
    h = np.ascontiguousarray(heights, np.int32).reshape(-1)
    if w.size != n or h.size != n:
        raise ValueError("one width and one height per frame")
    return w, h


def pnnquan_frames_device(q, d_pixels, widths, heights, nMaxColors):
    """nq_pnnquan_frames_device: ONE palette for a sequence of frames (HIP device addresses d_pixels[i], frame i of widths[i] x
    heights[i]) on the handle and kind of quantizer `q`; equals pnnquan on the concatenated frames.  The params stay in `q`, so
    q.dither_device(...) per frame applies the palette ("palettegen / paletteuse")."""
    n = len(d_pixels)
    w, h = _frame_sizes(widths, heights, n)
    src = (C.c_void_p * n)(*[int(a) for a in d_pixels])
    pal = np.zeros(max(int(nMaxColors), 2), np.int32)
    K = C.c_int32(0)
    q._check(q._L.nq_pnnquan_frames_device(q._h, n, src, w.ctypes.data, h.ctypes.data, int(nMaxColors), pal.ctypes.data, C.byref(K)))
    return pal[:K.value].copy()


def convert_frames_device(q, d_pixels, widths, heights, nMaxColors, dither, d_out_argb, d_out_index=None, mode=None, seeds=None):
    """nq_convert_frames_device: one shared palette for the frames, then every frame dithered with it (device addresses).  seeds[i]
    (default: q.seed for every frame) is frame i's random seed.  Returns the palette."""
    n = len(d_pixels)
    w, h = _frame_sizes(widths, heights, n)
    src = (C.c_void_p * n)(*[int(a) for a in d_pixels])
    dst = (C.c_void_p * n)(*[int(a) for a in d_out_argb])
    idx = (C.c_void_p * n)(*[int(a) or None for a in d_out_index]) if d_out_index is not None else None
    sd = np.array([q.seed] * n if seeds is None else list(seeds), np.int64)
    if sd.size != n:
        raise ValueError("one seed per frame")
    pal = np.zeros(max(int(nMaxColors), 2), np.int32)
    K = C.c_int32(0)
    q._check(q._L.nq_convert_frames_device(q._h, n, src, w.ctypes.data, h.ctypes.data, int(nMaxColors), int(bool(dither)), sd.ctypes.data,
                                           int(q.mode if mode is None else mode), dst, idx, pal.ctypes.data, C.byref(K)))
    return pal[:K.value].copy()


def _frames_quantizer(kind, frames, device, mode, tile):
    """(the frames as int32 arrays, a quantizer of `kind` whose handle runs the frame-sequence calls)."""
    frames = [_as_i32(f) for f in frames]
    if len(frames) == 0:
        raise ValueError("no frames")
    for f in frames:
        if f.ndim != 2:
            raise ValueError("every frame must be a 2-D (height, width) array")
    cls = PnnLABQuantizer if int(kind) == NQ_KIND_LAB else PnnQuantizer
    return frames, cls(frames[0], device=device, mode=mode, tile=tile)


def _ordered_keyword(ordered, seeds):
    """The `ordered` keyword of the converters: None, or the limit 0..255 of the ordered dither (ordered.py) that replaces the error
    diffusion.  It takes no seeds; a bool is not a limit."""
    if ordered is None:
        return None
    if isinstance(ordered, (bool, np.bool_)):
        raise TypeError("ordered is an integer 0..255 or None")
    if seeds is not None:
        raise ValueError("the ordered dither takes no seeds")
    if not 0 <= int(ordered) <= 255:
        raise ValueError("ordered must be 0..255, got %r" % (ordered,))
    return int(ordered)


def _convert_frames_on(q, frames, nMaxColors, dither, mode, seeds, refine=None, ordered=None):
    """nq_convert_frames of the int32 frames on the handle of quantizer `q`, which stays open; refine not None: nq_convert_frames_refined;
    ordered not None: nq_convert_frames_ordered with that limit (dither, mode and seeds then take no part)."""
    n = len(frames)
    ordered = _ordered_keyword(ordered, seeds)
    hs = np.array([f.shape[0] for f in frames], np.int32)
    ws = np.array([f.shape[1] for f in frames], np.int32)
    sd = np.array([0] * n if seeds is None else list(seeds), np.int64)
    if sd.size != n:
        raise ValueError("one seed per frame")
    outs = [np.empty(f.shape, np.int32) for f in frames]
    idxs = [np.empty(f.shape, np.uint16) for f in frames]
    src = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    idx = (C.c_void_p * n)(*[o.ctypes.data for o in idxs])
    pal = np.zeros(max(int(nMaxColors), 2), np.int32)
    K = C.c_int32(0)
    if ordered is not None:
        q._check(q._L.nq_convert_frames_ordered(q._h, n, src, ws.ctypes.data, hs.ctypes.data, int(nMaxColors), int(refine or 0), ordered,
                                                dst, idx, pal.ctypes.data, C.byref(K)))
    elif refine is None:
        q._check(q._L.nq_convert_frames(q._h, n, src, ws.ctypes.data, hs.ctypes.data, int(nMaxColors), int(bool(dither)), sd.ctypes.data,
                                        int(mode), dst, idx, pal.ctypes.data, C.byref(K)))
    else:
        q._check(q._L.nq_convert_frames_refined(q._h, n, src, ws.ctypes.data, hs.ctypes.data, int(nMaxColors), int(refine), int(bool(dither)),
                                                sd.ctypes.data, int(mode), dst, idx, pal.ctypes.data, C.byref(K)))
    palette = pal[:K.value].copy()
    return palette, [QuantizedImage(o, i, palette) for o, i in zip(outs, idxs)]


def convert_frames(kind, frames, nMaxColors, dither, device=0, mode=MODE_PARALLEL_TILED, seeds=None, tile=None):
    """nq_convert_frames on host arrays: `frames` is a sequence of 2-D int32/uint32 ARGB_8888 arrays (sizes may differ).  Returns
    (palette, [QuantizedImage per frame]) -- one palette shared by all frames (include/nquant_abi.h, "one palette for a sequence of
    frames").  seeds[i] defaults to 0 for every frame; tile as for the quantizer objects (None = automatic)."""
    frames, q = _frames_quantizer(kind, frames, device, mode, tile)
    try:
        return _convert_frames_on(q, frames, nMaxColors, dither, mode, seeds)
    finally:
        q.close()


class PnnLABQuantizer(PnnQuantizer):
    """CIELAB PNN quantizer (NQ/PnnLABQuantizer.java) on one MI355X."""
    KIND = NQ_KIND_LAB
