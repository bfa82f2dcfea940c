"""nquant.android_amd -- MI355X (gfx950) implementation of the PNN / PNN-LAB colour-quantizer hot path of
mcychan/nQuant.android, behind the reference's own PnnQuantizer / PnnLABQuantizer.convert() interface.

The product is the C-ABI shared library libnquant_hip.so (include/nquant_abi.h, csrc/); this package is the
Python host-side mirror used by the tests and bench.py.  It never imports the CPU oracle and has no CPU fallback:
constructing a quantizer without a usable HIP device raises."""
from .host import (NQ_KIND_RGB, NQ_KIND_LAB, MODE_REFERENCE_SEQUENTIAL, MODE_PARALLEL_TILED, MODE_LOOKUP_ONLY,
                   NqError, Params, PnnQuantizer, PnnLABQuantizer, QuantizedImage, load_library, library_path,
                   abi_symbols, device_bytes, convert_batch_device, convert_batch_host, convert_frames, convert_frames_device,
                   pnnquan_frames_device)
from .gif import (convert_clip_to_gif, convert_frames_to_gif, convert_shots_to_gif, encode_gif, encode_gif_delta, encode_gif_delta_device, encode_gif_device,
                  encode_gif_local, encode_gif_local_delta, encode_gif_local_delta_device, encode_gif_local_device, gif_local_max_bytes,
                  gif_max_bytes, write_gif)
from .png import convert_to_png, encode_png, encode_png_device, png_max_bytes, write_png
from .apng import apng_max_bytes, convert_frames_to_apng, encode_apng, encode_apng_device, write_apng
from .hold import hold_frames, hold_frames_device
from .shots import detect_shots, detect_shots_device, frame_signatures, frame_signatures_device, shots_from_signatures
from .refine import convert_frames_refined, palette_error, refine_palette, refine_palette_device
from .resample import fit_size, resample_frames, resample_frames_device
from .ordered import convert_frames_ordered, dither_ordered, dither_ordered_device
from .yuv import frames_from_yuv, frames_from_yuv_device, resample_frames_yuv, resample_frames_yuv_device, yuv_planes
from .yuv16 import frames_from_yuv16, frames_from_yuv16_device, resample_frames_yuv16, resample_frames_yuv16_device, yuv16_planes
from .retime import RetimePlan, retime_frames, retime_frames_device, retime_plan, timestamps_from_pts
from .orient import orient_frames, orient_frames_device, orientation, oriented_size, source_rect
from .compare import Quality, choose_colors, compare_frames, compare_frames_device, compare_indexed, compare_indexed_device
from .webp import convert_frames_to_webp, convert_to_webp, encode_webp, encode_webp_device, webp_max_bytes, write_webp
from .build import build as build_library

__all__ = ["NQ_KIND_RGB", "NQ_KIND_LAB", "MODE_REFERENCE_SEQUENTIAL", "MODE_PARALLEL_TILED", "MODE_LOOKUP_ONLY",
           "NqError", "Params", "PnnQuantizer", "PnnLABQuantizer", "QuantizedImage", "load_library", "library_path",
           "abi_symbols", "device_bytes", "build_library", "convert_batch_device", "convert_batch_host", "convert_frames",
           "convert_frames_device", "pnnquan_frames_device", "encode_gif", "encode_gif_device", "write_gif", "convert_frames_to_gif",
           "encode_gif_delta", "encode_gif_delta_device", "gif_max_bytes", "gif_local_max_bytes", "encode_gif_local", "encode_gif_local_device",
           "encode_gif_local_delta", "encode_gif_local_delta_device", "convert_shots_to_gif", "encode_png", "encode_png_device", "write_png",
           "convert_to_png", "png_max_bytes", "apng_max_bytes", "encode_apng", "encode_apng_device", "write_apng",
           "convert_frames_to_apng", "hold_frames", "hold_frames_device", "frame_signatures", "frame_signatures_device",
           "shots_from_signatures", "detect_shots", "detect_shots_device", "convert_clip_to_gif", "refine_palette",
           "refine_palette_device", "palette_error", "convert_frames_refined", "fit_size", "resample_frames", "resample_frames_device",
           "dither_ordered", "dither_ordered_device", "convert_frames_ordered", "frames_from_yuv", "frames_from_yuv_device",
           "resample_frames_yuv", "resample_frames_yuv_device", "yuv_planes", "frames_from_yuv16", "frames_from_yuv16_device",
           "resample_frames_yuv16", "resample_frames_yuv16_device", "yuv16_planes", "orient_frames", "orient_frames_device", "orientation",
           "oriented_size", "source_rect", "Quality", "choose_colors", "compare_frames", "compare_frames_device", "compare_indexed",
           "compare_indexed_device", "webp_max_bytes", "encode_webp", "encode_webp_device", "write_webp", "convert_to_webp",
           "convert_frames_to_webp", "RetimePlan", "retime_frames", "retime_frames_device", "retime_plan", "timestamps_from_pts"]
