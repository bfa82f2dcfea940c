"""Counts how often a wavefront of gilbert_fast_kernel takes its whole-wavefront fallbacks, on the headline image (4096 x 4096
gradient_noise, seed 3, LAB convert(256, dither=true), 8x8 tiles).

  NQ_BUILD_TAG=count NQ_BUILD_DEFS=-DNQ_FAST_COUNT python -m nquant.android_amd.build     (libnquant_hip.count.so, never the shipped library)
  NQ_LIB=nquant.android_amd/libnquant_hip.count.so python tools/fast_counts.py [out.txt]

A "wavefront-step" is one pass of a wavefront through the call site.  In the dither kernel a lane walks one 8x8 tile, 64 pixels in 64
steps, and a wavefront holds 64 lanes: one wavefront-step covers 64 pixels, so the image has 4096 * 4096 / 64 = 262144 of them."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ["fast_nearest", "fast_nearest_exact", "  lanes that needed it", "  sum of n2 over those lanes", "  sum of the largest n2 (trips of its loop)",
         "fast_nearest32 rolled tail (n2 > 8)", "fast_closest_tuple", "fast_closest_tuple rolled tail (n1 > 8)",
         "closest_err_exact (per candidate step)", "fast_ydiff_cmp", "f64 Y_Diff", "tanh_to_float", "tanh_library",
         "wavefronts that finished in the light walk", "wavefronts that walked again with the chain",
         "pixel-form light pass: steps without a draw (lanes)"]


def main():
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    lib = C.CDLL(nq.library_path())
    if not hasattr(lib, "nq_fast_counts"):
        raise SystemExit("NQ_LIB must point at a build with -DNQ_FAST_COUNT")
    W = H = 4096
    d_in = synth.gradient_noise_torch(W, H, 3)
    q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=nq.MODE_PARALLEL_TILED, seed=3, tile=(8, 8))
    q.width, q.height = W, H
    d_out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    d_idx = torch.empty(W * H, dtype=torch.int16, device="cuda")
    buf = (C.c_ulonglong * 24)()
    q.convert_device(d_in.data_ptr(), 256, True, d_out.data_ptr(), d_idx.data_ptr())       # (first call: tables, scratch)
    torch.cuda.synchronize()
    assert lib.nq_fast_counts(buf, 1) == 0
    q.convert_device(d_in.data_ptr(), 256, True, d_out.data_ptr(), d_idx.data_ptr())
    torch.cuda.synchronize()
    assert lib.nq_fast_counts(buf, 0) == 0
    fast, back = q.dither_path()
    v = list(buf)
    steps = W * H // 64
    lines = ["gilbert_fast_kernel fallback counts, %dx%d gradient_noise seed 3, K = 256, 8x8 tiles (specialised kernel %d, tiles handed back %d)" % (W, H, fast, back),
             "wavefront-steps of the image: %d" % steps, "", "%-52s %14s %12s" % ("call site (wavefront-steps with >= 1 lane in it)", "count", "per step")]
    for name, c in zip(NAMES, v):
        lines.append("%-52s %14d %12.5f" % (name, c, c / steps))
    if v[1]:
        lines += ["", "per fast_nearest_exact call: %.2f lanes need it, mean n2 of those lanes %.2f, loop trips (largest n2) %.2f"
                  % (v[2] / v[1], v[3] / max(v[2], 1), v[4] / v[1]),
                  "share of fast_nearest wavefront-steps that call it: %.4f; share of lanes: %.5f" % (v[1] / max(v[0], 1), v[2] / (64.0 * max(v[0], 1)))]
    # (a single convert runs the fused light walk, whose exit is per wavefront; in the split form -- NQ_OPT_DITHER_CHAIN = 3, or the finish
    # phase of a batch -- the same two slots count TILES: finished by gilbert_light_kernel / listed for the chain pass)
    lines += ["", "light walk (NQ_OPT_DITHER_CHAIN = 0): %d wavefronts finished without the error chain, %d walked again with it (of %d)"
              % (v[13], v[14], W * H // 4096)]
    # the pixel-form light pass (NQ_OPT_DITHER_CHAIN = 4): how many lanes of a wavefront-step enter fast_nearest
    q.set_option(4, 4)
    assert lib.nq_fast_counts(buf, 1) == 0
    q.convert_device(d_in.data_ptr(), 256, True, d_out.data_ptr(), d_idx.data_ptr())
    torch.cuda.synchronize()
    assert lib.nq_fast_counts(buf, 0) == 0
    p = list(buf)
    lines += ["", "pixel-form light pass (NQ_OPT_DITHER_CHAIN = 4), gilbert_pixel_kernel:",
              "wavefront-steps with a looked-up lane %d, of those with >= 1 lane in fast_nearest %d (%.4f)" % (p[16], p[17], p[17] / max(p[16], 1)),
              "lanes in fast_nearest %d: %.2f of 64 per wavefront-step, %.2f per step that enters it" % (p[18], p[18] / max(p[16], 1), p[18] / max(p[17], 1)),
              "steps without a draw (lanes) %d" % p[15]]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
