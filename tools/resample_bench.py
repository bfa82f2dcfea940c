"""What the frame reduction costs (nq_resample_frames_device): time per call for device-resident frames at two shapes a user would
run -- 16 frames of 3840x2160 to 960x540 and 8 frames of 4096x4096 to 1024x1024 -- in linear light and in stored values, on the
16-byte path and on the one-pixel path (every frame one element behind a 16-byte boundary); the source bytes read per second against
a device-to-device copy of the same source buffer timed in the same run.  No oracle.  A band of output rows of every timed case is
compared with the restatement in tests/resample_ref.py first.

    python tools/resample_bench.py [--reps 30] [--out profiles/r13/resample_bench.txt]

NQ_LIB=<another build of the library> (build.py NQ_BUILD_TAG) times a variant of the kernel."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((16, 3840, 2160, 960, 540), (8, 4096, 4096, 1024, 1024))
BAND = 8                                             # output rows compared with the restatement (both ratios are whole numbers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import resample_ref

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        """(best, median) event span of reps calls after a warm-up, ms."""
        spans = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            call()
            b.record()
            b.synchronize()
            spans.append(a.elapsed_time(b))
        return min(spans[1:]), float(np.median(spans[1:]))

    say("frame reduction on device-resident frames; library %s; best (median) event span of %d calls after a warm-up" % (
        os.path.basename(nq.library_path()), args.reps))
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    for n, W, H, dw, dh in SHAPES:
        px, PAD = W * H, 4                           # room to start every frame one element late (the one-pixel path)
        buf = torch.zeros(n * (px + PAD), dtype=torch.int32, device="cuda")
        frames = [buf[i * (px + PAD):(i + 1) * (px + PAD)] for i in range(n)]
        outs = [torch.zeros(dw * dh, dtype=torch.int32, device="cuda") for _ in range(n)]
        src_bytes = n * px * 4
        say("%d frames of %dx%d -> %dx%d: %.0f MB read, %.0f MB written per call" % (n, W, H, dw, dh, src_bytes / 1e6, n * dw * dh * 4 / 1e6))
        # the yardstick: the same source bytes through a device-to-device copy (read + write)
        dst = torch.empty_like(buf)
        copy_ms, copy_med = timed(lambda: dst.view(torch.float32).copy_(buf.view(torch.float32)))
        copy_read = buf.numel() * 4 / copy_ms / 1e6
        say("  device-to-device copy of the source buffer (torch copy_, float32 view): %.3f ms (%.3f), %.1f GB/s read (and as much written)" % (
            copy_ms, copy_med, copy_read))
        del dst
        for shift in (0, 1):
            for i, f in enumerate(frames):
                f[shift:shift + px].copy_(synth.gradient_noise_torch(W, H, 11 + i))
            torch.cuda.synchronize()
            src = [f.data_ptr() + 4 * shift for f in frames]
            assert all(p % 16 == 4 * shift for p in src)
            for linear in (True, False):
                call = lambda: nq.resample_frames_device(q, src, W, H, [o.data_ptr() for o in outs], (dw, dh), linear=linear)
                call()
                torch.cuda.synchronize()
                rows = BAND * H // dh
                for i in (0, n - 1):
                    top = frames[i][shift:shift + rows * W].cpu().numpy().reshape(rows, W)
                    want = resample_ref.resample([top], (dw, BAND), None, resample_ref.LINEAR if linear else 0)[0]
                    got = outs[i][:BAND * dw].cpu().numpy().reshape(BAND, dw)
                    assert (got == want).all(), "frame %d differs from the restatement (%s, shift %d)" % (i, linear, shift)
                span, med = timed(call)
                say("  %-13s %s path: %8.3f ms (%.3f) per call  %7.1f us per frame  %7.1f GB/s read  %.3f of the copy's read rate" % (
                    "linear light," if linear else "stored values,", "one-pixel" if shift else "16-byte  ", span, med, span * 1e3 / n,
                    src_bytes / span / 1e6, (src_bytes / span / 1e6) / copy_read))
        del buf, frames, outs
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
