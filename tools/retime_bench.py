"""What the retiming costs (nq_retime_frames_device): time per call for 64 device-resident frames at 60 fps blended down to 15 fps --
1920x1080 and 960x540 with the whole period as shutter, in linear light and in stored values; shutter 1 (every output copies one
frame); and every frame one element behind a 16-byte boundary (the one-pixel path) --, and the source bytes the plan reads per second
against a device-to-device copy of the source buffer timed in the same run.  No oracle.  The first and the last 4096 pixels of the
first and the last output of every timed case are compared with the restatement in tests/retime_ref.py first.

    python tools/retime_bench.py [--reps 30] [--out profiles/r21/retime_bench.txt]

NQ_LIB=<another build of the library> (build.py NQ_BUILD_TAG) times a variant of the kernel."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 64
SHAPES = ((1920, 1080), (960, 540))
BAND = 4096                                          # pixels compared with the restatement at either end of an output


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import retime_ref

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

    say("retiming of device-resident frames; library %s; best (median) event span of %d calls after a warm-up" % (
        os.path.basename(nq.library_path()), args.reps))
    t = [round(i * 1e6 / 60) for i in range(N + 1)]
    full = nq.retime_plan(t, fps=15)
    pick = nq.retime_plan(t, fps=15, shutter_us=1)
    say("%d frames at 60 fps -> 15 fps: %d outputs; full shutter: %d pairs (a source is read twice where a window's end cuts it); "
        "shutter 1: %d pairs" % (N, full.m, len(full.source), len(pick.source)))
    for W, H in SHAPES:
        px, PAD = W * H, 4                           # room to start every frame one element late (the one-pixel path)
        buf = torch.zeros(N * (px + PAD), dtype=torch.int32, device="cuda")
        frames = [buf[i * (px + PAD):(i + 1) * (px + PAD)] for i in range(N)]
        obuf = torch.zeros(full.m * (px + PAD), dtype=torch.int32, device="cuda")
        outs = [obuf[j * (px + PAD):(j + 1) * (px + PAD)] for j in range(full.m)]
        say("%d frames of %dx%d (%.0f MB) -> %d frames (%.0f MB)" % (N, W, H, N * px * 4 / 1e6, full.m, full.m * px * 4 / 1e6))
        # the yardstick: the source buffer through a device-to-device copy (read + write)
        dst = torch.empty_like(buf)
        copy_ms, copy_med = timed(lambda: dst.view(torch.float32).copy_(buf.view(torch.float32)))
        copy_read = buf.numel() * 4 / copy_ms / 1e6
        say("  device-to-device copy of the source buffer (torch copy_, float32 view): %.3f ms (%.3f), %.1f GB/s read (and as much written)" % (
            copy_ms, copy_med, copy_read))
        del dst
        cases = [("full shutter, linear light, ", full, True, 0), ("full shutter, stored values,", full, False, 0)]
        if (W, H) == SHAPES[0]:
            cases += [("shutter 1,    linear light, ", pick, True, 0), ("full shutter, linear light, ", full, True, 1)]
        filled = None
        for name, plan, linear, shift in cases:
            if filled != shift:
                for i, f in enumerate(frames):                  # three frames share a picture: footage repeats, and the fill is quick
                    if i % 3 == 0:
                        picture = synth.gradient_noise_torch(W, H, 11 + i)
                    f[shift:shift + px].copy_(picture)
                torch.cuda.synchronize()
                filled = shift
            src = [f.data_ptr() + 4 * shift for f in frames]
            dptr = [o.data_ptr() + 4 * shift for o in outs]
            assert all(p % 16 == 4 * shift for p in src + dptr)
            call = lambda: nq.retime_frames_device(0, 0, src, dptr, W, H, plan, linear)
            call()
            torch.cuda.synchronize()
            for j in (0, plan.m - 1):
                used = sorted(set(int(s) for s in plan.source[plan.offset[j]:plan.offset[j + 1]]))
                for lo in (0, px - BAND):
                    part = {i: frames[i][shift + lo:shift + lo + BAND].cpu().numpy().reshape(1, BAND) for i in used}
                    some = [part.get(i, np.zeros((1, BAND), np.int32)) for i in range(N)]
                    k0, k1 = int(plan.offset[j]), int(plan.offset[j + 1])
                    want = retime_ref.mix(some, 1, [0, k1 - k0], plan.source[k0:k1], plan.weight[k0:k1], retime_ref.LINEAR if linear else 0)[0]
                    got = outs[j][shift + lo:shift + lo + BAND].cpu().numpy().reshape(1, BAND)
                    assert (got == want).all(), "output %d differs from the restatement (%s shift %d)" % (j, name, shift)
            span, med = timed(call)
            read = len(plan.source) * px * 4
            say("  %s %s path: %8.3f ms (%.3f) per call  %7.1f us per output  %7.1f GB/s read  %.3f of the copy's read rate" % (
                name, "one-pixel" if shift else "16-byte  ", span, med, span * 1e3 / plan.m, read / span / 1e6, (read / span / 1e6) / copy_read))
        del buf, frames, obuf, outs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
