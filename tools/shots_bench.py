"""What shot detection costs (nq_frame_signatures_device / nq_detect_shots_device): time per call for device-resident frames, on
gradient_noise content (every lane its own values) and on flat frames (every pixel into four counters: the same-address case), on
the vector and on the scalar path; the bytes read per second against a device-to-device copy of the same buffer timed in the same
run; the call's fixed cost on 8x8 frames; and numpy computing the same signatures on the host.  No oracle.  The signatures of every
timed input are compared with numpy's first.

    python tools/shots_bench.py [--size 4096] [--frames 8] [--reps 50] [--out profiles/r11/shots_bench.txt]

NQ_LIB=<another build of the library> (build.py NQ_BUILD_TAG) times a variant of the kernel."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import shots_ref

    W = H = args.size
    n, px = args.frames, args.size * args.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("shot detection on %d device-resident frames of %dx%d (%.0f MB read per call); library %s" % (
        n, W, H, n * px * 4 / 1e6, os.path.basename(nq.library_path())))
    PAD = 4                                          # room to start every frame one element late (the scalar path)
    buf = torch.zeros(n * (px + PAD), dtype=torch.int32, device="cuda")
    frames = [buf[i * (px + PAD):(i + 1) * (px + PAD)] for i in range(n)]
    ptr = lambda shift: [f.data_ptr() + 4 * shift for f in frames]
    assert all(p % 16 == 0 for p in ptr(0))
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))

    def fill(content, shift):
        for i, f in enumerate(frames):
            if content == "noise":
                f[shift:shift + px].copy_(synth.gradient_noise_torch(W, H, 11 + i))
            else:
                f[shift:shift + px].fill_(-(0x01000000 - 0x336699 - 0x010101 * i))      # 0xFF336699 + 0x010101 i, one colour per frame
        torch.cuda.synchronize()

    def timed(call):
        """(best event span, best and median host wall time) of reps calls after a warm-up, ms."""
        spans, walls = [], []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            call()
            b.record()
            b.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            spans.append(a.elapsed_time(b))
        return min(spans[1:]), min(walls[1:]), float(np.median(walls[1:]))

    # the yardstick: the same bytes through a device-to-device copy (read + write)
    dst = torch.empty_like(buf)
    fill("noise", 0)
    copy_ms, _, _ = timed(lambda: dst.view(torch.float32).copy_(buf.view(torch.float32)))
    copy_bytes = 2 * buf.numel() * 4
    say("device-to-device copy of the buffer (torch copy_, float32 view): %.3f ms, %.1f GB/s read + written, %.1f GB/s read" % (
        copy_ms, copy_bytes / copy_ms / 1e6, copy_bytes / 2 / copy_ms / 1e6))
    del dst
    say("per call: best event span on the stream around nq_frame_signatures_device (pointer-table upload, zeroing %d KB of counters, one "
        "launch, %d KB read back), best and median host wall time of the call (it returns with the signatures on the host); best of %d" % (
            n * 4, n * 4, args.reps))
    results, numpy_s = {}, 0.0
    for content, shift in (("noise", 0), ("flat", 0), ("noise", 1), ("flat", 1)):
        fill(content, shift)
        got = nq.frame_signatures_device(q, ptr(shift), W, H)
        check = [0, n - 1]                           # numpy takes about a second per frame of this size
        t0 = time.perf_counter()
        want = shots_ref.signatures([frames[i][shift:shift + px].cpu().numpy() for i in check])
        numpy_s = (time.perf_counter() - t0) / len(check) if content == "noise" and shift == 0 else numpy_s
        assert (got[check] == want).all(), "signatures differ from numpy's on %s content, shift %d" % (content, shift)
        assert (got.sum(axis=2) == px).all()
        span, wall, med = timed(lambda: nq.frame_signatures_device(q, ptr(shift), W, H))
        results[content, shift] = span
        say("%-5s content, %s path: %8.3f ms per call  %7.1f us per frame  %7.1f GB/s read  %.3f of the copy's read rate   (host wall %.3f ms "
            "best, %.3f median)" % (content, "scalar" if shift else "vector", span, span * 1e3 / n, n * px * 4 / span / 1e6,
                                    (n * px * 4 / span) / (copy_bytes / 2 / copy_ms), wall, med))
    say("flat / noise: vector path %.3f, scalar path %.3f" % (results["flat", 0] / results["noise", 0], results["flat", 1] / results["noise", 1]))
    say("numpy on the host (np.bincount per channel, tests/shots_ref.py): %.1f ms per frame, %.0fx the vector path's time per frame on noise" % (
        numpy_s * 1e3, numpy_s * 1e3 / (results["noise", 0] / n)))
    fill("noise", 0)
    span, wall, med = timed(lambda: nq.detect_shots_device(q, ptr(0), W, H))
    say("nq_detect_shots_device (signatures + the rule on the host): %.3f ms per call (host wall %.3f best)" % (span, wall))
    small = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(n)]
    span, wall, med = timed(lambda: nq.frame_signatures_device(q, [t.data_ptr() for t in small], 8, 8))
    say("fixed cost: the same spans around a call on %d frames of 8x8: %.3f ms event span, %.3f ms host wall (table upload, zeroing, launch, "
        "read-back and the wait for it; part of every figure above)" % (n, span, wall))
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
