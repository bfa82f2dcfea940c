"""What the temporal hold (nq_hold_frames_device) buys on footage-like input, and what it costs: a still background with +-2 of noise
per channel and frame and a small moving sprite (tests/hold_ref.py noisy_sprite_sequence), PnnLABQuantizer, convert_frames_device with
equal seeds in tiled mode; the bytes of the delta GIF and of the APNG with the hold off and on, and the hold kernel's time measured
with events on the handle's stream around calls that do not fetch the counts.

    python tools/hold_bench.py [--size 1024] [--frames 16] [--colors 256] [--hold 4] [--reps 20] [--out profiles/r08/hold_bench.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--colors", type=int, default=256)
    ap.add_argument("--hold", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    import hold_ref

    W = H = args.size
    n, K, T = args.frames, args.colors, args.hold
    px = W * H
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("temporal hold on %d frames of %dx%d: noisy_sprite_sequence (noise -2..+2 per channel and frame, 12x12 sprite), PnnLABQuantizer, "
        "convert_frames_device(%d, true), equal seeds, tiled mode" % (n, W, H, K))
    frames, boxes = hold_ref.noisy_sprite_sequence(H, W, n, 3)
    PAD = 8                                          # room to start every buffer one element late (the scalar path)
    room = lambda dt: [torch.zeros(px + PAD, dtype=dt, device="cuda") for _ in range(n)]
    src, outs, idxs = room(torch.int32), room(torch.int32), room(torch.int16)
    for s, f in zip(src, frames):
        s[:px].copy_(torch.from_numpy(f.reshape(-1)))
    ptr = lambda ts, shift=0: [t.data_ptr() + shift * t.element_size() for t in ts]
    q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
    pal = nq.convert_frames_device(q, ptr(src), [W] * n, [H] * n, K, True, ptr(outs), ptr(idxs), seeds=[0] * n)
    torch.cuda.synchronize()
    keep_src, keep_idx, keep_out = [t.clone() for t in src], [t.clone() for t in idxs], [t.clone() for t in outs]
    say("palette: %d colours" % len(pal))

    def sizes(tag):
        gif, rects = nq.encode_gif_delta_device(q, ptr(idxs), W, H, pal, [4] * n, 0, return_rects=True)
        png = nq.encode_apng_device(q, ptr(idxs), W, H, pal, [4] * n, 0)
        area = int((rects[1:, 2].astype(np.int64) * rects[1:, 3]).sum())
        say("%-10s delta GIF %12d bytes   APNG %12d bytes   rectangles of frames 1.. cover %.4f of their pixels" % (
            tag, len(gif), len(png), area / ((n - 1) * px)))
        return len(gif), len(png)

    def restore(shift=0):
        for t, k in zip(src + idxs + outs, keep_src + keep_idx + keep_out):
            t[shift:shift + px].copy_(k[:px])
        torch.cuda.synchronize()

    def timed(with_out, shift):
        best = None
        for _ in range(args.reps + 1):              # (the first run is a warm-up)
            restore(shift)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            nq.hold_frames_device(q, ptr(src, shift), ptr(idxs, shift), W, H, T, ptr(outs, shift) if with_out else None, counts=False)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            best = ms if best is None or ms < best else best
        return best

    g0, p0 = sizes("hold off:")
    say("kernel time: best of %d event spans around nq_hold_frames_device(threshold %d) without counts (the span holds the upload of the "
        "pointer table and one launch); traffic counted per pixel of frames 1..%d: 6 B read + 2 B written (index stream only), with the "
        "ARGB outputs 10 B read + 6 B written; frame 0 is read once on top and not counted" % (args.reps, T, n - 1))
    for name, with_out, shift, bytes_px in (("vector path, indices only    ", False, 0, 8), ("vector path, with ARGB outputs", True, 0, 16),
                                            ("scalar path, indices only    ", False, 1, 8), ("scalar path, with ARGB outputs", True, 1, 16)):
        ms = timed(with_out, shift)
        say("%s %8.3f ms per call  %7.1f us per frame  %7.1f GB/s" % (name, ms, ms * 1e3 / (n - 1), (n - 1) * px * bytes_px / (ms * 1e-3) / 1e9))
    # the same span around a call that moves next to nothing: what the table upload and the launch cost by themselves
    ts, ti = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(n)], [torch.zeros(64, dtype=torch.int16, device="cuda") for _ in range(n)]
    fixed = None
    for _ in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nq.hold_frames_device(q, ptr(ts), ptr(ti), 8, 8, T, counts=False)
        b.record()
        b.synchronize()
        fixed = a.elapsed_time(b) if fixed is None else min(fixed, a.elapsed_time(b))
    say("fixed cost: the same span around a call on %d frames of 8x8: %.3f ms (table upload + launch; part of every figure above)" % (n, fixed))
    restore(0)
    held = nq.hold_frames_device(q, ptr(src), ptr(idxs), W, H, T, ptr(outs))
    say("held pixels per frame 1..: min %.4f  mean %.4f of the frame" % (held[1:].min() / px, held[1:].mean() / px))
    g1, p1 = sizes("hold=%d:" % T)
    say("hold=%d / hold off: delta GIF %.4fx the bytes, APNG %.4fx the bytes" % (T, g1 / g0, p1 / p0))
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
