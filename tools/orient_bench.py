"""What orientation costs (nq_orient_frames_device and the *_oriented calls) on 16 device-resident 3840x2160 frames.  Each case is
timed against a device-to-device copy that moves the same bytes:
  (a) ARGB frames at codes 3 (180 degrees: rows reversed, no transpose), 5 (transpose) and 6 (90 degrees clockwise): 8 bytes per pixel;
  (b) the same frames as NV12 through nq_frames_from_yuv_oriented_device (5.5 bytes per pixel) and through the two calls it replaces
      (convert, then orient: 13.5 bytes per pixel), at codes 3 and 6;
  (c) those to 540x960 (code 6) through nq_resample_frames_yuv_oriented_device, against the unoriented fused reducer to 960x540.
All cases in one run.  A span is the device-event time of INNER calls in a row; after a warm-up span, the best of `reps` spans and
the spread (worst - best) that a difference has to exceed, per call.  No oracle: a band of every timed result is compared with the
restatements in tests/orient_ref.py and tests/yuv_ref.py first.

    python tools/orient_bench.py [--reps 7] [--out profiles/r16/orient_bench.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, W, H, DW, DH = 16, 3840, 2160, 540, 960
INNER = 10                                           # calls per timed span
BAND = 16                                            # source rows / columns compared with the restatement


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import orient_ref
    import yuv_ref

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        """(best, worst) per-call time over reps spans of INNER calls after a warm-up span, ms."""
        spans = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(INNER):
                call()
            b.record()
            b.synchronize()
            spans.append(a.elapsed_time(b) / INNER)
        return min(spans[1:]), max(spans[1:])

    def copy_rate(nbytes):
        """GB/s moved by a device-to-device copy (torch copy_) that reads and writes nbytes / 2 each."""
        words = int(nbytes) // 8
        src = torch.zeros(words, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        ms, worst = timed(lambda: dst.copy_(src))
        rate = 2 * words * 4 / ms / 1e6
        say("  device-to-device copy moving %.0f MB: %.3f ms (%.3f), %.1f GB/s moved" % (2 * words * 4 / 1e6, ms, worst - ms, rate))
        return rate

    px, cpx = W * H, (W // 2) * (H // 2)
    pitch = (px + 2 * cpx + 15) // 16 * 16
    say("orientation on %d device-resident %dx%d frames; library %s; per call: best (worst - best) of %d spans of %d calls after a warm-up span" % (
        N, W, H, os.path.basename(nq.library_path()), args.reps, INNER))
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    host = [synth.yuv420(W, H, 31 + i, "nv12") for i in range(2)]                  # two pictures, alternating
    buf = torch.zeros(N * pitch, dtype=torch.uint8, device="cuda")
    for i in range(N):
        buf[i * pitch:i * pitch + px + 2 * cpx].copy_(torch.from_numpy(host[i % 2]))
    y = [buf.data_ptr() + i * pitch for i in range(N)]
    u, v = [p + px for p in y], [p + px + 1 for p in y]
    full = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(N)]
    turned = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(N)]
    turned2 = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(N)]
    small = [torch.zeros(DW * DH, dtype=torch.int32, device="cuda") for _ in range(N)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    kw = {"bt709": True}
    convert = lambda: nq.frames_from_yuv_device(q, y, u, v, W, H, W, W, 2, ptr(full), **kw)
    convert()
    torch.cuda.synchronize()
    planes = [nq.yuv_planes(h, W, H, "nv12") for h in host]
    top = [(p[0][:BAND], p[1][:BAND // 2], p[2][:BAND // 2]) for p in planes]      # the first BAND source rows
    top_argb = yuv_ref.convert(top, yuv_ref.BT709)

    def check(outs, code):
        """The part of frames 0 and N - 1 that the first BAND source rows give, against the restatement."""
        ow, oh = orient_ref.oriented_size(W, H, code)
        for i in (0, N - 1):
            want = orient_ref.orient(top_argb[i % 2], code)
            got = outs[i].cpu().numpy().reshape(oh, ow)
            part = {3: got[-BAND:], 5: got[:, :BAND], 6: got[:, -BAND:]}[code]
            assert part.shape == want.shape and (part == want).all(), "frame %d differs from the restatement (code %d)" % (i, code)

    say("(a) ARGB to ARGB, 8 bytes per pixel:")
    rate_a = copy_rate(N * px * 8)
    for code in (3, 5, 6):
        call = lambda: nq.orient_frames_device(q, ptr(full), W, H, ptr(turned), code)
        call()
        torch.cuda.synchronize()
        check(turned, code)
        ms, worst = timed(call)
        say("  code %d                          %8.3f ms (%.3f)  %7.1f GB/s moved  %.3f of the copy's rate" % (
            code, ms, worst - ms, N * px * 8 / ms / 1e6, (N * px * 8 / ms / 1e6) / rate_a))

    say("(b) NV12 to oriented ARGB, 5.5 bytes per pixel:")
    rate_b = copy_rate(N * px * 5.5)
    for code in (3, 6):
        fused = lambda: nq.frames_from_yuv_device(q, y, u, v, W, H, W, W, 2, ptr(turned), orient=code, **kw)
        two = lambda: (convert(), nq.orient_frames_device(q, ptr(full), W, H, ptr(turned2), code))
        fused(); two()
        torch.cuda.synchronize()
        check(turned, code)
        assert all((a == b).all() for a, b in zip(turned, turned2)), "the fused call differs from convert, then orient"
        ms2, worst2 = timed(two)
        ms1, worst1 = timed(fused)
        say("  code %d  convert, then orient    %8.3f ms (%.3f)" % (code, ms2, worst2 - ms2))
        say("  code %d  fused call              %8.3f ms (%.3f)  %7.1f GB/s moved  %.3f of the copy's rate  %.2f of the two calls" % (
            code, ms1, worst1 - ms1, N * px * 5.5 / ms1 / 1e6, (N * px * 5.5 / ms1 / 1e6) / rate_b, ms1 / ms2))

    say("(c) NV12 to %dx%d, code 6 (the reducer runs on the source, the small result is oriented):" % (DW, DH))
    plain = lambda: nq.resample_frames_yuv_device(q, y, u, v, W, H, W, W, 2, ptr(small), (DH, DW), **kw)
    oriented = lambda: nq.resample_frames_yuv_device(q, y, u, v, W, H, W, W, 2, ptr(small), (DW, DH), orient=6, **kw)
    plain()
    torch.cuda.synchronize()
    keep = [s.cpu().numpy().reshape(DW, DH) for s in (small[0], small[N - 1])]     # unoriented: DH wide, DW tall
    oriented()
    torch.cuda.synchronize()
    for k, i in enumerate((0, N - 1)):
        assert (small[i].cpu().numpy().reshape(DH, DW) == orient_ref.orient(keep[k], 6)).all(), "the oriented reduction differs"
    ms0, worst0 = timed(plain)
    ms1, worst1 = timed(oriented)
    say("  fused reducer, unoriented       %8.3f ms (%.3f)" % (ms0, worst0 - ms0))
    say("  nq_resample_frames_yuv_oriented %8.3f ms (%.3f)  %.3f of the unoriented call" % (ms1, worst1 - ms1, ms1 / ms0))
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
