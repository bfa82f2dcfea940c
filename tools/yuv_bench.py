"""What YUV input costs (nq_frames_from_yuv_device, nq_resample_frames_yuv_device) on 16 device-resident 3840x2160 frames:
  (a) the 1:1 conversion of NV12 frames against a device-to-device copy that moves the same bytes (5.5 per pixel: 1.5 read, 4 written);
  (b) the reduction to 960x540 by the fused call, by the two-call sequence (convert, then nq_resample_frames_device) and, as the
      yardstick, by the ARGB reducer alone on the converted frames; I420 and the byte path (every plane one byte behind a 16-byte
      boundary) once each.
All calls in one run; a warm-up, then the event spans of 5 calls: best, and the spread (worst - best) that a difference has to exceed.
No oracle.  A band of rows of every timed case is compared with the restatement in tests/yuv_ref.py first.

    python tools/yuv_bench.py [--reps 5] [--out profiles/r15/yuv_bench.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, W, H, DW, DH = 16, 3840, 2160, 960, 540
BAND = 8                                             # output rows compared with the restatement (the ratio is 4 on both axes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import yuv_ref

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        """(best, worst) event span of reps calls after a warm-up, ms."""
        spans = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            call()
            b.record()
            b.synchronize()
            spans.append(a.elapsed_time(b))
        return min(spans[1:]), max(spans[1:])

    px, cpx = W * H, (W // 2) * (H // 2)
    pitch = (px + 2 * cpx + 15) // 16 * 16 + 16       # a frame's bytes, a 16-byte boundary, room for a shift of one byte
    say("YUV input on %d device-resident %dx%d frames; library %s; best (worst - best) event span of %d calls after a warm-up" % (
        N, W, H, os.path.basename(nq.library_path()), args.reps))
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    host = {lay: [synth.yuv420(W, H, 31 + i, lay) for i in range(2)] for lay in ("nv12", "i420")}      # two pictures, alternating
    buf = torch.zeros(N * pitch, dtype=torch.uint8, device="cuda")
    full = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(N)]
    small = [torch.zeros(DW * DH, dtype=torch.int32, device="cuda") for _ in range(N)]
    small2 = [torch.zeros(DW * DH, dtype=torch.int32, device="cuda") for _ in range(N)]
    moved = N * px * 5.5

    # the yardstick of (a): a device-to-device copy that reads and writes 2.75 bytes per pixel
    words = int(N * px * 2.75) // 4
    a_src = torch.zeros(words, dtype=torch.float32, device="cuda")
    a_dst = torch.empty_like(a_src)
    copy_ms, copy_worst = timed(lambda: a_dst.copy_(a_src))
    copy_rate = 2 * words * 4 / copy_ms / 1e6
    say("device-to-device copy moving the same %.0f MB (torch copy_): %.3f ms (%.3f), %.1f GB/s moved" % (
        moved / 1e6, copy_ms, copy_worst - copy_ms, copy_rate))
    del a_src, a_dst

    def place(layout, shift):
        """The frames in `layout`, every one `shift` bytes behind a 16-byte boundary -> (y, u, v pointers, c_stride, c_step)."""
        for i in range(N):
            buf[i * pitch + shift:i * pitch + shift + px + 2 * cpx].copy_(torch.from_numpy(host[layout][i % 2]))
        torch.cuda.synchronize()
        y = [buf.data_ptr() + i * pitch + shift for i in range(N)]
        if layout == "nv12":
            return y, [p + px for p in y], [p + px + 1 for p in y], W, 2
        return y, [p + px for p in y], [p + px + cpx for p in y], W // 2, 1

    def check(layout, flags_kw, outs, reduced):
        for i in (0, N - 1):
            rows = BAND * H // DH if reduced else 2 * BAND
            planes = nq.yuv_planes(host[layout][i % 2], W, H, layout)
            top = (planes[0][:rows], planes[1][:rows // 2], planes[2][:rows // 2])
            flags = (yuv_ref.BT709 if flags_kw.get("bt709") else 0) | (yuv_ref.FULL_RANGE if flags_kw.get("full_range") else 0)
            if reduced:
                want = yuv_ref.resample([top], (DW, BAND), None, flags)[0]
                got = outs[i][:BAND * DW].cpu().numpy().reshape(BAND, DW)
            else:
                want = yuv_ref.convert([top], flags)[0]
                got = outs[i][:rows * W].cpu().numpy().reshape(rows, W)
            assert (got == want).all(), "frame %d differs from the restatement (%s, reduced %s)" % (i, layout, reduced)

    kw = {"bt709": True}
    ptr = lambda ts: [t.data_ptr() for t in ts]
    for layout, shift, name in (("nv12", 0, "NV12, wide path"), ("i420", 0, "I420, wide path"), ("nv12", 1, "NV12, byte path")):
        y, u, v, cs, step = place(layout, shift)
        convert = lambda: nq.frames_from_yuv_device(q, y, u, v, W, H, W, cs, step, ptr(full), **kw)
        reduce_argb = lambda: nq.resample_frames_device(q, ptr(full), W, H, ptr(small2), (DW, DH))
        fused = lambda: nq.resample_frames_yuv_device(q, y, u, v, W, H, W, cs, step, ptr(small), (DW, DH), **kw)
        two = lambda: (convert(), reduce_argb())
        convert(); fused(); reduce_argb()
        torch.cuda.synchronize()
        check(layout, kw, full, False)
        check(layout, kw, small, True)
        assert all((a == b).all() for a, b in zip(small, small2)), "the fused call differs from the two-call sequence"
        say("%s:" % name)
        ms, worst = timed(convert)
        say("  (a) 1:1 conversion             %8.3f ms (%.3f)  %7.1f GB/s moved  %.3f of the copy's rate" % (
            ms, worst - ms, moved / ms / 1e6, (moved / ms / 1e6) / copy_rate))
        if shift == 0 and layout == "nv12":
            ms, worst = timed(reduce_argb)
            say("  (b) ARGB reducer alone         %8.3f ms (%.3f)  (the yardstick: the converted frames to %dx%d)" % (ms, worst - ms, DW, DH))
        ms2, worst2 = timed(two)
        say("  (b) convert, then reduce       %8.3f ms (%.3f)" % (ms2, worst2 - ms2))
        ms1, worst1 = timed(fused)
        say("  (b) fused call                 %8.3f ms (%.3f)  %.2f of the two-call sequence" % (ms1, worst1 - ms1, ms1 / ms2))
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
