"""What 10-bit YUV input costs (nq_frames_from_yuv16_device, nq_resample_frames_yuv16_device) on 16 device-resident 3840x2160 P010
frames, per transfer (SDR, PQ, HLG):
  (a) the 1:1 conversion against a device-to-device copy that moves the same bytes (7 per pixel: 3 read, 4 written);
  (b) the reduction to 960x540 by the fused call against the two-call sequence (convert, then nq_resample_frames_device), each also
      as a fraction of a device-to-device copy that moves what the fused call has to move (3 bytes read per pixel, 4 written per
      output pixel);
  the one-pixel path (every plane one sample behind a 16-byte boundary) once, in PQ.
All calls in one run; a warm-up, then the event spans of 5 calls: best, and the spread (worst - best) that a difference has to exceed.
No oracle.  A band of rows of every timed case is compared with the restatement in tests/yuv16_ref.py first.  The yardstick to read the
figures against is the 8-bit call's (profiles/r15/yuv_bench.txt): 0.83 of the copy's rate at 1:1, the fused call 0.73 of convert-then-
reduce.

    python tools/yuv16_bench.py [--reps 5] [--out profiles/r19/yuv16_bench.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, W, H, DW, DH = 16, 3840, 2160, 960, 540
BAND = 8                                             # output rows compared with the restatement (the ratio is 4 on both axes)


def p010_frame(seed):
    """One P010 frame as 16-bit words: a diagonal luma ramp over the whole range with noise, chroma waves; samples in the high bits."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = np.clip((xx + yy) * 1023 // (W + H - 2) + rng.integers(-24, 25, (H, W)), 0, 1023)
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    u = np.clip(512 + 300 * np.sin(cx / 97.0 + seed) + rng.integers(-16, 17, cx.shape), 0, 1023).astype(np.int64)
    v = np.clip(512 + 300 * np.cos(cy / 61.0 - seed) + rng.integers(-16, 17, cx.shape), 0, 1023).astype(np.int64)
    return np.concatenate([luma.reshape(-1), np.stack([u, v], -1).reshape(-1)]).astype(np.uint16) << 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    import yuv16_ref

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

    def copy_rate(nbytes):
        """(ms, spread, GB/s moved) of a device-to-device copy that reads and writes nbytes in all."""
        words = int(nbytes) // 8
        src = torch.zeros(words, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        ms, worst = timed(lambda: dst.copy_(src))
        return ms, worst - ms, 2 * words * 4 / ms / 1e6

    px, cpx = W * H, (W // 2) * (H // 2)
    pitch = (px + 2 * cpx + 7) // 8 * 8 + 8          # a frame's words, a 16-byte boundary, room for a shift of one sample
    say("10-bit YUV input on %d device-resident %dx%d P010 frames; library %s; best (worst - best) event span of %d calls after a warm-up" % (
        N, W, H, os.path.basename(nq.library_path()), args.reps))
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    host = [p010_frame(31 + i) for i in range(2)]     # two pictures, alternating
    buf = torch.zeros(N * pitch, dtype=torch.int16, device="cuda")
    full = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(N)]
    small = [torch.zeros(DW * DH, dtype=torch.int32, device="cuda") for _ in range(N)]
    small2 = [torch.zeros(DW * DH, dtype=torch.int32, device="cuda") for _ in range(N)]
    moved = N * px * 7.0
    moved_fused = N * (px * 3.0 + DW * DH * 4.0)
    c_ms, c_spread, c_rate = copy_rate(moved)
    say("device-to-device copy moving the 1:1 call's %.0f MB (torch copy_): %.3f ms (%.3f), %.1f GB/s moved" % (moved / 1e6, c_ms, c_spread, c_rate))
    f_ms, f_spread, f_rate = copy_rate(moved_fused)
    say("device-to-device copy moving the fused call's %.0f MB: %.3f ms (%.3f), %.1f GB/s moved" % (moved_fused / 1e6, f_ms, f_spread, f_rate))

    def place(shift):
        """The frames, every one `shift` samples behind a 16-byte boundary -> (y, u, v pointers)."""
        for i in range(N):
            buf[i * pitch + shift:i * pitch + shift + px + 2 * cpx].copy_(torch.from_numpy(host[i % 2].view(np.int16)))
        torch.cuda.synchronize()
        y = [buf.data_ptr() + 2 * (i * pitch + shift) for i in range(N)]
        return y, [p + 2 * px for p in y], [p + 2 * px + 2 for p in y]

    def check(flags, outs, reduced):
        for i in (0, N - 1):
            rows = BAND * H // DH if reduced else 2 * BAND
            planes = nq.yuv16_planes(host[i % 2], W, H, "p010")
            top = (planes[0][:rows], planes[1][:rows // 2], planes[2][:rows // 2])
            if reduced:
                want = yuv16_ref.resample([top], (DW, BAND), None, flags)[0]
                got = outs[i][:BAND * DW].cpu().numpy().reshape(BAND, DW)
            else:
                want = yuv16_ref.convert([top], flags)[0]
                got = outs[i][:rows * W].cpu().numpy().reshape(rows, W)
            assert (got == want).all(), "frame %d differs from the restatement (flags %d, reduced %s)" % (i, flags, reduced)

    ptr = lambda ts: [t.data_ptr() for t in ts]
    cases = [("sdr", 0, "SDR (BT.709), wide path"), ("pq", 0, "PQ (BT.2020), wide path"), ("hlg", 0, "HLG (BT.2020), wide path"),
             ("pq", 1, "PQ (BT.2020), one-pixel path")]
    placed = None
    for transfer, shift, name in cases:
        if placed != shift:
            y, u, v = place(shift)
            placed = shift
        kw = {"transfer": transfer}
        flags = yuv16_ref.MSB | {"sdr": yuv16_ref.BT709, "pq": yuv16_ref.BT2020 | yuv16_ref.PQ, "hlg": yuv16_ref.BT2020 | yuv16_ref.HLG}[transfer]
        convert = lambda: nq.frames_from_yuv16_device(y, u, v, W, H, W, W, 2, ptr(full), **kw)
        reduce_argb = lambda: nq.resample_frames_device(q, ptr(full), W, H, ptr(small2), (DW, DH))
        fused = lambda: nq.resample_frames_yuv16_device(y, u, v, W, H, W, W, 2, ptr(small), (DW, DH), **kw)
        two = lambda: (convert(), reduce_argb())
        convert(); fused(); reduce_argb()
        torch.cuda.synchronize()
        check(flags, full, False)
        check(flags, small, True)
        assert all((a == b).all() for a, b in zip(small, small2)), "the fused call differs from the two-call sequence"
        say("%s:" % name)
        ms, worst = timed(convert)
        say("  (a) 1:1 conversion             %8.3f ms (%.3f)  %7.1f GB/s moved  %.3f of the copy's rate" % (
            ms, worst - ms, moved / ms / 1e6, (moved / ms / 1e6) / c_rate))
        ms2, worst2 = timed(two)
        say("  (b) convert, then reduce       %8.3f ms (%.3f)" % (ms2, worst2 - ms2))
        ms1, worst1 = timed(fused)
        say("  (b) fused call                 %8.3f ms (%.3f)  %.2f of the two-call sequence  %.3f of its copy's rate" % (
            ms1, worst1 - ms1, ms1 / ms2, (moved_fused / ms1 / 1e6) / f_rate))
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
