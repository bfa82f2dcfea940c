"""What the quality measurement costs, and what it says about the two ditherers (nq_compare_frames_device / nq_compare_indexed_device).
No oracle.

(a) Speed: ms per call over 8 device-resident pairs of frames -- ARGB form and indexed form, linear on and off, the 16-byte path and the
one-pixel path (every frame one element behind a 16-byte boundary) -- beside a yardstick timed in the same run: torch's
device-to-device copy of the source and output frames, which reads the bytes the ARGB form reads.  Every time is also shown as the
call's read rate over the copy's.  Before it is timed, every configuration is compared with the numpy restatement
(tests/compare_ref.py) on a 256 x 256 pair.  A time is the best event span of `reps` calls after a warm-up call.

(b) Figures: 16 frames of noisy-sprite footage (tests/hold_ref.py): psnr, lf_psnr and ssim (Quality.total over the frames) of error
diffusion against the ordered dither at K = 256 and K = 16.

    python tools/compare_bench.py [--size 4096] [--frames 8] [--clip-size 1024] [--clip-frames 16] [--reps 10] [--out profiles/r17/compare_bench.txt]

NQ_LIB=<another build of the library> (build.py NQ_BUILD_TAG) times a variant of the kernel."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--clip-size", type=int, default=1024)
    ap.add_argument("--clip-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-figures", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import compare_ref
    import hold_ref

    W = H = args.size
    N = args.frames
    px = W * H
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("quality measurement on %d device-resident pairs of %dx%d (ARGB form: %.0f MB read per call, indexed form: %.0f MB); library %s" % (
        N, W, H, N * px * 8 / 1e6, N * px * 6 / 1e6, os.path.basename(nq.library_path())))
    pitch = px + 8                                                        # room to start every frame one element late (the one-pixel path)
    src = torch.zeros(N * pitch, dtype=torch.int32, device="cuda")
    out = torch.zeros(N * pitch, dtype=torch.int32, device="cuda")
    idx = torch.zeros(N * pitch, dtype=torch.int16, device="cuda")
    res = torch.zeros(16 * N, dtype=torch.int64, device="cuda")
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 0
    K = 256
    palette = np.random.default_rng(K).integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000)

    def fill(shift):
        """Sources: gradient_noise; outputs: the source with the low three bits of every colour channel taken from another frame; index
        maps: the low byte of the source."""
        for i in range(N):
            s = synth.gradient_noise_torch(W, H, 11 + i)
            o = s ^ (synth.gradient_noise_torch(W, H, 111 + i) & 0x00070707)
            src[i * pitch + shift:i * pitch + shift + px].copy_(s)
            out[i * pitch + shift:i * pitch + shift + px].copy_(o)
            idx[i * pitch + shift:i * pitch + shift + px].copy_((s & 255).to(torch.int16))
        torch.cuda.synchronize()

    def timed(call):
        """best event span of reps calls after a warm-up, ms"""
        spans = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            call()
            b.record()
            b.synchronize()
            spans.append(a.elapsed_time(b))
        return min(spans[1:])

    def ptrs(t, size, shift, n=N):
        return [t.data_ptr() + size * (i * pitch + shift) for i in range(n)]

    small = torch.zeros(2 * N * 64, dtype=torch.int32, device="cuda")
    sp = [small.data_ptr() + 256 * i for i in range(2 * N)]
    fixed = timed(lambda: nq.compare_frames_device(sp[:N], sp[N:], [8] * N, [8] * N, res.data_ptr()))
    say("fixed cost: a call on %d pairs of 8x8: %.3f ms event span (one memset, one launch)" % (N, fixed))
    fill(0)
    dst = torch.empty(2 * N * px, dtype=torch.float32, device="cuda")

    def copy():
        dst[:N * px].copy_(src.view(torch.float32)[:N * px])
        dst[N * px:].copy_(out.view(torch.float32)[:N * px])
    copy_ms = timed(copy)
    copy_rate = N * px * 8 / copy_ms / 1e6
    say("device-to-device copy of the source and output frames (torch copy_, float32 view, two copies): %.3f ms, %.1f GB/s read" % (
        copy_ms, copy_rate))
    del dst
    say("per call = event span of the asynchronous call, best of %d; rate = bytes the form reads / span" % args.reps)
    for shift in (0, 1):
        if shift:
            fill(shift)
        s, o, x = ptrs(src, 4, shift), ptrs(out, 4, shift), ptrs(idx, 2, shift)
        crop_s = src[shift:shift + 65536].cpu().numpy().reshape(256, 256)
        crop_o = out[shift:shift + 65536].cpu().numpy().reshape(256, 256)
        crop_x = idx[shift:shift + 65536].cpu().numpy().view(np.uint16).reshape(256, 256)
        for form in ("ARGB", "indexed"):
            for linear in (True, False):
                if form == "ARGB":
                    call = lambda s=s, o=o, n=N, w=W, h=H: nq.compare_frames_device(s[:n], o[:n], [w] * n, [h] * n, res.data_ptr(), linear=linear)
                    want = compare_ref.compare(crop_s, crop_o, int(linear))
                    nbytes = 8
                else:
                    call = lambda s=s, o=x, n=N, w=W, h=H: nq.compare_indexed_device(s[:n], o[:n], palette, [w] * n, [h] * n, res.data_ptr(),
                                                                                     linear=linear)
                    want = compare_ref.compare_indexed([crop_s], [crop_x], palette, int(linear))[0]
                    nbytes = 6
                call(n=1, w=256, h=256)
                torch.cuda.synchronize()
                assert res[:16].cpu().numpy().tolist() == want.tolist(), (form, linear, shift)
                t = timed(call)
                rate = N * px * nbytes / t / 1e6
                say("%-7s form  %s  %s path: %8.3f ms per call  %7.1f GB/s read  %4.2f of the copy's rate" % (
                    form, "linear" if linear else "stored", "one-pixel" if shift else "16-byte  ", t, rate, rate / copy_rate))
    del src, out, idx

    if not args.skip_figures:
        S, F = args.clip_size, args.clip_frames
        say("")
        say("%d frames of %dx%d noisy-sprite footage (hold_ref.noisy_sprite_sequence, +-2 of noise per channel and frame), LAB kind; "
            "Quality.total over the frames, linear block means" % (F, S, S))
        frames, _ = hold_ref.noisy_sprite_sequence(S, S, F, 3)
        for K in (256, 16):
            runs = [("error diffusion, equal seeds", lambda: nq.convert_frames(1, frames, K, True, seeds=[5] * F))]
            runs += [("ordered=%d" % L, lambda L=L: nq.convert_frames_ordered(1, frames, K, L)) for L in (0, 16, 32, 64, 255)]
            for label, run in runs:
                pal, outs = run()
                q = nq.Quality.total(nq.compare_frames(frames, [o.argb for o in outs]))
                same = nq.Quality.total(nq.compare_indexed(frames, [o.index for o in outs], pal))
                assert same.slots.tolist() == q.slots.tolist()
                say("K=%3d %-30s psnr %6.2f dB   lf_psnr %6.2f dB   ssim %.4f   worst block %.4f   max diff %d" % (
                    K, label, q.psnr, q.lf_psnr, q.ssim, q.worst_block, q.max_diff))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
