"""What the ordered dither costs and what it buys (nq_dither_ordered_device / the converters' ordered= keyword).  No oracle.

(a) Speed: ms per call over 8 device-resident frames, at K = 256 and 16, with and without the ARGB output, on the vector and on the
scalar path, on gradient_noise and on flat frames -- beside two yardsticks timed in the same run over the same frames: a palette_error
pass (nq_refine_palette_device, iterations 0) and torch's device-to-device copy.  Every timed input is first compared with the numpy
restatement (tests/ordered_ref.py) on a crop.  A time is the event span of the call (no statistics: the call is asynchronous) minus
nothing; the call's fixed cost, its span on 8 frames of 8x8, is printed on its own line.

(b) Bytes: 16 frames of noisy-sprite footage (tests/hold_ref.py) to a delta GIF and an APNG: error diffusion + hold=4 against
ordered=L with and without hold=4 and lossy=16 (GIF only), L = 16, 32, 64, with the squared ARGB error of the index maps each file was
encoded from (after the hold, before the lossy step, which the encoder applies inside its chains).

    python tools/ordered_bench.py [--size 4096] [--frames 8] [--clip-size 1024] [--clip-frames 16] [--reps 10] [--out profiles/r14/ordered_bench.txt]

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
    ap.add_argument("--skip-bytes", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import hold_ref
    import ordered_ref

    W = H = args.size
    N = args.frames
    px = W * H
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("ordered dither on %d device-resident frames of %dx%d (%.0f MB read per call); library %s" % (
        N, W, H, N * px * 4 / 1e6, os.path.basename(nq.library_path())))
    pitch = px + 8                                                        # room to start every frame one element late (the scalar path)
    src = torch.zeros(N * pitch, dtype=torch.int32, device="cuda")
    out = torch.zeros(N * pitch, dtype=torch.int32, device="cuda")
    idx = torch.zeros(N * pitch, dtype=torch.int16, device="cuda")
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 0
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))

    def fill(content, shift):
        for i in range(N):
            if content == "noise":
                src[i * pitch + shift:i * pitch + shift + px].copy_(synth.gradient_noise_torch(W, H, 11 + i))
            else:
                src[i * pitch + shift:i * pitch + shift + px].fill_(-(0x01000000 - 0x336699) + i)       # 0xFF336699 + i
        torch.cuda.synchronize()

    def timed(call, reps=None):
        """best event span of reps calls after a warm-up, ms"""
        spans = []
        for _ in range((reps or args.reps) + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            call()
            b.record()
            b.synchronize()
            spans.append(a.elapsed_time(b))
        return min(spans[1:])

    def palette(K):
        rng = np.random.default_rng(K)
        return rng.integers(0, 1 << 24, K).astype(np.uint32) | np.uint32(0xFF000000)

    def ptrs(t, size, shift):
        return [t.data_ptr() + size * (i * pitch + shift) for i in range(N)]

    small = torch.zeros(N * 64, dtype=torch.int32, device="cuda")
    small_idx = torch.zeros(N * 64, dtype=torch.int16, device="cuda")
    fixed = timed(lambda: nq.dither_ordered_device(q, [small.data_ptr() + 256 * i for i in range(N)], [8] * N, [8] * N, palette(16), 32,
                                                   [small_idx.data_ptr() + 128 * i for i in range(N)]))
    say("fixed cost: a call on %d frames of 8x8, no statistics: %.3f ms event span (table and palette upload, one launch)" % (N, fixed))
    fill("noise", 0)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.view(torch.float32).copy_(src.view(torch.float32)))
    say("device-to-device copy of the frames (torch copy_, float32 view): %.3f ms, %.1f GB/s read" % (copy_ms, N * px * 4 / copy_ms / 1e6))
    del dst
    say("per call = event span, limit 64; error pass = nq_refine_palette_device, iterations 0, over the same frames (its span includes its "
        "read-back and wait); best of %d" % args.reps)
    for content in ("noise", "flat"):
        for shift in (0, 1):
            fill(content, shift)
            s, o, x = ptrs(src, 4, shift), ptrs(out, 4, shift), ptrs(idx, 2, shift)
            crop = src[shift:shift + 65536].cpu().numpy().reshape(256, 256)
            for K in (256, 16):
                pal = palette(K)
                st = nq.dither_ordered_device(q, s[:1], [256], [256], pal, 64, x[:1], o[:1], return_stats=True)
                widx, wout, wst = ordered_ref.dither([crop], pal, 64)
                assert st.tolist() == wst.tolist() and (idx[shift:shift + 65536].cpu().numpy().view(np.uint16) == widx[0].reshape(-1)).all() and \
                    (out[shift:shift + 65536].cpu().numpy().view(np.uint32) == wout[0].reshape(-1)).all(), (content, shift, K)
                err = timed(lambda: nq.refine_palette_device(q, s, [W] * N, [H] * N, pal, 0))
                for argb in (False, True):
                    for stats in (False, True):
                        t = timed(lambda: nq.dither_ordered_device(q, s, [W] * N, [H] * N, pal, 64, x, o if argb else None, return_stats=stats))
                        say("%-5s %s path K=%3d %s %s: %8.3f ms per call  %7.1f GB/s read  %5.2fx the copy  %5.2fx the error pass (%.3f ms)  "
                            "%6.1f Gpixel-entries/s" % (content, "scalar" if shift else "vector", K, "index+argb" if argb else "index only",
                                                        "with stats" if stats else "no stats  ", t, N * px * 4 / t / 1e6, t / copy_ms, t / err, err,
                                                        N * px * K / t / 1e6))
    q.close()
    del src, out, idx

    if not args.skip_bytes:
        S, F, K = args.clip_size, args.clip_frames, 256
        say("")
        say("bytes of %d frames of %dx%d noisy-sprite footage (hold_ref.noisy_sprite_sequence, +-2 of noise per channel and frame), LAB kind, "
            "K = %d, one handle per file; error = squared ARGB error of the index maps the file was encoded from" % (F, S, S, K))
        frames, _ = hold_ref.noisy_sprite_sequence(S, S, F, 3)

        def error(maps, pal):
            ch = ordered_ref._channels(pal)
            return sum(int(((ordered_ref._channels(f) - ch[m.reshape(-1).astype(np.int64)]) ** 2).sum()) for f, m in zip(frames, maps))

        def files(label, pal, maps, hold):
            if hold is not None:
                maps = nq.hold_frames(frames, maps, hold)[0]
            e = error(maps, np.asarray(pal))
            for lossy in (0, 16):
                say("%-34s delta GIF lossy=%-2d %10d bytes   error %d" % (label, lossy, len(nq.encode_gif_delta(maps, pal, lossy=lossy)), e))
            say("%-34s APNG              %10d bytes   error %d" % (label, len(nq.encode_apng(maps, pal)), e))

        pal, outs = nq.convert_frames(1, frames, K, True, seeds=[5] * F)
        files("error diffusion, equal seeds", pal, [o.index for o in outs], None)
        files("error diffusion, equal seeds, hold=4", pal, [o.index for o in outs], 4)
        for L in (16, 32, 64):
            pal, outs = nq.convert_frames_ordered(1, frames, K, L)
            files("ordered=%d" % L, pal, [o.index for o in outs], None)
            files("ordered=%d, hold=4" % L, pal, [o.index for o in outs], 4)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
