"""What palette refinement costs and what it buys (nq_refine_palette_device / nq_convert_frames_refined).  No oracle.

(a) Speed: ms per assignment pass over one device-resident frame, at K = 256, 64 and 16, on gradient_noise, on a flat frame (every
pixel to one entry: the same-address case) and on the tiled sample photograph, on the vector and on the scalar path -- beside two
yardsticks timed in the same run: torch's device-to-device copy of the same buffer, and one pass written in plain torch (chunked
matmul argmin + index_add_).  Every timed input is first compared with the numpy restatement (tests/refine_ref.py) on a crop.
A pass is the event span of an iterations=0 call minus the span of the same call on an 8x8 frame (table and state upload, the update
step, the read-back and the wait for it); where the passes do not stop early, (span of iterations=4 - span of iterations=0) / 4 is
printed beside it.  --convert-ms is bench.py's per-image convert time, to put a pass into proportion.

(b) Quality: for both kinds, K = 256 / 64 / 16, refine = 0 / 1 / 2 / 4 / 8, on the tiled photograph and on gradient_noise: sse[] of the
passes and the summed squared RGB error of the final out_argb with dither on and with dither off.

    python tools/refine_bench.py [--size 4096] [--quality-size 512] [--reps 20] [--convert-ms X] [--out profiles/r12/refine_bench.txt]

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
    ap.add_argument("--quality-size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--convert-ms", type=float, default=0.0)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import refine_ref

    W = H = args.size
    px = W * H
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rgb = np.load(os.path.join(ROOT, "tests", "golden", "sample_495x438.npz"))["rgb"]
    say("palette refinement on one device-resident frame of %dx%d (%.0f MB read per pass); library %s" % (
        W, H, px * 4 / 1e6, os.path.basename(nq.library_path())))
    buf = torch.zeros(px + 4, dtype=torch.int32, device="cuda")          # room to start the frame one element late (the scalar path)
    assert buf.data_ptr() % 16 == 0
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    small = torch.zeros(64, dtype=torch.int32, device="cuda")

    def fill(content, shift):
        if content == "noise":
            buf[shift:shift + px].copy_(synth.gradient_noise_torch(W, H, 11))
        elif content == "flat":
            buf[shift:shift + px].fill_(-(0x01000000 - 0x336699))          # 0xFF336699
        else:
            buf[shift:shift + px].copy_(torch.from_numpy(synth.tile_photo(rgb, W, H).reshape(-1)))
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

    # yardstick 1: the same bytes through a device-to-device copy (read + write)
    fill("noise", 0)
    dst = torch.empty_like(buf)
    copy_ms = timed(lambda: dst.view(torch.float32).copy_(buf.view(torch.float32)))
    say("device-to-device copy of the buffer (torch copy_, float32 view): %.3f ms, %.1f GB/s read" % (copy_ms, px * 4 / copy_ms / 1e6))
    del dst

    # yardstick 2: one pass in plain torch
    def torch_pass(K):
        pal = torch.from_numpy(palette(K).astype(np.int64)).cuda()
        c = torch.stack([(pal >> 24) & 255, (pal >> 16) & 255, (pal >> 8) & 255, pal & 255], 1).float()
        c2 = (c * c).sum(1)
        cnt = torch.zeros(K, dtype=torch.int64, device="cuda")
        sums = torch.zeros(K, 3, dtype=torch.int64, device="cuda")
        sse = torch.zeros((), dtype=torch.int64, device="cuda")
        ar = torch.arange(K, dtype=torch.int32, device="cuda")
        CH = 1 << 20
        for s in range(0, px, CH):
            v = buf[s:min(s + CH, px)].to(torch.int64) & 0xFFFFFFFF
            p = torch.stack([(v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255], 1)
            pf = p.float()
            d = c2[None, :] - 2.0 * (pf @ c.t())                            # exact in float32: every term is an integer below 2^24
            m = (d.to(torch.int32) * 256 + ar[None, :]).min(1).values      # (the lowest index on a tie, as the definition has it)
            k = (m & 255).to(torch.int64)
            sse += ((m >> 8) + (p * p).sum(1)).sum()
            cnt.index_add_(0, k, torch.ones_like(k))
            sums.index_add_(0, k, p[:, 1:])
        return cnt, sums, sse

    fixed = timed(lambda: nq.refine_palette_device(q, [small.data_ptr()], [8], [8], palette(16), 0))
    say("fixed cost: an iterations=0 call on one 8x8 frame: %.3f ms event span (uploads, one pass, the update step, read-back and wait)" % fixed)
    say("per pass = span(iterations=0) - fixed cost; in brackets (span(iterations=4) - span(iterations=0)) / 4 where all 5 passes ran; best of %d" % args.reps)
    res = {}
    for content in ("noise", "flat", "photo"):
        for shift in (0, 1):
            fill(content, shift)
            ptr = buf.data_ptr() + 4 * shift
            crop = buf[shift:shift + 65536].cpu().numpy().reshape(256, 256)
            for K in (256, 64, 16):
                pal = palette(K)
                got = nq.refine_palette_device(q, [ptr], [256], [256], pal, 1)
                want = refine_ref.refine([crop], pal, 1)
                assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3], (content, shift, K)
                s0 = timed(lambda: nq.refine_palette_device(q, [ptr], [W], [H], pal, 0))
                out4 = nq.refine_palette_device(q, [ptr], [W], [H], pal, 4)
                s4 = timed(lambda: nq.refine_palette_device(q, [ptr], [W], [H], pal, 4), max(args.reps // 4, 3)) if out4[3] == 5 else None
                one = s0 - fixed
                res[content, shift, K] = one
                say("%-5s %s path K=%3d: %8.3f ms per pass%s  %7.1f GB/s read  %5.2fx the copy  %6.1f Gpixel-entries/s%s" % (
                    content, "scalar" if shift else "vector", K, one, "  [%.3f]" % ((s4 - s0) / 4) if s4 else "", px * 4 / one / 1e6,
                    one / copy_ms, px * K / one / 1e6, "  %.1f %% of a convert" % (100 * one / args.convert_ms) if args.convert_ms else ""))
    for K in (256, 64, 16):
        say("flat / noise at K=%d: vector path %.3f, scalar path %.3f" % (K, res["flat", 0, K] / res["noise", 0, K], res["flat", 1, K] / res["noise", 1, K]))
    fill("noise", 0)
    for K in (256, 16):
        cnt, sums, sse = torch_pass(K)
        want = nq.refine_palette_device(q, [buf.data_ptr()], [W], [H], palette(K), 0)
        assert np.array_equal(cnt.cpu().numpy(), want[2]) and int(sse) == int(want[1][0]), "the torch pass differs"
        t = timed(lambda: torch_pass(K), 3)
        say("one pass in plain torch (chunked float32 matmul argmin + index_add_), noise, K=%d: %.2f ms, %.1fx the kernel's vector path" % (
            K, t, t / res["noise", 0, K]))
    q.close()

    if not args.skip_quality:
        S = args.quality_size
        say("")
        say("quality on 3 frames of %dx%d, MODE_PARALLEL_TILED, seeds 0: sse[] of the passes (squared ARGB error of the nearest-entry "
            "assignment), and the summed squared RGB error of out_argb against the frames" % (S, S))

        def rgb_err(frames, outs):
            e = 0
            for f, o in zip(frames, outs):
                a, b = f.view(np.uint32).astype(np.int64), o.argb.view(np.uint32).astype(np.int64)
                for sh in (16, 8, 0):
                    d = ((a >> sh) & 255) - ((b >> sh) & 255)
                    e += int((d * d).sum())
            return e

        contents = {"photo": [synth.tile_photo(rgb, S, S, slot) for slot in range(3)], "noise": [synth.gradient_noise(S, S, 20 + i) for i in range(3)]}
        for name, frames in contents.items():
            for kind in (0, 1):
                for K in (256, 64, 16):
                    base = None
                    for refine in (0, 1, 2, 4, 8):
                        pal, on = nq.convert_frames_refined(kind, frames, K, True, refine)
                        _, off = nq.convert_frames_refined(kind, frames, K, False, refine)
                        if refine == 0:
                            base = pal
                            _, sse, _, passes = nq.refine_palette(frames, base, 8)
                            say("%-5s %s K=%3d: sse[0..8] = %s (%d passes ran)" % (name, "LAB" if kind else "RGB", K, sse.tolist(), passes))
                        e_on, e_off, e_pal = rgb_err(frames, on), rgb_err(frames, off), nq.palette_error(frames, pal)
                        if refine == 0:
                            b_on, b_off, b_pal = e_on, e_off, e_pal
                        say("    refine=%d: palette error %d (%.3f)  out_argb error dither on %d (%.3f)  dither off %d (%.3f)" % (
                            refine, e_pal, e_pal / b_pal, e_on, e_on / b_on, e_off, e_off / b_off))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
