"""Lossless WebP encoding on the GPU (nq_encode_webp_device) against the project's other encoders on the same index maps, and against
libwebp's own lossless encoder (Pillow) on the same pictures: file sizes, and wall clock per call until the file is in host memory
(best / median of --reps) next to nq_encode_png_device in the same run.  Two inputs:
  * a dithered 256-colour map of --size^2 (the sample photo tiled, PnnLABQuantizer.convert(256, true));
  * the noisy clip of tools/hold_bench.py: --frames frames of --clip^2, a still background with +-2 of noise per channel and frame and
    a small moving sprite, convert_frames_device(256, true) with equal seeds in tiled mode and the temporal hold at threshold 4.
Every WebP file is read back by libwebp (Pillow) and compared with palette[index].  Records, not thresholds.

    python tools/webp_bench.py [--size 4096] [--clip 1024] [--frames 16] [--reps 5] [--out profiles/r18/webp_bench.txt]"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times), sorted(times)[len(times) // 2], out


def rgba_of(index, pal):
    p = np.asarray(pal).astype(np.int64).astype(np.uint32)[np.asarray(index)]
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255, p >> 24], -1).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--clip", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    import hold_ref
    try:
        from PIL import Image, features
        pillow = features.check("webp")
    except ImportError:
        pillow = False
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def libwebp_reads(data, maps, pal, which):
        if not pillow:
            return "Pillow has no WebP: the file was not read back"
        im = Image.open(io.BytesIO(data))
        assert getattr(im, "n_frames", 1) == len(maps)
        for i in which:
            im.seek(i)
            assert (np.asarray(im.convert("RGBA")) == rgba_of(maps[i], pal)).all(), i
        return "libwebp composes frame(s) %s back to palette[index]" % ", ".join(str(i) for i in which)

    # ---- a still picture ----
    S = args.size
    rgb = np.load(os.path.join(ROOT, "tests", "golden", "sample_495x438.npz"))["rgb"]
    img = synth.tile_photo(rgb, S, S)
    q = nq.PnnLABQuantizer(img)
    out = q.convert(256, True)
    pal = out.palette
    index = np.ascontiguousarray(out.index, np.uint16)
    say("still picture: the sample photo tiled to %dx%d, PnnLABQuantizer.convert(256, true): %d colours; best / median of %d calls" % (
        S, S, len(pal), args.reps))
    dev = torch.from_numpy(index.view(np.int16).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    png_call = lambda: nq.encode_png_device(q, [dev.data_ptr()], [S], [S], [pal])[0]
    webp_call = lambda: nq.encode_webp_device([dev.data_ptr()], S, S, pal)
    png_call(); webp_call()
    tp, mp, png = timed(png_call, args.reps)
    tw, mw, webp = timed(webp_call, args.reps)
    say("  nq_encode_png_device    %9.3f / %9.3f ms  %10d bytes" % (tp * 1e3, mp * 1e3, len(png)))
    rows = 1 << max(p for p in range(2, 10) if S << p <= 32768)
    say("  nq_encode_webp_device   %9.3f / %9.3f ms  %10d bytes   (bands of %d packed rows: %d chains)" % (
        tw * 1e3, mw * 1e3, len(webp), rows, -(-S // rows)))
    say("  WebP / PNG: time %.3f, bytes %.3f" % (tw / tp, len(webp) / len(png)))
    if pillow:
        t = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(rgba_of(index, pal), "RGBA").save(buf, format="WEBP", lossless=True)
        say("  libwebp lossless (Pillow, CPU, default effort) %9.1f ms  %10d bytes; ours / libwebp's bytes %.3f" % (
            (time.perf_counter() - t) * 1e3, buf.tell(), len(webp) / buf.tell()))
    say("  " + libwebp_reads(webp, [index], pal, [0]))
    q.close()
    del dev

    # ---- a clip ----
    W = H = args.clip
    n, px = args.frames, args.clip * args.clip
    frames, _ = hold_ref.noisy_sprite_sequence(H, W, n, 3)
    src = [torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).cuda() for f in frames]
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(n)]
    idxs = [torch.zeros(px, dtype=torch.int16, device="cuda") for _ in range(n)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
    pal = nq.convert_frames_device(q, ptr(src), [W] * n, [H] * n, 256, True, ptr(outs), ptr(idxs), seeds=[0] * n)
    nq.hold_frames_device(q, ptr(src), ptr(idxs), W, H, 4, ptr(outs), counts=False)
    torch.cuda.synchronize()
    maps = [t.cpu().numpy().view(np.uint16).reshape(H, W) for t in idxs]
    say("clip: %d frames of %dx%d, noisy_sprite_sequence, convert_frames_device(256, true), equal seeds, tiled mode, hold 4: %d colours" % (
        n, W, H, len(pal)))
    delays = [4] * n
    calls = (("nq_encode_png_device, %d stills" % n, lambda: b"".join(nq.encode_png_device(q, ptr(idxs), [W] * n, [H] * n, [pal] * n))),
             ("nq_encode_gif_delta_device", lambda: nq.encode_gif_delta_device(q, ptr(idxs), W, H, pal, delays, 0)),
             ("nq_encode_apng_device", lambda: nq.encode_apng_device(q, ptr(idxs), W, H, pal, delays, 0)),
             ("nq_encode_webp_device, delta = 0", lambda: nq.encode_webp_device(ptr(idxs), W, H, pal, delays, 0, delta=False)),
             ("nq_encode_webp_device, delta = 1", lambda: nq.encode_webp_device(ptr(idxs), W, H, pal, delays, 0)))
    size = {}
    for name, fn in calls:
        try:
            fn()
            t, m, data = timed(fn, args.reps)
        except nq.NqError as e:
            say("  %-36s refused: %s" % (name, e))
            continue
        size[name] = len(data)
        say("  %-36s %9.3f / %9.3f ms  %10d bytes" % (name, t * 1e3, m * 1e3, len(data)))
    data, rects = nq.encode_webp_device(ptr(idxs), W, H, pal, delays, 0, return_rects=True)
    area = int((rects[1:, 2].astype(np.int64) * rects[1:, 3]).sum())
    say("  the WebP rectangles of frames 1.. cover %.4f of their pixels" % (area / float((n - 1) * px)))
    ours = size["nq_encode_webp_device, delta = 1"]
    for name in ("nq_encode_png_device, %d stills" % n, "nq_encode_gif_delta_device", "nq_encode_apng_device"):
        if name in size:
            say("  WebP (delta) / %s: bytes %.3f" % (name, ours / size[name]))
    if pillow:
        t = time.perf_counter()
        buf = io.BytesIO()
        ims = [Image.fromarray(rgba_of(m, pal), "RGBA") for m in maps]
        ims[0].save(buf, format="WEBP", save_all=True, append_images=ims[1:], lossless=True, duration=40, loop=0)
        say("  libwebp lossless animation (Pillow, CPU, default effort) %9.1f ms  %10d bytes; ours / libwebp's bytes %.3f" % (
            (time.perf_counter() - t) * 1e3, buf.tell(), ours / buf.tell()))
    say("  " + libwebp_reads(data, maps, pal, [0, n // 2, n - 1]))
    q.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
