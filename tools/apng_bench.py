"""APNG encoding of index-map sequences on the GPU (nq_encode_apng_device) against one n-image nq_encode_png_device call on the same
frames: wall clock until the file(s) are in host memory, best of --reps, and the byte ratio of the two.  Two sequences in index space
(K = 255, an opaque palette, so mark mode; --crop: K = 256, crop mode): a sprite that moves over a static background, and noise that
changes everywhere.  The still-image call on one frame of the first sequence is timed as well (the figure to compare between two
builds).  Every APNG is read back with Pillow when it is installed and compared with the frames.

    python tools/apng_bench.py [--size 1024] [--frames 16] [--sprite 128] [--reps 5] [--crop] [--out FILE]"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times), sorted(times)[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--sprite", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--crop", action="store_true", help="K = 256: no room for the unchanged index, frames are cropped only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq

    W = H = args.size
    n, sp = args.frames, args.sprite
    K = 256 if args.crop else 255
    pal = 0xFF000000 | (np.arange(K, dtype=np.int64) * 0x010203 & 0xFFFFFF)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("APNG encoding of %d frames of %dx%d, K = %d (%s mode); best / median of %d" % (n, W, H, K, "crop" if args.crop else "mark", args.reps))
    rng = np.random.default_rng(1)
    # a smooth background with a little noise (compressible, like a dithered picture), a noise sprite moving along the diagonal
    yy, xx = np.mgrid[0:H, 0:W]
    back = ((xx * 3 + yy * 5) // 16 + rng.integers(0, 3, (H, W))) % K
    sprite = rng.integers(0, K, (sp, sp))
    moving = []
    for i in range(n):
        f = back.copy()
        o = (W - sp) * i // max(n - 1, 1)
        f[o:o + sp, o:o + sp] = sprite
        moving.append(f.astype(np.uint16))
    noise = [rng.integers(0, K, (H, W)).astype(np.uint16) for _ in range(n)]
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    for name, frames in (("moving %d^2 sprite" % sp, moving), ("noise, changes everywhere", noise)):
        dev = [torch.from_numpy(f.view(np.int16).reshape(-1).copy()).cuda() for f in frames]
        torch.cuda.synchronize()
        ptrs = [d.data_ptr() for d in dev]
        one = lambda: nq.encode_png_device(q, ptrs[:1], [W], [H], [pal])[0]
        stills = lambda: nq.encode_png_device(q, ptrs, [W] * n, [H] * n, [pal] * n)
        anim = lambda: nq.encode_apng_device(q, ptrs, W, H, pal, [4] * n, 0, return_rects=True)
        one(); stills(); anim()
        t1, m1, png = timed(one, args.reps)
        ts, ms, files = timed(stills, args.reps)
        ta, ma, (data, rects) = timed(anim, args.reps)
        nb = sum(len(f) for f in files)
        area = sum(int(r[2]) * int(r[3]) for r in rects) / float(n * W * H)
        say("%s:" % name)
        say("  encode_png_device, 1 image       %8.3f / %8.3f ms  %9d bytes" % (t1 * 1e3, m1 * 1e3, len(png)))
        say("  encode_png_device, %2d images     %8.3f / %8.3f ms  %9d bytes" % (n, ts * 1e3, ms * 1e3, nb))
        say("  encode_apng_device, %2d frames    %8.3f / %8.3f ms  %9d bytes   rectangles cover %.3f of the pixels" % (n, ta * 1e3, ma * 1e3, len(data), area))
        say("  APNG / %d stills: time %.3f, bytes %.3f" % (n, ta / ts, len(data) / nb))
        try:
            from PIL import Image
            im = Image.open(io.BytesIO(data))
            assert im.n_frames == n
            for i in (0, n // 2, n - 1):
                im.seek(i)
                rgb = np.array(im.convert("RGB"))
                c = pal[frames[i]]
                assert (rgb == np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1)).all(), i
            say("  Pillow composes frames 0, %d and %d back to the index maps' colours" % (n // 2, n - 1))
        except ImportError:
            say("  Pillow is not installed: the file was not read back")
        del dev
    q.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
