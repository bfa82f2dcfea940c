"""PNG encoding of 4096x4096 index maps on the GPU (nq_encode_png_device / nq_encode_png) against the CPU writers on the same host --
zlib level 1 and level 6 over the same raw stream, indexed_png.write_indexed_png -- and against encode_gif_device on the same map.
The maps are what the headline bench converts (gradient_noise, PnnLABQuantizer.convert(256, true)).  Wall clock until the files are
in host memory, best of --reps.  Every GPU file is inflated with zlib (and opened with Pillow when it is installed) and compared with
the map.

    python tools/png_bench.py [--size 4096] [--batch 64] [--reps 5] [--out FILE]"""
import argparse
import io
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    best, out = None, None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best, out


def idat_of(png):
    """The IDAT chunk's data (every chunk CRC checked)."""
    pos, idat = 8, None
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        body = png[pos + 4:pos + 8 + n]
        assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(body), body[:4]
        if body[:4] == b"IDAT":
            idat = body[4:]
        pos += 12 + n
    return idat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4, help="distinct converted maps the batch cycles through")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    from nquant.android_amd.indexed_png import write_indexed_png

    W = H = args.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("PNG encoding of %dx%d index maps (gradient_noise seeds 3.., PnnLABQuantizer.convert(256, true)); best of %d" % (W, H, args.reps))
    maps, pals = [], []
    for k in range(args.distinct):
        q = nq.PnnLABQuantizer(synth.gradient_noise(W, H, 3 + k))
        o = q.convert(256, True)
        q.close()
        maps.append(o.index)
        pals.append(o.palette)
    dev = [torch.from_numpy(m.view(np.int16).reshape(-1).copy()).cuda() for m in maps]
    torch.cuda.synchronize()
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    Mpx = W * H / 1e6

    def check(png, m):
        raw = zlib.decompress(idat_of(png))
        rows = np.frombuffer(raw, np.uint8).reshape(H, -1)
        assert len(pals[0]) > 16 and (rows[:, 0] == 0).all() and (rows[:, 1:] == m).all()
        return raw

    one = lambda: nq.encode_png_device(q, [dev[0].data_ptr()], [W], [H], [pals[0]])[0]
    one()
    t1, png1 = timed(one, args.reps)
    raw = check(png1, maps[0])
    say("gpu  encode_png_device, 1 image          %9.2f ms/image  %8.0f Mpx/s  %d bytes" % (t1 * 1e3, Mpx / t1, len(png1)))
    th, pngh = timed(lambda: nq.encode_png(maps[0], pals[0]), args.reps)
    assert pngh == png1
    say("gpu  encode_png (host maps), 1 image     %9.2f ms/image  %8.0f Mpx/s" % (th * 1e3, Mpx / th))
    for S in (8192, 65535):
        ts, pngs = timed(lambda: nq.encode_png_device(q, [dev[0].data_ptr()], [W], [H], [pals[0]], S)[0], args.reps)
        check(pngs, maps[0])
        say("gpu  encode_png_device, segment %5d    %9.2f ms/image  %8.0f Mpx/s  %d bytes" % (S, ts * 1e3, Mpx / ts, len(pngs)))
    B = args.batch
    ptrs = [dev[i % len(dev)].data_ptr() for i in range(B)]
    bp = [pals[i % len(dev)] for i in range(B)]
    batch = lambda: nq.encode_png_device(q, ptrs, [W] * B, [H] * B, bp)
    batch()
    tb, files = timed(batch, max(2, args.reps // 2))
    for i in range(len(dev)):
        check(files[i], maps[i])
    assert files[0] == png1
    say("gpu  encode_png_device, %d images        %9.2f ms/image  %8.0f Mpx/s  %d bytes (%.1f ms per call)" % (
        B, tb / B * 1e3, B * Mpx / tb, sum(len(f) for f in files), tb * 1e3))
    tg, gif = timed(lambda: nq.encode_gif_device(q, [dev[0].data_ptr()], [W], [H], pals[0]), args.reps)
    say("gpu  encode_gif_device, 1 frame          %9.2f ms/frame  %8.0f Mpx/s  %d bytes" % (tg * 1e3, Mpx / tg, len(gif)))
    # CPU writers on the same host
    for level in (1, 6):
        tz, z = timed(lambda: zlib.compress(raw, level), 2)
        say("cpu  zlib level %d over the raw stream    %9.2f ms/image  %8.1f Mpx/s  %d bytes" % (level, tz * 1e3, Mpx / tz, len(z)))
        if level == 1:
            t_l1, n_l1 = tz, len(z)
        else:
            n_l6 = len(z)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "a.png")
        tw, _ = timed(lambda: write_indexed_png(path, maps[0], pals[0]), 2)
        say("cpu  write_indexed_png                   %9.2f ms/image  %8.1f Mpx/s  %d bytes" % (tw * 1e3, Mpx / tw, os.path.getsize(path)))
    n_idat = len(idat_of(png1))
    say("IDAT %d bytes = %.4f x zlib level 1, %.4f x zlib level 6, %.4f x the GIF; %.2f bits per pixel" % (
        n_idat, n_idat / n_l1, n_idat / n_l6, len(png1) / len(gif), 8.0 * len(png1) / (W * H)))
    say("speed-up, 1 image: %.0fx zlib level 1, %.0fx write_indexed_png; batch of %d: %.0fx zlib level 1; PNG / GIF time %.2f" % (
        t_l1 / t1, tw / t1, B, t_l1 / (tb / B), t1 / tg))
    try:
        from PIL import Image
        Image.MAX_IMAGE_PIXELS = None
        im = Image.open(io.BytesIO(png1))
        im.load()
        assert im.mode == "P" and (np.array(im) == maps[0]).all()
        say("Pillow opens the GPU file as mode P with the same indices")
    except ImportError:
        say("Pillow is not installed: the zlib check alone was run")
    q.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
