"""GIF encoding of 4096x4096 index maps on the GPU (nq_encode_gif_device / nq_encode_gif) against the CPU writers on the same host:
Pillow's GIF encoder and indexed_png.write_indexed_png.  The maps are what the headline bench converts (gradient_noise,
PnnLABQuantizer.convert(256, true)).  Times are wall clock around calls that return when the file is in host memory (the GPU calls
end in a stream synchronise and the copy of the file).

    python tools/gif_bench.py [--size 4096] [--batch 64] [--reps 5] [--out FILE]

--delta measures the delta mode instead (nq_encode_gif_delta_device next to nq_encode_gif_device on the same maps): --batch frames from
nq_convert_frames_device with equal seeds, once a sprite moving over a still background and once unrelated images.

    python tools/gif_bench.py --delta [--size 4096] [--batch 64] [--reps 3] [--out profiles/r07/gif_delta_bench.txt]

--lossy N (repeatable) measures the lossy mode instead (nq_encode_gif_lossy_device): one index map from convert_frames, encoded without
and with every threshold N; per call the file bytes, their ratio to the lossless file, the ms per call, and the share of pixels that
decode to another index than the source's, found by decoding each file with the decoder below.

    python tools/gif_bench.py --lossy 8 --lossy 16 --lossy 32 [--size 4096] [--reps 5] [--out profiles/r09/gif_lossy_bench.txt]

--local measures the local colour tables instead: (a) one --size map through nq_encode_gif_local_device next to nq_encode_gif_device on
the same map, lossless and at lossy 16; (b) a two-shot sequence of --shot-frames frames of --shot-size pixels a side (each shot a
gradient_noise background of its own, the second with its channels rotated so that the shots' colours differ, and a moving sprite)
through convert_shots_to_gif and through convert_frames_to_gif(delta=True) at K = 256 and 64: file bytes and the summed squared RGB error
of Pillow's canvases against the source frames.

    python tools/gif_bench.py --local [--size 4096] [--shot-size 1024] [--shot-frames 16] [--reps 5] [--out profiles/r10/gif_local_bench.txt]"""
import argparse
import io
import os
import sys
import tempfile
import time

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


def delta_bench(args, say):
    """Bytes and ms per call of the delta encoder and of the full-frame encoder on the same device-resident index maps."""
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth

    W = H = args.size
    n, K = args.batch, 255
    side = max(16, W // 16)                          # the sprite: a square of unrelated pixels, moved 3/4 of its side per frame
    say("delta-mode GIF encoding of %d frames of %dx%d (PnnLABQuantizer, convert_frames_device(%d, true), equal seeds, tiled mode); "
        "best of %d" % (n, W, H, K, args.reps))
    outs = [torch.empty(W * H, dtype=torch.int32, device="cuda") for _ in range(n)]
    idxs = [torch.empty(W * H, dtype=torch.int16, device="cuda") for _ in range(n)]

    def run(name, frames):
        q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
        t = time.perf_counter()
        pal = nq.convert_frames_device(q, [f.data_ptr() for f in frames], [W] * n, [H] * n, K, True, [o.data_ptr() for o in outs],
                                       [i.data_ptr() for i in idxs], seeds=[0] * n)
        torch.cuda.synchronize()
        say("%s: convert_frames_device %.0f ms, K = %d" % (name, (time.perf_counter() - t) * 1e3, len(pal)))
        ptrs = [i.data_ptr() for i in idxs]
        full = lambda: nq.encode_gif_device(q, ptrs, [W] * n, [H] * n, pal, [4] * n, 0)
        delta = lambda: nq.encode_gif_delta_device(q, ptrs, W, H, pal, [4] * n, 0, return_rects=True)
        full()
        delta()
        tf, gf = timed(full, args.reps)
        td, (gd, rects) = timed(delta, args.reps)
        area = int((rects[:, 2].astype(np.int64) * rects[:, 3]).sum())
        say("%s: encode_gif_device        %9.1f ms per call  %12d bytes" % (name, tf * 1e3, len(gf)))
        say("%s: encode_gif_delta_device  %9.1f ms per call  %12d bytes  (%.3fx the time, %.3fx the bytes; rectangles cover %.3f of the "
            "pixels)" % (name, td * 1e3, len(gd), td / tf, len(gd) / len(gf), area / (n * W * H)))
        q.close()

    back = synth.gradient_noise_torch(W, H, 3).reshape(H, W)
    sprite = synth.uniform_rgb(side, side, 1)
    sprite = torch.from_numpy(sprite).cuda()
    frames = []
    for i in range(n):
        f = back.clone()
        x = (i * 3 * side // 4) % (W - side)
        y = (i * side // 2) % (H - side)
        f[y:y + side, x:x + side] = sprite
        frames.append(f.reshape(-1).contiguous())
    run("moving sprite   ", frames)
    del frames, back
    frames = [synth.gradient_noise_torch(W, H, 3 + k) for k in range(n)]
    run("unrelated images", frames)


def lzw_indices(data, m, count):
    """The first `count` indices of a GIF frame's LZW data (sub-blocks already joined).  The codes between two Clear codes have
    widths that depend only on how many codes came since the Clear, so each such run is cut out of the bit string in one numpy
    gather; the strings are then put together code by code."""
    clear, eoi = 1 << m, (1 << m) + 1
    bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")
    nbits = bits.size
    run = 4096 + 64
    size = eoi + 1 + np.maximum(np.arange(run) - 1, 0)
    w = np.minimum(12, np.maximum(m + 1, np.floor(np.log2(np.minimum(size, 4096))).astype(np.int64) + 1))
    off = np.concatenate([[0], np.cumsum(w)])
    bits = np.concatenate([bits, np.zeros(12 * run + 64, np.uint8)])
    lane, weight = np.arange(12), 1 << np.arange(12)
    base = [bytes([i]) for i in range(clear)] + [None, None]
    out, have, pos = [], 0, 0
    while pos + m + 1 <= nbits and have < count:
        codes = ((bits[(pos + off[:run])[:, None] + lane] * (lane < w[:, None])) @ weight)
        stop = np.nonzero((codes == clear) | (codes == eoi) | (pos + off[1:] > nbits))[0]
        n = int(stop[0]) if stop.size else run
        if n == run:                                 # (a table that stays full for longer than the margin: not met with this encoder)
            raise ValueError("no Clear code within %d codes" % run)
        table = list(base)
        prev = None
        for code in codes[:n].tolist():
            if prev is None:
                e = table[code]
            elif code < len(table):
                e = table[code]
                if len(table) < 4096:
                    table.append(prev + e[:1])
            else:
                e = prev + prev[:1]
                table.append(e)
            out.append(e)
            have += len(e)
            prev = e
        if pos + off[n + 1] > nbits or codes[n] == eoi:
            break
        pos += int(off[n + 1])
    return np.frombuffer(b"".join(out), np.uint8)[:count]


def first_frame_indices(gif):
    """The index map (flat) of the first frame of a GIF file written by this library."""
    assert gif[:6] == b"GIF89a"
    pos = 13 + (3 << ((gif[10] & 7) + 1))
    while gif[pos] == 0x21:                          # extensions
        pos += 2
        while gif[pos]:
            pos += 1 + gif[pos]
        pos += 1
    assert gif[pos] == 0x2C
    w, h = gif[pos + 5] | gif[pos + 6] << 8, gif[pos + 7] | gif[pos + 8] << 8
    m = gif[pos + 10]
    pos += 11
    data = bytearray()
    while gif[pos]:
        data += gif[pos + 1:pos + 1 + gif[pos]]
        pos += 1 + gif[pos]
    return lzw_indices(bytes(data), m, w * h)


def lossy_bench(args, say):
    """Bytes, ms per call and substituted pixels of the lossy encoder next to the lossless call on the same device-resident index map."""
    import torch
    import nquant.android_amd as nq
    from nquant.android_amd import synth

    W = H = args.size
    say("lossy GIF encoding of one %dx%d index map (gradient_noise seed 3, PnnLABQuantizer, convert_frames(256, true)); best of %d"
        % (W, H, args.reps))
    frame = synth.gradient_noise(W, H, 3)
    nq.convert_frames(nq.NQ_KIND_LAB, [frame], 256, True)
    tc, (pal, outs) = timed(lambda: nq.convert_frames(nq.NQ_KIND_LAB, [frame], 256, True), 2)
    say("convert_frames (host frames, upload and read-back included)  %9.2f ms per call, K = %d" % (tc * 1e3, len(pal)))
    src = outs[0].index.reshape(-1)
    dev = torch.from_numpy(outs[0].index.view(np.int16).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    t0 = n0 = None
    for lossy in [0] + list(args.lossy):
        call = lambda: nq.encode_gif_device(q, [dev.data_ptr()], [W], [H], pal, lossy=lossy)
        call()
        t, gif = timed(call, args.reps)
        if lossy == 0:
            t0, n0 = t, len(gif)
        dec = first_frame_indices(gif)
        assert dec.size == src.size
        changed = int((dec != src).sum())
        assert lossy > 0 or changed == 0
        say("%-22s %9.2f ms per call (%.3fx lossless)  %10d bytes (%.4fx lossless)  %.4f of the pixels substituted" % (
            "encode_gif_device" if lossy == 0 else "  lossy = %d" % lossy, t * 1e3, t / t0, len(gif), len(gif) / n0, changed / src.size))
        if lossy > 0:
            rgb = np.stack([(pal.astype(np.int64) >> s) & 255 for s in (16, 8, 0)], -1)
            worst = int(np.abs(rgb[dec] - rgb[src]).max())
            say("%-22s largest channel error of a decoded pixel: %d" % ("", worst))
            assert worst <= lossy
    q.close()


def local_bench(args, say):
    """(a) ms per call of the local-table encoder next to the global-table one on one device-resident map; (b) bytes and squared error
    of one palette per shot against one shared palette."""
    import torch
    from PIL import Image
    import nquant.android_amd as nq
    from nquant.android_amd import synth

    W = H = args.size
    say("(a) one %dx%d index map (gradient_noise seed 3, PnnLABQuantizer.convert(256, true)), device-resident; best of %d" % (W, H, args.reps))
    q0 = nq.PnnLABQuantizer(synth.gradient_noise(W, H, 3))
    o = q0.convert(256, True)
    q0.close()
    pal = o.palette
    dev = torch.from_numpy(o.index.view(np.int16).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))
    for lossy in (0, 16):
        glob = lambda: nq.encode_gif_device(q, [dev.data_ptr()], [W], [H], pal, lossy=lossy)
        loc = lambda: nq.encode_gif_local_device(q, [dev.data_ptr()], [W], [H], [pal], lossy=lossy)
        glob()
        loc()
        tg, gg = timed(glob, args.reps)
        tl, gl = timed(loc, args.reps)
        tg2, _ = timed(glob, args.reps)              # the global call again: what two runs of the same call differ by
        say("lossy %2d: encode_gif_device       %8.2f ms per call (again: %.2f)  %10d bytes" % (lossy, tg * 1e3, tg2 * 1e3, len(gg)))
        say("lossy %2d: encode_gif_local_device %8.2f ms per call (%.3fx)        %10d bytes" % (lossy, tl * 1e3, tl / min(tg, tg2), len(gl)))
        a, b = Image.open(io.BytesIO(gg)), Image.open(io.BytesIO(gl))
        assert (np.array(a.convert("RGB")) == np.array(b.convert("RGB"))).all()
    say("check: Pillow decodes both files of either threshold to the same picture")
    q.close()
    del dev

    S, n = args.shot_size, args.shot_frames
    half = n // 2
    say("(b) %d frames of %dx%d, a cut after frame %d; PnnLABQuantizer, dither, equal seeds, delta mode, host frames" % (n, S, S, half - 1))
    side = max(16, S // 16)
    sprite = synth.uniform_rgb(side, side, 1)
    backs = [synth.gradient_noise(S, S, 3), synth.gradient_noise(S, S, 4)]
    v = backs[1].view(np.uint32)                     # second shot: R <- G <- B <- R
    backs[1] = (0xFF000000 | (v & 0xFFFF) << 8 | (v >> 16) & 0xFF).astype(np.uint32).view(np.int32)
    frames = []
    for i in range(n):
        f = backs[i >= half].copy()
        x, y = (i * 3 * side // 4) % (S - side), (i * side // 2) % (S - side)
        f[y:y + side, x:x + side] = sprite
        frames.append(f)
    src = [np.stack([(f.view(np.uint32) >> s) & 255 for s in (16, 8, 0)], -1).astype(np.int64) for f in frames]

    def sse(gif):
        im = Image.open(io.BytesIO(gif))
        total = 0
        for i in range(im.n_frames):
            im.seek(i)
            total += int(((np.array(im.convert("RGB")).astype(np.int64) - src[i]) ** 2).sum())
        return total

    for K in (256, 64):
        shots, pals = nq.convert_shots_to_gif(nq.NQ_KIND_LAB, frames, [0, half], K, True, seeds=[0] * n)
        one, p1 = nq.convert_frames_to_gif(nq.NQ_KIND_LAB, frames, K, True, seeds=[0] * n, delta=True)
        es, e1 = sse(shots), sse(one)
        say("K = %3d: one palette per shot (K %s)  %10d bytes  squared error %d" % (K, [len(p) for p in pals], len(shots), es))
        say("K = %3d: one shared palette (K %d)    %10d bytes  squared error %d  (per shot / shared: %.3fx the bytes, %.3fx the error)"
            % (K, len(p1), len(one), e1, len(shots) / len(one), es / e1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4, help="distinct converted maps the batch cycles through")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=4, help="frames of the Pillow animation timed on the CPU")
    ap.add_argument("--out", default=None)
    ap.add_argument("--delta", action="store_true", help="measure the delta mode against the full-frame call instead")
    ap.add_argument("--lossy", type=int, action="append", default=[], metavar="N",
                    help="measure the lossy mode at threshold N (1..255; repeatable) against the lossless call instead")
    ap.add_argument("--local", action="store_true", help="measure the local colour tables against the global-table calls instead")
    ap.add_argument("--shot-size", type=int, default=1024, help="--local: side of the two-shot sequence's frames")
    ap.add_argument("--shot-frames", type=int, default=16, help="--local: frames of the two-shot sequence")
    args = ap.parse_args()
    if args.delta or args.lossy or args.local:
        lines = []

        def say(s):
            print(s, flush=True)
            lines.append(s)
        (local_bench if args.local else lossy_bench if args.lossy else delta_bench)(args, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    import torch
    from PIL import Image
    import nquant.android_amd as nq
    from nquant.android_amd import synth
    from nquant.android_amd.indexed_png import write_indexed_png

    W = H = args.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("GIF encoding of %dx%d index maps (gradient_noise seeds 3.., PnnLABQuantizer.convert(256, true)); best of %d" % (W, H, args.reps))
    maps, pals = [], []
    for k in range(args.distinct):
        q = nq.PnnLABQuantizer(synth.gradient_noise(W, H, 3 + k))
        o = q.convert(256, True)
        q.close()
        maps.append(o.index)
        pals.append(o.palette)
    pal = pals[0]
    dev = [torch.from_numpy(m.view(np.int16).reshape(-1).copy()).cuda() for m in maps]
    torch.cuda.synchronize()
    q = nq.PnnQuantizer(np.zeros((1, 1), np.int32))

    # GPU, one frame
    one = lambda: nq.encode_gif_device(q, [dev[0].data_ptr()], [W], [H], pal)
    one()
    t1, gif1 = timed(one, args.reps)
    say("gpu  encode_gif_device, 1 frame          %9.2f ms/frame  %8.0f Mpx/s  %d bytes" % (t1 * 1e3, W * H / t1 / 1e6, len(gif1)))
    th, gifh = timed(lambda: nq.encode_gif(maps[0], pal), args.reps)
    assert gifh == gif1
    say("gpu  encode_gif (host maps), 1 frame     %9.2f ms/frame  %8.0f Mpx/s" % (th * 1e3, W * H / th / 1e6))
    # GPU, a batch of frames in one call (one animation)
    B = args.batch
    ptrs = [dev[i % len(dev)].data_ptr() for i in range(B)]
    batch = lambda: nq.encode_gif_device(q, ptrs, [W] * B, [H] * B, pal, [4] * B, 0)
    batch()
    tb, gifb = timed(batch, max(2, args.reps // 2))
    say("gpu  encode_gif_device, %d frames        %9.2f ms/frame  %8.0f Mpx/s  %d bytes (%.1f ms per call)" % (
        B, tb / B * 1e3, B * W * H / tb / 1e6, len(gifb), tb * 1e3))
    # CPU writers
    im = Image.fromarray(maps[0].astype(np.uint8), "P")
    im.putpalette([v for c in pal for v in ((int(c) >> 16) & 255, (int(c) >> 8) & 255, int(c) & 255)])

    def pillow_one():
        b = io.BytesIO()
        im.save(b, "GIF")
        return b.getvalue()
    tp, pgif = timed(pillow_one, 2)
    say("cpu  Pillow GIF, 1 frame                 %9.2f ms/frame  %8.1f Mpx/s  %d bytes" % (tp * 1e3, W * H / tp / 1e6, len(pgif)))
    F = args.cpu_frames
    ims = []
    for i in range(F):
        x = Image.fromarray(maps[i % len(maps)].astype(np.uint8), "P")
        x.putpalette(im.getpalette())
        ims.append(x)

    def pillow_anim():
        b = io.BytesIO()
        ims[0].save(b, "GIF", save_all=True, append_images=ims[1:], duration=40, loop=0, optimize=False)
        return b.getvalue()
    ta, _ = timed(pillow_anim, 1)
    say("cpu  Pillow GIF, %d-frame animation       %9.2f ms/frame  %8.1f Mpx/s" % (F, ta / F * 1e3, F * W * H / ta / 1e6))
    with tempfile.TemporaryDirectory() as d:
        tn, nbytes = timed(lambda: write_indexed_png(os.path.join(d, "x.png"), maps[0], pal), 2)
    say("cpu  write_indexed_png, 1 frame          %9.2f ms/frame  %8.1f Mpx/s  %d bytes" % (tn * 1e3, W * H / tn / 1e6, nbytes))
    say("speed-up vs Pillow: %.0fx (1 frame), %.0fx (batch of %d vs the Pillow animation); size vs Pillow: %.4fx" % (
        tp / t1, (ta / F) / (tb / B), B, len(gif1) / len(pgif)))
    # the GPU file decodes to the map
    dec = Image.open(io.BytesIO(gif1))
    dec.load()
    assert (np.array(dec) == maps[0]).all()
    say("check: Pillow decodes the GPU file to the index map exactly")
    q.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
