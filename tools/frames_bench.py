"""One palette for a sequence of frames (nq_convert_frames_device): stage times against the same stages of nq_pnnquan_device on a
concatenated copy (which must give the identical palette -- asserted), per-frame dither time against separate nq_dither_device calls,
the dither path per frame, and nq_convert_batch_device (one palette per frame) on the same frames.

Workloads: (a) 64 x 1920x1080 gradient-noise frames panning across one larger image (frame t = window offset by 8t px), LAB 256 + dither;
(b) 256 x 480x270 of the same kind (GIF-sized); (c) 64 crops panning across the reference's sample photograph tiled to 1080p.

  python tools/frames_bench.py [--workloads abc] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nquant.android_amd as nq                      # noqa: E402
from nquant.android_amd import synth                 # noqa: E402


def panning_gradient(n, W, H, seed):
    big = synth.gradient_noise_torch(W + 8 * (n - 1), H, seed).reshape(H, -1)
    return [big[:, 8 * t:8 * t + W].contiguous() for t in range(n)]


def panning_photo(n, W, H):
    import torch
    rgb = np.load(os.path.join(ROOT, "tests", "golden", "sample_495x438.npz"))["rgb"]
    big = torch.from_numpy(synth.tile_photo(rgb, W + 8 * (n - 1), H)).cuda()
    return [big[:, 8 * t:8 * t + W].contiguous() for t in range(n)]


def fmt(d, keys=("prescan", "histogram", "nn_init", "merge", "palette_fill", "dither", "bluenoise", "total")):
    return " ".join("%s %.3f" % (k, d[k]) for k in keys)


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def run(name, frames, K, dither, reps):
    import torch
    n = len(frames)
    H, W = frames[0].shape
    print("== workload %s: %d frames of %dx%d, LAB %d, dither %s" % (name, n, W, H, K, dither))
    ptrs = [f.data_ptr() for f in frames]
    outs = [torch.empty(W * H, dtype=torch.int32, device="cuda") for _ in range(n)]
    idxs = [torch.empty(W * H, dtype=torch.int16, device="cuda") for _ in range(n)]
    seeds = list(range(1, n + 1))

    # the frames call
    q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
    stages, walls = [], []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pal = nq.convert_frames_device(q, ptrs, [W] * n, [H] * n, K, dither, [o.data_ptr() for o in outs], [i.data_ptr() for i in idxs], seeds=seeds)
        torch.cuda.synchronize()
        if r:
            walls.append(1e3 * (time.perf_counter() - t0))
            stages.append(q.stage_ms())
    sf = {k: median([s[k] for s in stages]) for k in stages[0]}
    params = q.params
    print("frames call    : wall %.2f ms | %s" % (median(walls), fmt(sf)))
    print("  bins %d, merge %.2f ms = %.0f %% of the call" % (params.maxbins, sf["merge"], 100.0 * sf["merge"] / max(median(walls), 1e-9)))

    # nq_pnnquan_device on a concatenated copy: its stage times come from nq_convert_device (the same pnnquan_device in front of the
    # dither pass) on the copy laid out as k frames side by side -- the pixel sequence is the concatenation either way
    concat = torch.cat([f.reshape(-1) for f in frames])
    k = next(k for k in range(1, n + 1) if n % k == 0 and H * (n // k) <= 65535 and W * k <= 65535)
    CW, CH = W * k, H * (n // k)
    qc = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
    qc.width, qc.height = CW, CH
    cout = torch.empty(CW * CH, dtype=torch.int32, device="cuda")
    cst = []
    for r in range(reps + 1):
        want = qc.convert_device(concat.data_ptr(), K, dither, cout.data_ptr())
        torch.cuda.synchronize()
        if r:
            cst.append(qc.stage_ms())
    assert len(want) == len(pal) and (want == pal).all(), "the frames palette differs from pnnquan of the concatenated copy"
    sc = {k: median([s[k] for s in cst]) for k in cst[0]}
    print("concat pnnquan : %s (nq_convert_device on the copy as %dx%d)" % (fmt(sc, ("prescan", "histogram", "nn_init", "merge")), CW, CH))
    a, b = sf["prescan"] + sf["histogram"], sc["prescan"] + sc["histogram"]
    print("  prescan+histogram: frames %.3f ms, concatenated %.3f ms, ratio %.3f (target <= 1.1); palettes identical" % (a, b, a / b))
    del concat, cout

    # separate nq_dither_device calls with the same palette and params
    qd = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))
    qd.set_params(params)
    qd.width, qd.height = W, H
    sep, paths = [], []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(n):
            qd.dither_device(ptrs[i], pal, dither, outs[i].data_ptr(), idxs[i].data_ptr(), seed=seeds[i])
            if r == 0:
                paths.append(qd.dither_path())
        e1.record()
        torch.cuda.synchronize()
        if r:
            sep.append(e0.elapsed_time(e1))
    print("dither per frame: frames call %.4f ms, separate nq_dither_device %.4f ms (incl. list build each)" % (sf["dither"] / n, median(sep) / n))
    print("  dither path per frame (specialised kernel, tiles handed back): %s" % (
        "all (%d, %d)" % paths[0] if len(set(paths)) == 1 else " ".join("(%d,%d)" % p for p in paths)))

    # nq_convert_batch_device: one palette per frame
    qs = [nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), seed=seeds[i]) for i in range(n)]
    for qq in qs:
        qq.width, qq.height = W, H
    bw = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nq.convert_batch_device(qs, ptrs, K, dither, [o.data_ptr() for o in outs], [i.data_ptr() for i in idxs])
        torch.cuda.synchronize()
        if r:
            bw.append(1e3 * (time.perf_counter() - t0))
    bins = [qq.params.maxbins for qq in qs]
    print("convert_batch  : wall %.2f ms (one palette per frame; bins per frame %d..%d)  vs frames call %.2f ms" % (
        median(bw), min(bins), max(bins), median(walls)))
    for qq in qs:
        qq.close()
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="abc")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    nq.load_library()
    if "a" in args.workloads:
        run("a", panning_gradient(64, 1920, 1080, 5), 256, True, args.reps)
    if "b" in args.workloads:
        run("b", panning_gradient(256, 480, 270, 6), 256, True, args.reps)
    if "c" in args.workloads:
        run("c", panning_photo(64, 1920, 1080), 256, True, args.reps)


if __name__ == "__main__":
    main()
