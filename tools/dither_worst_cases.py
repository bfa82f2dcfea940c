"""Times the dither pass of one 4096x4096 image (8x8 tiles, K = 256) under every NQ_OPT_DITHER_CHAIN form, on the images that are hardest
for the light walk: the headline image, `dense` (a white pixel at step 0 of every tile), `sparse` (one white pixel per wavefront, at the
last step of lane 63's tile) and `white strip` (rows 1024..1535 all white).  stage_ms()['dither'] of a stand-alone nq_dither_device call
(the kernel(s) and the hand-back pass), `reps` passes each.
Usage: python tools/dither_worst_cases.py [out.txt] [reps]"""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nquant.android_amd as nq
from nquant.android_amd import synth, host

W = H = 4096
TILE = 8
FORMS = ((1, "chain"), (2, "fused"), (3, "split"), (0, "auto"))


def images():
    base = synth.gradient_noise(W, H, 3)
    # first and last position of the generalised Hilbert curve over a square tile of even side; the
    # listed-tiles column of the output shows whether the pixels sit where they should: 262144 for `dense`, 4096 for `sparse`
    (fx, fy), (lx, ly) = (0, 0), (TILE - 1, 0)
    dense = base.copy()
    dense[fy::TILE, fx::TILE] = -1
    sparse = base.copy()
    tiles_x = W // TILE
    for t in range(63, tiles_x * (H // TILE), 64):
        ty, tx = divmod(t, tiles_x)
        sparse[ty * TILE + ly, tx * TILE + lx] = -1
    strip = base.copy()
    strip[1024:1536, :] = -1
    return (("headline", base), ("dense (white pixel at step 0 of every tile)", dense),
            ("sparse (one white pixel per wavefront, last step of lane 63)", sparse), ("white strip (rows 1024..1535 all white)", strip))


def main():
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    lines = ["Single %dx%d image, %dx%d tiles, K = 256, one handle, NQ_OPT_DITHER_CHAIN 1 (chain in every step) / 2 (fused light walk) / 3 (split: "
             "light kernel + chain pass, serial) / 0 (automatic), %d dither passes each, stage_ms()['dither'] in ms: median (min)" % (W, H, TILE, TILE, reps), ""]
    for name, img in images():
        d_in = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
        q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=1, seed=3)
        q.width, q.height = W, H
        pal = q.pnnquan_device(d_in.data_ptr(), 256)
        q.set_tile(TILE, TILE)
        d_out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        d_idx = torch.zeros(W * H, dtype=torch.int16, device="cuda")
        cells, shas, listed = [], set(), 0
        for chain, label in FORMS:
            q.set_option(host.OPT_DITHER_CHAIN, chain)
            acc = []
            for _ in range(reps + 1):
                q.dither_device(d_in.data_ptr(), pal, True, d_out.data_ptr(), d_idx.data_ptr())
                torch.cuda.synchronize()
                acc.append(q.stage_ms()["dither"])
            acc = sorted(acc[1:])
            if chain == 3:
                before = host.dither_split_stats()[2]
                q.dither_path()
                listed = host.dither_split_stats()[2] - before
            shas.add(hashlib.sha256(d_idx.cpu().numpy().tobytes()).hexdigest())
            cells.append("%s %.4f (%.4f)" % (label, acc[len(acc) // 2], acc[0]))
        lines.append("%-62s %s | same output %s | path %s | split lists %d of %d tiles | weight %.5f"
                     % (name, " | ".join(cells), len(shas) == 1, q.dither_path(), listed, (W // TILE) * (H // TILE), q.params.weight))
        q.close()
        del d_in, d_out, d_idx
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
