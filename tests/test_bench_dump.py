"""bench.py --dump-outputs without a GPU: dump_outputs() on host tensors, in a child process (importing bench.py sets the process's
HIP queue count).  The files must hold exactly the sampled outputs, be float64, stay under 64 MB and come out the same for the same outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import bench
n, side = int(sys.argv[3]), int(sys.argv[4])
g = torch.Generator().manual_seed(7)
outs = [torch.randint(-2 ** 31, 2 ** 31 - 1, (side * side,), dtype=torch.int32, generator=g) for _ in range(n)]
idxs = [torch.randint(-2 ** 15, 2 ** 15 - 1, (side * side,), dtype=torch.int16, generator=g) for _ in range(n)]
pals = [np.random.default_rng(k).integers(-2 ** 31, 2 ** 31 - 1, 256 - k % 3, dtype=np.int64).astype(np.int32) for k in range(n)]
for d in sys.argv[2].split(","):
    bench.dump_outputs(d, pals, outs, idxs)
np.savez(sys.argv[2].split(",")[0] + "/../inputs.npz", outs=torch.stack(outs).numpy(), idxs=torch.stack(idxs).numpy(),
         pals=np.array([np.pad(p, (0, 256 - len(p)), constant_values=0) for p in pals]), sizes=np.array([len(p) for p in pals]))
"""


@pytest.mark.parametrize("n,side", [(20, 64), (3, 2048)])
def test_dump_outputs_files(tmp_path, n, side):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    subprocess.run([sys.executable, "-c", CHILD, ROOT, ",".join(dirs), str(n), str(side)], check=True, timeout=300)
    src = np.load(tmp_path / "inputs.npz")
    names = ["argb", "index", "palette", "palette_images", "palette_size", "sample_images", "sample_pixels"]
    assert sorted(f[:-4] for f in os.listdir(dirs[0])) == names
    got = {k: np.load(os.path.join(dirs[0], k + ".npy")) for k in names}
    for k in names:
        assert got[k].dtype == np.float64
        assert (np.load(os.path.join(dirs[1], k + ".npy")) == got[k]).all(), k
    assert sum(os.path.getsize(os.path.join(dirs[0], k + ".npy")) for k in names) < 64 << 20
    imgs, pos = got["sample_images"].astype(np.int64), got["sample_pixels"].astype(np.int64)
    assert len(imgs) == min(n, 8) and len(set(imgs)) == len(imgs)
    if side * side * len(imgs) <= 1 << 21:
        assert (pos == np.arange(side * side)).all()
    else:
        assert len(pos) == (1 << 21) // len(imgs) and (np.diff(pos) > 0).all()
    for j, i in enumerate(imgs):
        assert (got["argb"][j] == (src["outs"][i][pos].astype(np.int64) & 0xFFFFFFFF)).all()
        assert (got["index"][j] == (src["idxs"][i][pos].astype(np.int64) & 0xFFFF)).all()
    assert (got["palette_images"] == np.arange(n)).all() and (got["palette_size"] == src["sizes"]).all()
    for i in range(n):
        K = src["sizes"][i]
        assert (got["palette"][i, :K] == (src["pals"][i, :K].astype(np.int64) & 0xFFFFFFFF)).all()
        assert (got["palette"][i, K:] == -1).all()
