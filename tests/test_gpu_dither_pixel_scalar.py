"""The pixel-form light pass (gilbert_pixel_kernel, NQ_OPT_DITHER_CHAIN = 4) where it takes its per-tile values from the scalar unit and its
palette Lab from the table the list builders leave behind the packed records (csrc/nq_dither_fast.hip, nq_dither.inc).

At 8x8 tiles a wavefront iteration is one tile: tile number, row / column, shape, origin and the 64-bit tile seed are computed once per
wavefront from a wave index taken through readfirstlane.  A wrong scalar tile shows as a wrong origin (pixels of another tile), a wrong shape
(a partial tile walked with the full path) or a wrong seed (other draws), so every case compares option 4 with the oracle's tiled dither bit
for bit, indices and ARGB, and its listed / handed-back counts with option 3 (gilbert_light_kernel, one lane per tile).

The Lab table is written once per list build by build_lab_lists_kernel with the same RGB2LAB the kernel used to run in every workgroup; it
must belong to the palette of the pass that reads it: the next palette on the same handle, a palette of fewer than 256 entries (zero from
entry K on), and the scratch sets a batch rotates through.

The nearest-colour fallback queue of the issue (part C) is not built (the lane count), so it has no cases here."""
import numpy as np
import pytest

from nquant.android_amd import synth

import test_gpu_dither_pixel as pixel
from test_gpu_dither_pixel import WEIGHT, WHITE_44, WHITE_88, _run, _tiles_with_white
from test_gpu_dither_split import OPT_CHAIN, TILED, _cap250, _copy_params, _counters, _oracle_dither, _plant, _split_stats_of

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _want(oracle, key, img, K, tile, seed=4321):
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_dither(oracle, img, K, tile, WEIGHT, seed)
    return _ORACLE[key]


def _both(nq, img, pal, op, tile, want_argb, want_idx, seed=4321):
    """options 4 and 3 against the oracle's output; returns the (handed back, listed) pair both must agree on"""
    seen = {}
    for chain in (4, 3):
        argb, idx, path, (n_split, n_side, n_listed) = _run(nq, img, pal, op, tile, 1, chain, seed=seed)
        assert (n_split, n_side) == (1, 0) and path[0] == 1, (chain, n_split, n_side, path)
        bad = int((idx.astype(np.int32) != want_idx).sum())
        assert bad == 0, "chain=%d: %d of %d indices differ from the oracle" % (chain, bad, want_idx.size)
        assert (argb == want_argb).all(), "chain=%d: ARGB differs from the oracle" % chain
        seen[chain] = (path[1], n_listed)
    assert seen[4] == seen[3], seen
    return seen[4]


# ---- 1. workgroup cuts at 8x8 tiles: 516 x 36 = 65 x 5 = 325 tiles, right column 4 wide, bottom row 4 high, 4 x 4 corner --------------------
@pytest.mark.parametrize("run", ["1", "3", "64", "1000"])
def test_workgroup_cuts_8x8(nq, oracle, monkeypatch, run):
    """NQ_PIXEL_RUN tiles per workgroup: 1 (every wavefront but the first of a workgroup starts past g_end), 3 (the cut falls inside a tile
    row, one wavefront of four idles), 64 (the default: six workgroups, the last with 5 tiles), 1000 (one workgroup, g_end = the image's
    tiles).  White pixels list tiles in several wavefronts and in the partial tiles."""
    tile = (8, 8)
    img = _plant(oracle, pixel._base(True), tile, WHITE_88)
    pal, op, want_argb, want_idx, cnt = _want(oracle, ("white", tile), img, 256, tile)
    monkeypatch.setenv("NQ_PIXEL_RUN", run)
    assert _both(nq, img, pal, op, tile, want_argb, want_idx) == (0, _tiles_with_white(img, tile))


# ---- 2. smaller tiles: the per-lane form (four / two tiles per wavefront), partial last wavefront ------------------------------------------
@pytest.mark.parametrize("tile,spots", [((4, 4), WHITE_44), ((8, 4), [(10, 3), (21, -1), (164, 0)])], ids=["4x4", "8x4"])
def test_smaller_tiles(nq, oracle, tile, spots):
    """258 x 18: at 4x4 65 x 5 tiles (the last wavefront holds the 2 x 2 corner alone), at 8x4 33 x 5 (tile 164 is the 2 x 2 corner, the
    last wavefront holds it alone as well)"""
    img = _plant(oracle, pixel._base(False), tile, spots)
    pal, op, want_argb, want_idx, cnt = _want(oracle, ("white", tile), img, 256, tile)
    assert _both(nq, img, pal, op, tile, want_argb, want_idx) == (0, _tiles_with_white(img, tile))


# ---- 3. tile base ---------------------------------------------------------------------------------------------------------------------------
def test_banded_call_reaches_the_pixel_kernel(nq, oracle):
    """nq_set_band with option 4 forced: rows 16..35 of the 516 x 36 image as a band (y_origin 16, tile_base 130).  The banded entry point
    takes the same launch_gilbert_fast, so the pixel kernel runs (a split pass is counted, two tiles listed); the seed of a tile is
    mix64(seed + tile_base + tile) with the band's tile number, the blue-noise position uses y_origin."""
    import torch
    tile, y0, seed = (8, 8), 16, 4321
    img = _plant(oracle, pixel._base(True), tile, [(205, 11), (324, 3), (20, 1)])         # tile 20 lies above the band
    pal, op, want_argb, want_idx, cnt = _want(oracle, ("band", tile), img, 256, tile, seed)
    assert cnt[6] == 3 and cnt[4] == 0, cnt
    h, w = img.shape
    rows = h - y0
    d_in = torch.from_numpy(np.ascontiguousarray(img[y0:]).reshape(-1)).cuda()
    for chain in (4, 3):
        gq = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED, seed=seed, tile=tile)
        try:
            gq.set_params(_copy_params(op, nq.Params))
            gq.set_option(OPT_CHAIN, chain)
            gq.width, gq.height = w, rows
            gq.set_band(y0, h)
            d_out = torch.zeros(w * rows, dtype=torch.int32, device="cuda")
            d_idx = torch.zeros(w * rows, dtype=torch.int16, device="cuda")
            _split_stats_of()
            gq.dither_device(d_in.data_ptr(), pal, True, d_out.data_ptr(), d_idx.data_ptr())
            torch.cuda.synchronize()
            assert _split_stats_of(gq) == (1, 0, 2), chain
            assert gq.dither_path() == (1, 0), chain
            assert (d_idx.cpu().numpy().astype(np.int32).reshape(rows, w) == want_idx[y0:]).all(), chain
            assert (d_out.cpu().numpy().reshape(rows, w) == want_argb[y0:]).all(), chain
        finally:
            gq.close()


# ---- 4. the Lab table -----------------------------------------------------------------------------------------------------------------------
def test_two_palettes_on_one_handle(nq, oracle):
    """the image's own palette, then the palette of another image, then the first again, on ONE handle: each pass must read the table of its
    own list build"""
    tile = (8, 8)
    img = pixel._base(True)
    pal_a, op, argb_a, idx_a, cnt = _want(oracle, ("base", tile), img, 256, tile)
    key = ("other_palette", tile)
    if key not in _ORACLE:
        other = _cap250(synth.uniform_rgb(516, 36, 175))
        oq = oracle.OracleQuantizer(1, other)
        oq.prescan(256)
        pal_b = oq.pnnquan(256)
        oq = oracle.OracleQuantizer(1, img)
        oq.prescan(256)
        oq.pnnquan(256)
        oq.set_params(op)
        oq.set_seed(4321)
        _ORACLE[key] = (pal_b,) + tuple(oq.dither(pal_b, True, tile=tile))
    pal_b, argb_b, idx_b = _ORACLE[key]
    assert len(pal_a) == len(pal_b) == 256 and not (np.asarray(pal_a) == np.asarray(pal_b)).all()
    assert (idx_a != idx_b).any()
    gq = nq.PnnLABQuantizer(img, mode=TILED, seed=4321, tile=tile)
    try:
        gq.set_params(_copy_params(op, nq.Params))
        gq.set_option(OPT_CHAIN, 4)
        for rep, (pal, want_argb, want_idx) in enumerate(((pal_a, argb_a, idx_a), (pal_b, argb_b, idx_b), (pal_a, argb_a, idx_a))):
            _split_stats_of()
            argb, idx = gq.dither(pal, True)
            assert _split_stats_of(gq)[:2] == (1, 0) and gq.dither_path()[0] == 1, rep
            assert (idx.astype(np.int32) == want_idx).all(), "pass %d: indices differ from the oracle" % rep
            assert (argb == want_argb).all(), "pass %d: ARGB differs from the oracle" % rep
    finally:
        gq.close()


def test_palette_of_200(nq, oracle):
    """K = 200: the table's entries 200..255 are zero, as the kernel's own staging left them"""
    tile = (8, 8)
    img = pixel._base(True)
    pal, op, want_argb, want_idx, cnt = _want(oracle, ("k200", tile), img, 200, tile)
    assert len(pal) == 200
    _both(nq, img, pal, op, tile, want_argb, want_idx)


_BATCH = {}


def _batch_images(oracle):
    """five 72 x 40 images (9 x 5 tiles of 8x8) of different content, so five different palettes, and the oracle's convert() of each"""
    if not _BATCH:
        imgs, want = [], []
        for i in range(5):
            img = _cap250(synth.uniform_rgb(72, 40, 180 + i) if i % 2 else synth.gradient_noise(72, 40, 180 + i))
            oq = oracle.OracleQuantizer(1, img, seed=pixel.BATCH_SEED)
            oq.prescan(256)
            pal = oq.pnnquan(256)
            _counters(oracle, reset=True)
            argb, idx = oq.dither(pal, True, tile=pixel.BATCH_TILE)
            cnt = _counters(oracle)
            assert cnt[4] == 0 and cnt[6] == 0, (i, cnt)
            imgs.append(img)
            want.append((pal, argb, idx))
        for i in range(1, 5):
            assert len(want[i][0]) != len(want[0][0]) or not (np.asarray(want[i][0]) == np.asarray(want[0][0])).all()
        _BATCH["imgs"], _BATCH["want"] = imgs, want
    return _BATCH["imgs"], _BATCH["want"]


@pytest.mark.parametrize("sets", ["2", "3"])
def test_batch_of_five_palettes(nq, oracle, monkeypatch, sets):
    """nq_convert_batch_device, NQ_FINISH_SETS scratch sets in rotation: image i dithers from set i % S while image i + 1 builds its lists;
    with 2 sets every set is reused by another palette, with 3 the rotation is out of step with the parity.
    Five 72 x 40 images: 2880 pixels give convert() a weight near 0.09, so GilbertCurve runs with DITHER_MAX 9 and the generic dither
    kernel takes these images -- the list builders still write a table per image into the rotating sets, nothing reads it, and the outputs
    must be the oracle's.  Then five 516 x 44 images of different palettes (the fixtures of test_gpu_dither_pixel.py, computed once for both
    files: two noise images, and one with 1, 390 and 1 white pixels, which change the palette and list tiles): weight 0.0115, every image
    through gilbert_pixel_kernel on the side-stream form, each reading the table of its own set."""
    import torch
    monkeypatch.setenv("NQ_FINISH_SETS", sets)
    imgs, want = _batch_images(oracle)
    qs = []
    try:
        for img in imgs:
            q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED, seed=pixel.BATCH_SEED, tile=pixel.BATCH_TILE)
            q.height, q.width = img.shape
            qs.append(q)
        d_in = [torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda() for img in imgs]
        outs = [torch.zeros_like(d) for d in d_in]
        idxs = [torch.zeros(d.numel(), dtype=torch.int16, device="cuda") for d in d_in]
        pals = nq.convert_batch_device(qs, [d.data_ptr() for d in d_in], 256, True, [o.data_ptr() for o in outs], [x.data_ptr() for x in idxs])
        torch.cuda.synchronize()
        for i, (pal, argb, idx) in enumerate(want):
            assert len(pals[i]) == len(pal) and (pals[i] == pal).all(), i
            assert (idxs[i].cpu().numpy().astype(np.int32).reshape(idx.shape) == idx).all(), "image %d: indices differ from the oracle" % i
            assert (outs[i].cpu().numpy().reshape(argb.shape) == argb).all(), "image %d: ARGB differs from the oracle" % i
    finally:
        for q in qs:
            q.close()
    names = ("none", "all", "clean_b", "one", "one_corner")
    big = pixel._batch_images(oracle)[1]
    for a in range(5):
        for b in range(a + 1, 5):
            pa, pb = np.asarray(big[names[a]][0]), np.asarray(big[names[b]][0])
            assert pa.shape != pb.shape or not (pa == pb).all(), (names[a], names[b])
    pixel._batch_check(nq, oracle, names)          # (asserts the split form on the side stream for all five, and every output)
