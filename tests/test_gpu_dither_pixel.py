"""The pixel form of the split dither pass (csrc/nq_dither_fast.hip, NQ_OPT_DITHER_CHAIN = 4): gilbert_pixel_kernel runs the light pass with
one lane per PIXEL -- lane l of a wavefront is path step l % tilepx of tile l / tilepx of its tile group -- for power-of-two tiles of 16, 32
or 64 pixels.  The only thing a light step takes from the steps before it is the tile's java.util.Random, and that is a 48-bit LCG: the draw
of a step is the (n + 1)-th state behind the tile seed, n = the earlier steps of the tile that drew (the pick draws exactly when
closest[2] != 0), taken from a jump table.  A tile with a step that needs the error chain, or whose draw nextInt(32767) would reject, goes
onto the need list and is not written; the chain pass walks it with the sequential Random.

Every stand-alone case runs option 4, option 3 (gilbert_light_kernel, one lane per tile) and the generic kernel, each against the oracle's
tiled dither bit for bit, indices and ARGB; the listed and handed-back counts of option 4 must be those of option 3 and of the oracle's event
counters ([4] second-stage entries, [6] direct-branch pixels).

Fixtures.  The bases are those of test_gpu_dither_split.py (516 x 36 at 8x8 tiles: 325 tiles = 65 x 5, right column 4 wide, bottom row 4
high, one tile per wavefront iteration, the last of them the 4 x 4 corner with 48 of 64 lanes dead; 258 x 18 at 4x4 tiles: four tiles per
wavefront, partial tiles 2 wide and 2 high, the last wavefront holds the 2 x 2 corner alone), capped at 250 so that no tile is listed, with
flat patches painted over them whose colours the palette then holds exactly: a pixel of such a patch often reaches closestColorIndex as the
palette colour itself (closest[2] == 0: NO draw), its neighbours do not, and the patch borders cross the tiles -- so steps without a draw
precede steps with one inside a tile, and a wrong draw prefix shows.  Steps without a draw per fixture, from the oracle's counter [7]
(closest[2] == 0 in closestColorIndex; a -DNQ_FAST_COUNT build has the slot FC_PIXEL_NODRAW for the device's count, tools/fast_counts.py):
516 x 36 at 8x8 and 16x16: 361; 258 x 18 at 4x4, 8x4 and 16x4: 208.  Each case asserts at least 200."""
import numpy as np
import pytest

from nquant.android_amd import host, synth

import test_gpu_dither_split as split
from test_gpu_dither_split import OPT_CHAIN, OPT_FAST, TILED, WHITE, _cap250, _copy_params, _counters, _oracle_dither, _plant, _split_stats_of

pytestmark = pytest.mark.gpu

WAYS = ((1, 4), (1, 3), (0, 0))           # (NQ_OPT_FAST_DITHER, NQ_OPT_DITHER_CHAIN)
WEIGHT = 0.0115
# flat patches (x0, y0, w, h), each painted with the base's colour at its centre
PATCHES_516 = [(35, 3, 42, 13), (203, 10, 37, 22), (400, 1, 50, 9), (505, 20, 11, 16), (120, 18, 60, 14), (300, 2, 45, 30)]
PATCHES_258 = [(3, 1, 37, 9), (101, 5, 30, 11), (238, 7, 20, 11), (45, 9, 45, 9), (140, 0, 50, 6), (196, 3, 35, 13), (5, 11, 30, 7), (95, 0, 40, 4),
               (135, 8, 50, 10)]
_BASE = {}
_ORACLE = {}


def _base(big):
    if big not in _BASE:
        src = _cap250(synth.gradient_noise(516, 36, 171) if big else synth.gradient_noise(258, 18, 172))
        img = src.copy()
        for x0, y0, w, h in (PATCHES_516 if big else PATCHES_258):
            img[y0:y0 + h, x0:x0 + w] = src[y0 + h // 2, x0 + w // 2]
        img.setflags(write=False)
        _BASE[big] = img
    return _BASE[big]


def _want(oracle, key, img, tile, seed=4321):
    """the oracle's dither of a fixture, computed once per key"""
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_dither(oracle, img, 256, tile, WEIGHT, seed)
    return _ORACLE[key]


def _run(nq, img, pal, op, tile, fast, chain, seed=4321):
    """one GPU dither; returns (argb, index, dither_path(), split-stats delta)"""
    gq = nq.PnnLABQuantizer(img, mode=TILED, seed=seed, tile=tile)
    try:
        gq.set_params(_copy_params(op, nq.Params))
        gq.set_option(OPT_FAST, fast)
        gq.set_option(OPT_CHAIN, chain)
        _split_stats_of()
        argb, idx = gq.dither(pal, True)
        stats = _split_stats_of(gq)
        return argb, idx, gq.dither_path(), stats
    finally:
        gq.close()


def _check(nq, oracle, key, img, tile, ways=WAYS):
    """oracle vs the GPU paths; returns (the oracle's counters, {chain: (tiles handed back, tiles listed)})"""
    pal, op, want_argb, want_idx, cnt = _want(oracle, key, img, tile)
    seen = {}
    for fast, chain in ways:
        argb, idx, path, (n_split, n_side, n_listed) = _run(nq, img, pal, op, tile, fast, chain)
        assert (n_split, n_side) == (1 if chain in (3, 4) else 0, 0), (fast, chain, n_split, n_side)
        assert path[0] == fast, (fast, chain)
        bad = int((idx.astype(np.int32) != want_idx).sum())
        assert bad == 0, "fast=%d chain=%d: %d of %d indices differ from the oracle" % (fast, chain, bad, want_idx.size)
        assert (argb == want_argb).all(), "fast=%d chain=%d: ARGB differs from the oracle" % (fast, chain)
        seen[chain] = (path[1], n_listed)
    if 3 in seen and 4 in seen:
        assert seen[4] == seen[3], seen
    return cnt, seen


# tile -> the large (516 x 36) or the small (258 x 18) base
SHAPES = {(8, 8): True, (4, 4): False, (8, 4): False, (16, 4): False, (16, 16): True}


@pytest.mark.parametrize("tile", sorted(SHAPES))
def test_no_tile_listed(nq, oracle, tile):
    """8x8: one tile per wavefront iteration, 4x4: four, 8x4: two, 16x4: one (64 pixels); 16x16 keeps gilbert_light_kernel under option 4
    and still counts as a split pass"""
    cnt, seen = _check(nq, oracle, ("base", tile), _base(SHAPES[tile]), tile)
    assert cnt[4] == 0 and cnt[6] == 0, cnt
    assert cnt[7] >= 200, "steps without a draw in the fixture: %d" % cnt[7]
    assert seen[4] == (0, 0) and seen[0] == (0, 0), seen


def _tiles_with_white(img, tile):
    ys, xs = np.nonzero(img == WHITE)
    tiles_x = (img.shape[1] + tile[0] - 1) // tile[0]
    return len({(int(y) // tile[1]) * tiles_x + int(x) // tile[0] for y, x in zip(ys, xs)})


# (tile number, path step) of the white pixels: first and last steps of tiles in different wavefronts, and the partial tiles
WHITE_88 = [(3, 0), (70, -1), (129, 0), (129, -1), (200, 0), (200, -1), (300, -1), (322, 0), (324, 0), (324, -1)]
# 258 x 18 at 4x4: 65 x 5 tiles, a wavefront holds four: tiles 5 and 7 are the second and fourth tile of wavefront 1, 41 and 43 of wavefront 10
WHITE_44 = [(5, 0), (7, -1), (41, -1), (43, 0), (64, 0), (64, -1), (129, -1), (270, 0), (324, 0), (324, -1)]


@pytest.mark.parametrize("tile,spots", [((8, 8), WHITE_88), ((4, 4), WHITE_44)], ids=["8x8", "4x4"])
def test_planted_white_pixels(nq, oracle, tile, spots):
    img = _plant(oracle, _base(SHAPES[tile]), tile, spots)
    cnt, seen = _check(nq, oracle, ("white", tile), img, tile)
    n_tiles = _tiles_with_white(img, tile)
    assert n_tiles == len({t for t, _ in spots})
    assert cnt[4] == 0 and cnt[6] == int((img == WHITE).sum()), cnt           # every event is a direct-branch pixel: one tile each here
    assert seen[4] == (0, n_tiles), seen


def test_white_pixels_in_two_tiles_of_one_wavefront_other_tiles_written(nq, oracle):
    """8x4 tiles (two per wavefront): white pixels in the first tile of one wavefront and the second of another -- the other tile of each
    wavefront is written by the light pass"""
    tile = (8, 4)
    img = _plant(oracle, _base(False), tile, [(10, 3), (21, -1), (164, 0)])          # 33 x 5 tiles; tile 164 is the 2 x 2 corner
    cnt, seen = _check(nq, oracle, ("white", tile), img, tile)
    assert cnt[6] == 3 and cnt[4] == 0, cnt
    assert seen[4] == (0, 3), seen


def test_hand_back(nq, oracle):
    """pixels with alpha <= 0xF: the lookup hands their tiles back (tile 70 holds a white pixel too: listed, then handed back by the chain
    pass); the counts must be option 3's"""
    tile = (8, 8)
    img = _plant(oracle, _base(True), tile, [(70, 5)])
    img = _plant(oracle, img, tile, [(70, 2), (200, 40), (201, 0), (324, -1), (64, 7)], value=0)
    cnt, seen = _check(nq, oracle, ("handback", tile), img, tile)
    assert cnt[6] == 1, cnt
    assert seen[4] == seen[3] == (5, 1), seen


def test_jump_table(nq):
    """nq_selftest_fast, mode JUMP: for 4096 random states and every n in 0..64 the jumped draw equals the draw after n sequential steps --
    on the device (jr_next) and here (Python integers); states built by inverting the LCG so that next(31) is 2^31 - 1 or 2^31 - 2 report a
    rejected draw, and nothing else does"""
    M, B, MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1
    Minv = pow(M, -1, 1 << 48)
    rng = np.random.default_rng(20240)
    states = [int(v) for v in rng.integers(0, 1 << 48, 4096 - 8, dtype=np.int64)]
    planted = []
    for top, low in ((2 ** 31 - 1, 0), (2 ** 31 - 1, 0x1FFFF), (2 ** 31 - 2, 12345), (2 ** 31 - 2, 0)):
        s1 = top << 17 | low                              # the state whose next(31) is `top`
        s0 = ((s1 - B) * Minv) & MASK                       # ... is the first state behind s0
        assert (s0 * M + B) & MASK == s1
        planted.append(s0)
        planted.append(((s0 - B) * Minv) & MASK)            # ... and the second behind this one
    states += planted
    q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED)
    try:
        out = q.selftest_fast("JUMP", records=np.array(states, np.int64))
    finally:
        q.close()
    assert out.shape == (4096, 66)
    assert (out[:, 65] == 0).all(), "jumped draws differ from jr_next on the device"
    want = np.zeros((4096, 65), np.uint32)
    for i, s in enumerate(states):
        for n in range(65):
            s = (s * M + B) & MASK
            uu = s >> 17
            rejected = uu - uu % 32767 + 32766 >= 2 ** 31
            want[i, n] = uu | (0x80000000 if rejected else 0)
    assert (out[:, :65] == want).all()
    for j in range(4):
        assert out[4088 + 2 * j, 0] >> 31 == 1 and out[4088 + 2 * j + 1, 1] >> 31 == 1, j
    assert int((want >> 31).sum()) == 8


def test_reject_switch(nq, oracle, monkeypatch):
    """NQ_LIGHT_REJECT=3: a draw whose low three bits are zero counts as rejected, so most tiles go to the chain pass -- and the output is
    still the oracle's: listing a tile is always safe"""
    tile = (8, 8)
    pal, op, want_argb, want_idx, cnt = _want(oracle, ("base", tile), _base(True), tile)
    monkeypatch.setenv("NQ_LIGHT_REJECT", "3")
    argb, idx, path, stats = _run(nq, _base(True), pal, op, tile, 1, 4)
    monkeypatch.delenv("NQ_LIGHT_REJECT")
    assert stats[:2] == (1, 0) and path == (1, 0)
    assert stats[2] > 100, stats            # (a tile of 64 steps with ~60 draws escapes with probability (7/8)^60)
    assert (idx.astype(np.int32) == want_idx).all() and (argb == want_argb).all()
    argb, idx, path, stats = _run(nq, _base(True), pal, op, tile, 1, 4)
    assert stats == (1, 0, 0)               # the switch is read at every launch


@pytest.mark.parametrize("tile", [(8, 8), (4, 4)])
@pytest.mark.parametrize("run", ["1", "100000"])
def test_workgroup_run_length(nq, oracle, monkeypatch, tile, run):
    """NQ_PIXEL_RUN (tiles per workgroup): one tile group per workgroup, and more groups than the image has (one workgroup)"""
    img = _plant(oracle, _base(SHAPES[tile]), tile, WHITE_88 if tile == (8, 8) else WHITE_44)
    pal, op, want_argb, want_idx, cnt = _want(oracle, ("white", tile), img, tile)
    monkeypatch.setenv("NQ_PIXEL_RUN", run)
    argb, idx, path, stats = _run(nq, img, pal, op, tile, 1, 4)
    assert path == (1, 0) and stats == (1, 0, _tiles_with_white(img, tile))
    assert (idx.astype(np.int32) == want_idx).all() and (argb == want_argb).all()


# ---- the batch entry points: the pixel form is what "automatic" takes; S scratch sets, S - 1 side streams ------------------------------
BATCH_TILE, BATCH_SEED = split.BATCH_TILE, split.BATCH_SEED
_BATCH = {}
CLEAN = ("none", "clean_b", "clean_b", "none", "none", "clean_b", "none", "clean_b", "clean_b")
WHITES = ("one", "all", "one_corner", "all", "one", "one_corner", "one_corner", "one", "all")


def _batch_images(oracle):
    """the four 516 x 44 images of test_gpu_dither_split.py (computed once for both files) and one more clean one"""
    if not _BATCH:
        imgs, want = split._batch_images(oracle)
        imgs, want = dict(imgs), dict(want)
        for name, seed in (("clean_b", 174),):
            img = _cap250(synth.uniform_rgb(516, 44, seed))
            oq = oracle.OracleQuantizer(1, img, seed=BATCH_SEED)
            oq.prescan(256)
            pal = oq.pnnquan(256)
            _counters(oracle, reset=True)
            argb, idx = oq.dither(pal, True, tile=BATCH_TILE)
            cnt = _counters(oracle)
            assert cnt[4] == 0 and cnt[6] == 0, (name, cnt)
            imgs[name], want[name] = img, (pal, argb, idx, 0)
        _BATCH["imgs"], _BATCH["want"] = imgs, want
    return _BATCH["imgs"], _BATCH["want"]


def _batch_check(nq, oracle, names, host_form=False):
    import torch
    imgs, want = _batch_images(oracle)
    qs = []
    try:
        for k in names:
            q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED, seed=BATCH_SEED, tile=BATCH_TILE)
            q.height, q.width = imgs[k].shape
            qs.append(q)
        _split_stats_of()
        if host_form:
            src = [np.ascontiguousarray(imgs[k]).reshape(-1) for k in names]
            outs = [np.zeros_like(s) for s in src]
            idxs = [np.zeros(s.size, np.uint16) for s in src]
            pals = host.convert_batch_host(qs, [s.ctypes.data for s in src], 256, True, [o.ctypes.data for o in outs], [x.ctypes.data for x in idxs])
            got = [(o, x.astype(np.int32)) for o, x in zip(outs, idxs)]
        else:
            d_in = [torch.from_numpy(np.ascontiguousarray(imgs[k]).reshape(-1)).cuda() for k in names]
            outs = [torch.zeros_like(d) for d in d_in]
            idxs = [torch.zeros(d.numel(), dtype=torch.int16, device="cuda") for d in d_in]
            pals = nq.convert_batch_device(qs, [d.data_ptr() for d in d_in], 256, True, [o.data_ptr() for o in outs], [x.data_ptr() for x in idxs])
            torch.cuda.synchronize()
            got = [(o.cpu().numpy(), x.cpu().numpy().astype(np.int32)) for o, x in zip(outs, idxs)]
        assert _split_stats_of() == (len(names), len(names), 0), "not the split form on the side stream"
        for i, k in enumerate(names):
            pal, argb, idx, direct = want[k]
            what = "image %d (%s)" % (i, k)
            assert len(pals[i]) == len(pal) and (pals[i] == pal).all(), what
            assert qs[i].dither_path() == (1, 0), what
            assert _split_stats_of(qs[i]) == (0, 0, direct), what
            assert (got[i][1].reshape(idx.shape) == idx).all(), what
            assert (got[i][0].reshape(argb.shape) == argb).all(), what
    finally:
        for q in qs:
            q.close()


@pytest.mark.parametrize("sets", ["2", "3", "4"])
@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_batch_device(nq, oracle, monkeypatch, lanes, sets):
    """nine images through nq_convert_batch_device: clean ones (no tile listed), then one with white pixels in every image (1, 390 or 1
    tiles listed: every chain pass has work, on a side stream)"""
    monkeypatch.setenv("NQ_BATCH_LANES", lanes)
    monkeypatch.setenv("NQ_FINISH_SETS", sets)
    _batch_check(nq, oracle, CLEAN)
    _batch_check(nq, oracle, WHITES)


@pytest.mark.parametrize("sets", ["2", "4"])
def test_batch_host_buffers(nq, oracle, monkeypatch, sets):
    monkeypatch.setenv("NQ_FINISH_SETS", sets)
    _batch_check(nq, oracle, ("none", "one", "clean_b", "all", "none"), host_form=True)
