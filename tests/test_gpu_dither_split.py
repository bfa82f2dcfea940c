"""The split form of the specialised dither kernel (csrc/nq_dither_fast.hip, NQ_OPT_DITHER_CHAIN = 3): gilbert_light_kernel walks every
tile without the error-diffusion chain, a lane whose step needs the chain (the direct branch `K >= 256 && sal > .99`, or the second stage
of ditherPixel) appends its TILE to a need list, blanks the tile's write-out and goes idle; gilbert_fast_kernel then runs the full walk
over the listed tiles, and the generic kernel over the tiles either of them handed back.  In the finish phase of the batch entry points
the chain pass of image i runs on a side stream beside the light kernel of image i + 1, on two scratch sets by image parity.

Every stand-alone case runs four ways -- option 3 (split), 2 (fused light walk), 1 (the chain in every step) and the generic kernel
(NQ_OPT_FAST_DITHER off) -- and each must equal the oracle's tiled dither bit for bit, indices and ARGB.  The oracle's event counters
(nqo_debug_counters: [4] = entries into the second stage, [6] = direct-branch pixels) are asserted per case; that the split form really ran (and, in a batch, with its
chain pass on the side stream) and how many tiles its light kernel listed is read from the library's cumulative counters (nq_get_dither_split_stats): the listed count is
asserted in every case, so a light kernel that lists more tiles than need the chain does not pass for being redone by the chain pass.

Shapes (those of test_gpu_dither_chainfree.py): 516 x 36 with 8x8 tiles = 65 x 5 = 325 tiles in two workgroups, wavefront 5 holds tiles
320..324 and 59 dead lanes, right column 4 wide, bottom row 4 high, 16-byte row write-out; 258 x 18 with 4x4 tiles (scalar write-out).  The
base images hold no channel above 250, so no tile needs the chain until a case plants a white pixel.  The batch cases convert whole
images (pre-scan, palette, dither), where the image's own histogram sets the GilbertCurve weight: 516 x 44 uniform noise (capped at 250) has
~19 000 bins, weight .0134 -- DITHER_MAX 25, the specialised kernel's family (the 516 x 36 images give .0159 / .027: the generic kernel);
65 x 6 = 390 tiles, wavefront 6 holds tiles 384..389."""
import ctypes as C

import numpy as np
import pytest

from nquant.android_amd import host, synth

pytestmark = pytest.mark.gpu

TILED = 1
OPT_FAST = 2
OPT_CHAIN = 4
WHITE = -1          # 0xFFFFFFFF
WAYS = ((1, 3), (1, 2), (1, 1), (0, 0))       # (NQ_OPT_FAST_DITHER, NQ_OPT_DITHER_CHAIN)


def _copy_params(src, dst_cls):
    p = dst_cls()
    for f, _ in dst_cls._fields_:
        setattr(p, f, getattr(src, f))
    return p


def _counters(oracle, reset=False):
    L = oracle.lib()
    L.nqo_debug_counters.argtypes = [C.c_void_p, C.c_int]
    c = (C.c_int64 * 16)()
    L.nqo_debug_counters(c, 1 if reset else 0)
    return list(c)


def _cap250(img):
    u = img.view(np.uint32)
    out = np.uint32(0xFF000000) | np.minimum(u & 0xFF, 250) | (np.minimum((u >> 8) & 0xFF, 250) << 8) | (np.minimum((u >> 16) & 0xFF, 250) << 16)
    return out.astype(np.uint32).view(np.int32)


_BASE = {}


def _base(tile):
    if tile not in _BASE:
        _BASE[tile] = _cap250(synth.gradient_noise(516, 36, 171) if tile == (8, 8) else synth.gradient_noise(258, 18, 172))
        _BASE[tile].setflags(write=False)
    return _BASE[tile]


def _tile_step_xy(oracle, img, tile, t, step):
    """image position of path step `step` (negative: from the end) of tile number t"""
    h, w = img.shape
    tiles_x = (w + tile[0] - 1) // tile[0]
    ty, tx = divmod(t, tiles_x)
    x0, y0 = tx * tile[0], ty * tile[1]
    xy = oracle.gilbert_path(min(tile[0], w - x0), min(tile[1], h - y0))
    return x0 + int(xy[step][0]), y0 + int(xy[step][1])


def _plant(oracle, base, tile, spots, value=WHITE):
    img = base.copy()
    for t, step in spots:
        x, y = _tile_step_xy(oracle, img, tile, t, step)
        img[y, x] = value
    return img


def _oracle_dither(oracle, img, K, tile, weight, seed):
    """the oracle's palette, parameters, tiled dither and the counters of that dither pass"""
    oq = oracle.OracleQuantizer(1, img)
    oq.prescan(K)
    pal = oq.pnnquan(K)
    op = oq.params
    if weight is not None:
        op.weight = weight
        op.isNano = 1 if weight <= .015 else 0
        oq.set_params(op)
    oq.set_seed(seed)
    _counters(oracle, reset=True)
    want_argb, want_idx = oq.dither(pal, True, tile=tile)
    return pal, op, want_argb, want_idx, _counters(oracle)


_SEEN = [0, 0, 0]


def _split_stats_of(*qs):
    """Called without a quantizer before the pass under test, to set the baseline.  What the dither passes since the last call added to nq_get_dither_split_stats: (split passes, those with the chain pass on a side
    stream, tiles listed); the listed tiles of a pass are counted when its dither_path() is asked, so the quantizers are asked here."""
    for q in qs:
        q.dither_path()
    now = host.dither_split_stats()
    delta = tuple(n - s for n, s in zip(now, _SEEN))
    _SEEN[:] = now
    return delta


def _check(nq, oracle, K, img, tile, weight, seed=4321, ways=WAYS):
    """oracle vs the four GPU paths; returns (the oracle's counters, tiles the split form handed back, tiles its light kernel listed)"""
    pal, op, want_argb, want_idx, cnt = _oracle_dither(oracle, img, K, tile, weight, seed)
    params = _copy_params(op, nq.Params)
    failed = listed = None
    for fast, chain in ways:
        gq = nq.PnnLABQuantizer(img, mode=TILED, seed=seed, tile=tile)
        try:
            gq.set_params(params)
            gq.set_option(OPT_FAST, fast)
            gq.set_option(OPT_CHAIN, chain)
            _split_stats_of()
            got_argb, got_idx = gq.dither(pal, True)
            split, side, n_listed = _split_stats_of(gq)
            assert (split, side) == (1 if chain == 3 else 0, 0), (fast, chain, split, side)
            assert chain == 3 or n_listed == 0, (fast, chain, n_listed)
            assert gq.dither_path()[0] == fast, (fast, chain, op.weight, len(pal))
            bad = int((got_idx.astype(np.int32) != want_idx).sum())
            assert bad == 0, "fast=%d chain=%d: %d of %d indices differ from the oracle" % (fast, chain, bad, want_idx.size)
            assert (got_argb == want_argb).all(), "fast=%d chain=%d: ARGB differs from the oracle" % (fast, chain)
            if chain == 3:
                failed, listed = gq.dither_path()[1], n_listed
        finally:
            gq.close()
    return cnt, failed, listed


@pytest.mark.parametrize("tile", [(8, 8), (4, 4)])
def test_no_tile_listed(nq, oracle, tile):
    cnt, failed, listed = _check(nq, oracle, 256, _base(tile), tile, 0.0115)
    assert cnt[6] == 0 and cnt[4] == 0, cnt
    assert failed == 0 and listed == 0


# tile number, path step of the one white pixel (516 x 36, 8x8 tiles: 65 tile columns)
ONE_LISTED = {
    "step_0": (68, 0),
    "last_step": (70, -1),
    "partial_wavefront_corner": (324, 9),      # the 4 x 4 corner tile, lane 4 of the wavefront with 59 dead lanes
    "right_column": (129, 17),                 # 4 x 8
    "bottom_row": (300, 30),                   # 8 x 4
}


@pytest.mark.parametrize("where", sorted(ONE_LISTED))
def test_one_listed_tile(nq, oracle, where):
    img = _plant(oracle, _base((8, 8)), (8, 8), [ONE_LISTED[where]])
    assert int((img == WHITE).sum()) == 1
    cnt, failed, listed = _check(nq, oracle, 256, img, (8, 8), 0.0115)
    assert cnt[6] == 1 and cnt[4] == 0, cnt
    assert failed == 0 and listed == 1


def test_one_listed_tile_scalar_write_out(nq, oracle):
    img = _plant(oracle, _base((4, 4)), (4, 4), [(324, 2), (64, 5)])         # the 2 x 2 corner tile, a 2 x 4 right-column tile
    cnt, failed, listed = _check(nq, oracle, 256, img, (4, 4), 0.0115)
    assert cnt[6] == 2 and cnt[4] == 0, cnt
    assert failed == 0 and listed == 2


@pytest.mark.parametrize("tile", [(8, 8), (4, 4)])
def test_every_tile_listed(nq, oracle, tile):
    """a white pixel at step 0 of each tile: the light kernel writes nothing, the chain pass everything"""
    img = _plant(oracle, _base(tile), tile, [(t, 0) for t in range(325)])
    cnt, failed, listed = _check(nq, oracle, 256, img, tile, 0.0115)
    assert cnt[6] == 325, cnt
    assert failed == 0 and listed == 325


def test_one_white_pixel_per_wavefront_at_lane_63s_last_step(nq, oracle):
    """the fused form's worst case (every wavefront walks twice); here six tiles are listed"""
    spots = [(63, -1), (127, -1), (191, -1), (255, -1), (319, -1), (324, -1)]       # lane 63 of wavefronts 0..4; the last live lane of wavefront 5
    img = _plant(oracle, _base((8, 8)), (8, 8), spots)
    cnt, failed, listed = _check(nq, oracle, 256, img, (8, 8), 0.0115)
    assert cnt[6] == len(spots) and cnt[4] == 0, cnt
    assert failed == 0 and listed == len(spots) == 6


# K, image, weight: the second stage of ditherPixel is live WITH the light walk (2 * acceptedDiff > 100)
SECOND_STAGE = [
    (60, lambda: synth.gradient_noise(96, 96, 146), 0.003),        # margin 8, 2 * acceptedDiff = 104: the stage recomputes the colour
    (57, lambda: synth.gradient_noise(96, 96, 146), 0.0045),       # margin 6, 2 * acceptedDiff = 102: the stage hands back the accumulated colour
    (65, lambda: synth.uniform_rgb(96, 96, 5), 0.006),             # margin 6, K > 64 ladder
]


@pytest.mark.parametrize("K,mk,weight", SECOND_STAGE)
def test_second_stage_lists_the_tile(nq, oracle, K, mk, weight):
    cnt, failed, listed = _check(nq, oracle, K, mk(), (8, 8), weight)
    assert cnt[4] > 0, cnt
    assert failed == 0
    print("second stage: K %d, %d entries in the oracle, %d of 144 tiles listed" % (K, cnt[4], listed))
    # a tile is listed at its first entry into the second stage (up to there its walk is the oracle's), so no more tiles than entries;
    # 96 x 96 in 8x8 tiles = 144 tiles, and these images leave some of them without an entry
    assert 0 < listed <= min(cnt[4], 143)


def test_tile_handed_back_and_listed(nq, oracle):
    """Tile 70 holds a pixel with alpha <= 0xF (step 2) and a white pixel (step 5): the light kernel lists it, the chain pass hands it
    back; tile 200 holds only such a pixel: the light kernel hands it back.  The generic pass over the hand-back list overwrites, so it has
    to run behind the chain pass."""
    img = _plant(oracle, _base((8, 8)), (8, 8), [(70, 5)])
    img = _plant(oracle, img, (8, 8), [(70, 2), (200, 40)], value=0)
    cnt, failed, listed = _check(nq, oracle, 256, img, (8, 8), 0.0115)
    assert cnt[6] == 1, cnt
    assert listed == 1                # tile 70: the light kernel walks on past the transparent pixel and lists the tile at the white one
    assert failed == 2                # tile 200 by the light kernel, tile 70 by the chain pass (the transparent pixel at its step 2)


def test_banded_call(nq, oracle):
    """nq_set_band: rows 16..35 of the 516 x 36 image as a band of their own (y_origin 16, tile_base 130), white pixels in a full tile and
    in the corner tile of the band, against the oracle's rows."""
    import torch
    tile, y0, seed = (8, 8), 16, 4321
    img = _plant(oracle, _base(tile), tile, [(205, 11), (324, 3), (20, 1)])         # tile 20 lies above the band
    pal, op, want_argb, want_idx, cnt = _oracle_dither(oracle, img, 256, tile, 0.0115, seed)
    assert cnt[6] == 3 and cnt[4] == 0, cnt
    h, w = img.shape
    rows = h - y0
    d_in = torch.from_numpy(np.ascontiguousarray(img[y0:]).reshape(-1)).cuda()
    for chain in (3, 2, 1):
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
            assert _split_stats_of(gq) == ((1, 0, 2) if chain == 3 else (0, 0, 0)), chain       # tiles 205 and 324; tile 20 is not in the band
            assert gq.dither_path() == (1, 0), chain
            assert (d_idx.cpu().numpy().astype(np.int32).reshape(rows, w) == want_idx[y0:]).all(), chain
            assert (d_out.cpu().numpy().reshape(rows, w) == want_argb[y0:]).all(), chain
        finally:
            gq.close()


def test_split_three_times_over(nq, oracle):
    """the order of the need list comes from atomics: the outputs must not"""
    spots = [(t, (7 * t) % 32) for t in range(0, 320, 3)] + [(324, 15)]       # (every tile of rows 0..4 but the corner has >= 32 steps)
    img = _plant(oracle, _base((8, 8)), (8, 8), spots)
    pal, op, want_argb, want_idx, cnt = _oracle_dither(oracle, img, 256, (8, 8), 0.0115, 77)
    assert cnt[6] == len(spots), cnt
    gq = nq.PnnLABQuantizer(img, mode=TILED, seed=77, tile=(8, 8))
    try:
        gq.set_params(_copy_params(op, nq.Params))
        gq.set_option(OPT_CHAIN, 3)
        for rep in range(3):
            _split_stats_of()
            got_argb, got_idx = gq.dither(pal, True)
            assert gq.dither_path() == (1, 0) and _split_stats_of(gq) == (1, 0, len(spots)), rep
            assert (got_idx.astype(np.int32) == want_idx).all() and (got_argb == want_argb).all(), rep
    finally:
        gq.close()


# ---- the batch entry point: chain pass on the side stream, two scratch sets by parity --------------------------------------------
BATCH_TILE, BATCH_SEED = (8, 8), 11
_BATCH = {}


def _batch_images(oracle):
    """none, one tile, all tiles, none, one tile -- and the oracle's whole convert() of each"""
    if not _BATCH:
        base = _cap250(synth.uniform_rgb(516, 44, 173))
        imgs = {"none": base, "one": _plant(oracle, base, BATCH_TILE, [(70, 5)]),
                "all": _plant(oracle, base, BATCH_TILE, [(t, 0) for t in range(390)]),
                "one_corner": _plant(oracle, base, BATCH_TILE, [(389, 3)])}
        want = {}
        for name, img in imgs.items():
            oq = oracle.OracleQuantizer(1, img, seed=BATCH_SEED)
            oq.prescan(256)
            pal = oq.pnnquan(256)
            _counters(oracle, reset=True)
            argb, idx = oq.dither(pal, True, tile=BATCH_TILE)
            cnt = _counters(oracle)
            assert cnt[4] == 0, (name, cnt)
            want[name] = (pal, argb, idx, cnt[6])
        assert [want[k][3] for k in ("none", "one", "all", "one_corner")] == [0, 1, 390, 1]
        _BATCH["imgs"], _BATCH["want"] = imgs, want
    return _BATCH["imgs"], _BATCH["want"]


@pytest.mark.parametrize("names", [("none", "one", "all", "none", "one_corner"), ("one",)], ids=["five", "single"])
def test_batch_on_a_callers_stream_twice(nq, oracle, names):
    """convert_batch_device on a caller-created stream, twice on the same handles: the side stream, both scratch sets, their reuse at
    image i + 2, the re-zeroed counts; with one image the join at the end of the phase runs without a successor."""
    import torch
    imgs, want = _batch_images(oracle)
    stream = torch.cuda.Stream()
    qs = []
    try:
        with torch.cuda.stream(stream):
            d_in = [torch.from_numpy(np.ascontiguousarray(imgs[k]).reshape(-1)).cuda() for k in names]
        for k in names:
            q = nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED, seed=BATCH_SEED, tile=BATCH_TILE)
            q.height, q.width = imgs[k].shape
            qs.append(q)
        qs[0].set_stream(stream.cuda_stream)
        for rep in range(2):
            with torch.cuda.stream(stream):
                outs = [torch.zeros_like(d) for d in d_in]
                idxs = [torch.zeros(d.numel(), dtype=torch.int16, device="cuda") for d in d_in]
            _split_stats_of()
            pals = nq.convert_batch_device(qs, [d.data_ptr() for d in d_in], 256, True, [o.data_ptr() for o in outs], [x.data_ptr() for x in idxs])
            stream.synchronize()
            assert _split_stats_of() == (len(names), len(names), 0), "pass %d: not the split form on the side stream" % rep
            for i, k in enumerate(names):
                pal, argb, idx, direct = want[k]
                what = "pass %d, image %d (%s)" % (rep, i, k)
                assert len(pals[i]) == len(pal) and (pals[i] == pal).all(), what
                assert qs[i].dither_path()[0] == 1, what
                assert _split_stats_of(qs[i]) == (0, 0, direct), what          # 0, 1, 390, 0, 1 tiles listed
                assert (idxs[i].cpu().numpy().astype(np.int32).reshape(idx.shape) == idx).all(), what
                assert (outs[i].cpu().numpy().reshape(argb.shape) == argb).all(), what
    finally:
        stream.synchronize()
        for q in qs:
            q.close()
