"""The light walk of the specialised dither kernel (csrc/nq_dither_fast.hip, NQ_OPT_DITHER_CHAIN): a wavefront first walks its tiles
without the error-diffusion chain and starts over with the chain at the first step whose index depends on it (the direct branch
`K >= 256 && sal > .99`, or the second stage of ditherPixel).  Every case runs three ways -- option 0 (automatic), option 1 (the chain in
every step) and the generic kernel (NQ_OPT_FAST_DITHER off) -- and each must equal the oracle's tiled dither bit for bit, indices and ARGB.

The oracle's event counters (nqo_debug_counters: [4] = entries into the second stage of ditherPixel, [6] = direct-branch pixels) are
asserted per case, so that a case really holds the events it is built for.

Shapes: 516 x 36 with 8x8 tiles = 65 x 5 = 325 tiles (two workgroups; wavefront 5 holds tiles 320..324 and 59 dead lanes; the right
column is 4 wide, the bottom row 4 high; 16-byte row write-out) and 258 x 18 with 4x4 tiles = 65 x 5 tiles (right column 2 wide, bottom row
2 high; scalar write-out).  The base images hold no channel above 250: L <= 98.2, no saliency above .99, every wavefront stays light.

Measured on the CPU oracle for the second-stage cases: (256, gradient_noise(96, 96, 146), weight 0.003) has margin 8 but counter 4 = 0
(gamma * acceptedDiff = .18 * 248 = 44.6 is never exceeded), and (128, ..., weight 0.006) has counter 4 = 0 as well; both stay in as
parity cases.  The second stage is live WITH the light walk (2 * acceptedDiff > 100) for K = 57..65: those cases are added below, margin 8
(weight 0.003: the stage recomputes the colour) and margin 6 (weight >= 0.004: the stage hands back the accumulated colour)."""
import ctypes as C

import numpy as np
import pytest

from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

TILED = 1
OPT_FAST = 2
OPT_CHAIN = 4
WHITE = -1          # 0xFFFFFFFF


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


def _capped(w, h, seed):
    """gradient_noise with every channel <= 250 (L <= 98.2: no pixel takes the direct branch)"""
    u = synth.gradient_noise(w, h, seed).view(np.uint32)
    out = np.uint32(0xFF000000) | np.minimum(u & 0xFF, 250) | (np.minimum((u >> 8) & 0xFF, 250) << 8) | (np.minimum((u >> 16) & 0xFF, 250) << 16)
    return out.astype(np.uint32).view(np.int32)


_BASE = {}


def _base(tile):
    if tile not in _BASE:
        _BASE[tile] = _capped(516, 36, 171) if tile == (8, 8) else _capped(258, 18, 172)
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


def _with_white(oracle, tile, spots):
    img = _base(tile).copy()
    for t, step in spots:
        x, y = _tile_step_xy(oracle, img, tile, t, step)
        img[y, x] = WHITE
    return img


def _check(nq, oracle, kind, K, dither, img, tile, weight, seed=4321):
    """oracle vs the three GPU paths; returns the oracle's counters of its dither pass"""
    oq = oracle.OracleQuantizer(kind, img)
    oq.prescan(K)
    pal = oq.pnnquan(K)
    op = oq.params
    if weight is not None:
        op.weight = weight
        op.isNano = 1 if weight <= .015 else 0
        oq.set_params(op)
    params = _copy_params(op, nq.Params)
    oq.set_seed(seed)
    _counters(oracle, reset=True)
    want_argb, want_idx = oq.dither(pal, dither, tile=tile)
    cnt = _counters(oracle)
    cls = nq.PnnLABQuantizer if kind == 1 else nq.PnnQuantizer
    for fast, chain in ((1, 0), (1, 1), (0, 0)):
        gq = cls(img, mode=TILED, seed=seed, tile=tile)
        gq.set_params(params)
        gq.set_option(OPT_FAST, fast)
        gq.set_option(OPT_CHAIN, chain)
        got_argb, got_idx = gq.dither(pal, dither)
        assert gq.dither_path()[0] == fast, (fast, chain, op.weight, len(pal))
        bad = int((got_idx.astype(np.int32) != want_idx).sum())
        assert bad == 0, "fast=%d chain=%d: %d of %d indices differ from the oracle" % (fast, chain, bad, want_idx.size)
        assert (got_argb == want_argb).all(), "fast=%d chain=%d: ARGB differs from the oracle" % (fast, chain)
    return cnt


@pytest.mark.parametrize("tile", [(8, 8), (4, 4)])
def test_no_direct_pixel_every_wavefront_stays_light(nq, oracle, tile):
    cnt = _check(nq, oracle, 1, 256, True, _base(tile), tile, 0.0115)
    assert cnt[6] == 0 and cnt[4] == 0, cnt


# tile number, path step of the one white pixel (516 x 36, 8x8 tiles: 65 tile columns)
ONE_WHITE = {
    "first_step": (68, 0),
    "last_step": (70, -1),
    "lane0": (128, 20),           # wavefront 2, lane 0
    "lane63": (191, 41),          # wavefront 2, lane 63
    "ragged_corner": (324, 9),    # the 4 x 4 corner tile, lane 4 of the wavefront with 59 dead lanes
}


@pytest.mark.parametrize("where", sorted(ONE_WHITE))
def test_one_white_pixel(nq, oracle, where):
    img = _with_white(oracle, (8, 8), [ONE_WHITE[where]])
    assert int((img == WHITE).sum()) == 1
    cnt = _check(nq, oracle, 1, 256, True, img, (8, 8), 0.0115)
    assert cnt[6] == 1 and cnt[4] == 0, cnt


@pytest.mark.parametrize("tile", [(8, 8), (4, 4)])
def test_white_pixel_in_every_tile_rewalks_at_step_0(nq, oracle, tile):
    img = _with_white(oracle, tile, [(t, 0) for t in range(325)])
    cnt = _check(nq, oracle, 1, 256, True, img, tile, 0.0115)
    assert cnt[6] == 325, cnt


def test_one_white_pixel_per_wavefront_at_the_last_step(nq, oracle):
    """the worst case for the early exit: every wavefront walks all its steps light, then all of them again"""
    spots = [(63, -1), (64, -1), (191, -1), (192, -1), (319, -1), (324, -1)]       # wavefronts 0..5; tile 64 is 4 wide, 319 4 high, 324 4 x 4
    img = _with_white(oracle, (8, 8), spots)
    cnt = _check(nq, oracle, 1, 256, True, img, (8, 8), 0.0115)
    assert cnt[6] == len(spots), cnt


# K, image, weight, counter 4 > 0 expected (None: not asserted -- see the module docstring)
SECOND_STAGE = [
    (256, lambda: synth.gradient_noise(96, 96, 146), 0.003, False),      # margin 8, but gamma * acceptedDiff = 44.6 is out of reach
    (40, lambda: synth.gradient_noise(80, 96, 147), 0.0026, True),       # 2 * acceptedDiff = 56: both Y_Diff tests live, chain in every step
    (128, lambda: synth.gradient_noise(120, 88, 139), 0.006, False),
    (60, lambda: synth.gradient_noise(96, 96, 146), 0.003, True),        # margin 8, 2 * acceptedDiff = 104: light walk, second stage recomputes
    (57, lambda: synth.gradient_noise(96, 96, 146), 0.0045, True),       # margin 6, 2 * acceptedDiff = 102: the stage hands back the accumulated colour
    (65, lambda: synth.uniform_rgb(96, 96, 5), 0.006, True),             # margin 6, K > 64 ladder
]


@pytest.mark.parametrize("K,mk,weight,live", SECOND_STAGE)
def test_second_stage(nq, oracle, K, mk, weight, live):
    cnt = _check(nq, oracle, 1, K, True, mk(), (8, 8), weight)
    assert (cnt[4] > 0) == live, cnt


def test_chain_always_without_dither(nq, oracle):
    """dither = false: GilbertCurve never calls ditherPixel, every step reads the accumulated colour"""
    _check(nq, oracle, 1, 256, False, _base((8, 8)), (8, 8), 0.0115)


def test_chain_always_rgb_kind(nq, oracle):
    """PnnQuantizer (KIND 0) has no saliencies: accumulate -> nearestColorIndex in every step"""
    cnt = _check(nq, oracle, 0, 256, True, synth.uniform_rgb(192, 160, 137), (8, 8), None)
    assert cnt[4] == 0 and cnt[6] == 0, cnt


def test_alternating_the_option_on_one_handle(nq, oracle):
    img = _with_white(oracle, (8, 8), [(5, 7), (200, 63), (324, 0)])
    oq = oracle.OracleQuantizer(1, img)
    oq.prescan(256)
    pal = oq.pnnquan(256)
    op = oq.params
    op.weight = 0.0115
    op.isNano = 1
    oq.set_params(op)
    oq.set_seed(9)
    want_argb, want_idx = oq.dither(pal, True, tile=(8, 8))
    gq = nq.PnnLABQuantizer(img, mode=TILED, seed=9, tile=(8, 8))
    gq.set_params(_copy_params(op, nq.Params))
    for chain in (0, 1, 0, 1):
        gq.set_option(OPT_CHAIN, chain)
        got_argb, got_idx = gq.dither(pal, True)
        assert gq.dither_path() == (1, 0)
        assert (got_idx.astype(np.int32) == want_idx).all() and (got_argb == want_argb).all(), chain
