"""The quantizer at degenerate image and tile geometry: 1x1 placeholders, one-pixel-high strips, thumbnails below one wavefront of
pixels, tiles larger than the image, remainder tiles of one column, Gilbert paths shorter than the five steps of the specialised
kernel's register window, one-row bands, 1x1 frames.  Every comparison is exact equality with the CPU oracle (oracle/nq_oracle.c),
which throws on none of these inputs: NQ_ERR_UNSUPPORTED and NQ_ERR_REFERENCE_THROWS are failures here, and no case of the grid is
skipped.  Each test walks its whole part of the grid, collects every disagreement and fails with the list."""
import numpy as np
import pytest

from nquant.android_amd import synth
from test_gpu_frames import _cls, _copy_params

pytestmark = pytest.mark.gpu

SEQ, TILED = 0, 1
SHAPES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (1, 3), (3, 3), (2, 3), (5, 4), (4, 5), (7, 7), (8, 8), (9, 8), (15, 16), (16, 15),
          (17, 17), (17, 1), (1, 17), (64, 1), (1, 64), (65, 1), (1, 65), (33, 3), (3, 33), (63, 2), (2, 63)]      # (width, height)
KS = [1, 2, 3, 16, 256]
SEED = 5
GENS = {   # every generator is seeded per shape
    "uniform": lambda w, h, s: synth.uniform_rgb(w, h, s),
    "gradient": lambda w, h, s: synth.gradient_noise(w, h, s),
    "few3": lambda w, h, s: synth.few_colors(w, h, s, 3),
    "alpha": lambda w, h, s: synth.with_alpha(synth.uniform_rgb(w, h, s), s, p_transparent=0.2, p_semi=0.3),
    "one_colour": lambda w, h, s: np.full((h, w), -1, np.int32),              # opaque white everywhere
    "transparent": lambda w, h, s: np.zeros((h, w), np.int32),                # every pixel 0
}
# the 14 scalars test_gpu_parity.py compares after pnnquan
SCALARS = ("hasSemiTransparency", "transparentPixelIndex", "transparentColor", "maxbins", "quan_rt", "isNano", "texicab",
           "paletteLength", "PR", "PG", "PB", "PA", "ratio", "weight")
# nMaxColors <= 2: convert() does not call pnnquan (NQ/PnnQuantizer.java:441-452), so the fields pnnquan alone computes have no
# reference value; the ones the pre-scan and convert() itself set do
SCALARS_K2 = ("hasSemiTransparency", "transparentPixelIndex", "transparentColor", "isNano", "paletteLength", "PR", "PG", "PB", "PA",
              "ratio", "weight")
BLACK, WHITE = np.int32(-16777216), np.int32(-1)


def _image(gen, w, h):
    img = np.ascontiguousarray(GENS[gen](w, h, w * 31 + h))
    assert img.shape == (h, w) and img.dtype == np.int32
    return img


def _clamped(tile, w, h):
    return (min(tile[0], w), min(tile[1], h))


def _diff(got_argb, got_idx, want_argb, want_idx):
    """'' when both outputs are the oracle's, else a short description."""
    if got_idx.shape != want_idx.shape or got_argb.shape != want_argb.shape:
        return "shape %s / %s, oracle %s" % (got_idx.shape, got_argb.shape, want_idx.shape)
    bi, ba = int((got_idx.astype(np.int32) != want_idx).sum()), int((got_argb != want_argb).sum())
    return "" if bi == 0 and ba == 0 else "%d indices, %d ARGB pixels of %d differ" % (bi, ba, want_idx.size)


def _gpu(nq, bad, tag, fn):
    """fn() on the GPU side; an error status is a failure of the case (the oracle throws on none of them).  A HIP runtime error ends
    the test at once: nothing more is started on the device."""
    try:
        return fn()
    except nq.NqError as e:
        if e.status == -2:
            raise
        bad.append("%s: %s" % (tag, e))
        return None


def _report(bad, n):
    print("%d cases, %d disagreements" % (n, len(bad)))
    assert not bad, "%d of %d cases disagree with the oracle:\n%s" % (len(bad), n, "\n".join(bad[:40]))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. whole convert() in REFERENCE_SEQUENTIAL mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", list(GENS))
@pytest.mark.parametrize("kind", [0, 1])
def test_whole_convert_sequential_equals_oracle_convert(nq, oracle, kind, gen):
    """26 shapes x K {1, 2, 3, 16, 256} x dither on / off = 260 converts per (kind, generator): palette, index map and ARGB."""
    bad, n = [], 0
    for (w, h) in SHAPES:
        img = _image(gen, w, h)
        gq = _cls(nq, kind)(img, mode=SEQ, seed=SEED)
        for K in KS:
            for dither in (False, True):
                tag = "kind %d %s %dx%d K %d dither %d" % (kind, gen, w, h, K, dither)
                n += 1
                oq = oracle.OracleQuantizer(kind, img, seed=SEED)
                want_argb, want_idx, want_pal = oq.convert(K, dither)
                oq.close()
                out = _gpu(nq, bad, tag, lambda: gq.convert(K, dither))
                if out is None:
                    continue
                if len(out.palette) != len(want_pal) or (out.palette != want_pal).any():
                    bad.append("%s: palette %s, oracle %s" % (tag, out.palette[:4], want_pal[:4]))
                    continue
                d = _diff(out.argb, out.index, want_argb, want_idx)
                if d:
                    bad.append("%s: %s" % (tag, d))
        gq.close()
    _report(bad, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. pnnquan + tiled dither
# ---------------------------------------------------------------------------------------------------------------------------------
TILES_B = [(4, 4), (16, 16), (7, 5), (1, 1), None]        # None: automatic on the GPU = 4x4 at these sizes


def _oracle_palette(oracle, kind, img, K):
    """The oracle after convert()'s pre-scan and palette step, ready for nqo_dither_tiled: (quantizer, palette)."""
    oq = oracle.OracleQuantizer(kind, img, seed=SEED)
    oq.prescan(K)
    if K > 2:
        return oq, oq.pnnquan(K)
    # NQ/PnnQuantizer.java:441-452, restated as nqo_convert does (and checked against it)
    p = oq.params
    pal = np.array([p.transparentColor, BLACK] if p.transparentPixelIndex >= 0 else [BLACK, WHITE], np.int32)[:K]
    p.weight = 1.0
    p.paletteLength = K
    oq.set_params(p)
    ref = oracle.OracleQuantizer(kind, img, seed=SEED)
    assert (ref.convert(K, False)[2] == pal).all()
    ref.close()
    return oq, pal


@pytest.mark.parametrize("dither", [False, True])
@pytest.mark.parametrize("gen", list(GENS))
@pytest.mark.parametrize("kind", [0, 1])
def test_pnnquan_and_tiled_dither_equal_oracle(nq, oracle, kind, gen, dither):
    """26 shapes x 5 K = 130 palettes (+ the 14 scalars) and x 5 tiles = 650 tiled dithers per (kind, generator, dither).  A tile
    larger than the image must give what the tile clamped to the image gives (the oracle is asked for both)."""
    bad, n = [], 0
    for (w, h) in SHAPES:
        img = _image(gen, w, h)
        gq = _cls(nq, kind)(img, mode=TILED, seed=SEED)
        for K in KS:
            tag = "kind %d %s %dx%d K %d dither %d" % (kind, gen, w, h, K, dither)
            n += 1
            oq, want_pal = _oracle_palette(oracle, kind, img, K)
            got_pal = _gpu(nq, bad, tag + " pnnquan", lambda: gq.pnnquan(K))
            if got_pal is None:
                continue
            if len(got_pal) != len(want_pal) or (got_pal != want_pal).any():
                bad.append("%s: palette %s, oracle %s" % (tag, got_pal[:4], want_pal[:4]))
                continue
            po, pg = oq.params, gq.params
            for f in (SCALARS if K > 2 else SCALARS_K2):
                # (the oracle leaves paletteLength unset on the few-colours early return: the length itself is the reference)
                want_f = len(want_pal) if f == "paletteLength" else getattr(po, f)
                if getattr(pg, f) != want_f:
                    bad.append("%s: %s is %r, oracle %r" % (tag, f, getattr(pg, f), want_f))
            for tile in TILES_B:
                n += 1
                otile = _clamped(tile or (4, 4), w, h)
                oq.set_seed(SEED)
                want_argb, want_idx = oq.dither(want_pal, dither, tile=otile)
                if tile is not None and otile != tile:
                    oq.set_seed(SEED)
                    big_argb, big_idx = oq.dither(want_pal, dither, tile=tile)
                    assert (big_argb == want_argb).all() and (big_idx == want_idx).all(), "the oracle itself: tile %s on %dx%d" % (tile, w, h)
                if tile is None:
                    gq.set_tile(0, 0)
                else:
                    gq.set_tile(*tile)
                got = _gpu(nq, bad, "%s tile %s" % (tag, tile), lambda: gq.dither(got_pal, dither))
                if got is None:
                    continue
                d = _diff(got[0], got[1], want_argb, want_idx)
                if d:
                    bad.append("%s tile %s: %s" % (tag, tile, d))
            oq.close()
        gq.close()
    _report(bad, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the dither stage with an injected 256-colour palette (K > 32 and the specialised kernel on images that cannot hold 33 colours)
# ---------------------------------------------------------------------------------------------------------------------------------
TILES_C = [(4, 4), (8, 8), (16, 16), (7, 5), (1, 1), (64, 1), (1, 64)]
_BIG = {}


def _big_palette(oracle, kind):
    """Palette and params of the oracle on gradient_noise(96, 96, 7) at K = 256, computed once per kind."""
    if kind not in _BIG:
        oq = oracle.OracleQuantizer(kind, synth.gradient_noise(96, 96, 7))
        oq.prescan(256)
        pal = oq.pnnquan(256)
        assert len(pal) == 256
        p = oq.params
        if p.distinctColors <= 0:            # (the tiled BlueNoise weight needs a count: the same one goes to both sides)
            p.distinctColors = 9216
        _BIG[kind] = (pal, p)
        oq.close()
    return _BIG[kind]


def _injected(oracle, kind, weight):
    """(palette, oracle params) with the palette's own weight (weight None) or the DITHER_MAX 25 family of fuzz_parity.py's fast mode."""
    pal, p0 = _big_palette(oracle, kind)
    p = _copy_params(p0, oracle.Params)
    if weight is not None:
        p.weight = weight
        p.isNano = 1
    return pal, p


def _fast_expected(kind, p, dither, asked):
    """Whether gilbert_fast_kernel must have run with the INJECTED weight (.008, isNano: DITHER_MAX 25, no sorted queue), restating
    gilbert_fast_eligible (csrc/nq_dither_fast.hip) for exactly what test_dither_stage_with_injected_palette feeds it.  It assumes:
      * K = 256, no semi-transparency, nMaxColors > 2 and the candidate lists switched on (closest and nearest lists exist);
      * every tile holds 1..1024 pixels (TILES_C);
      * LAB kind: the rule fuzz_parity.py's fast mode asserts -- the kernel runs when asked for and ratio >= 0;
      * RGB kind (beyond what fuzz_parity.py pins): the kernel exists for dither = true on an image WITHOUT a transparent colour (the
        RGB nearest lists are built for such images only) and without saliencies (the RGB kind has none).  The "gradient" generator is
        opaque; with another generator this expectation has to be restated."""
    if not asked:
        return 0
    if kind == 1:
        return 1 if p.ratio >= 0 else 0
    assert p.transparentPixelIndex < 0 and not p.hasSemiTransparency
    return 1 if dither else 0


@pytest.mark.parametrize("dither", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_dither_stage_with_injected_palette(nq, oracle, kind, dither):
    """26 shapes x 7 tiles x {own weight, weight .008 with the specialised kernel off, ... on} = 546 dithers per (kind, dither); with the
    injected weight the kernel that ran is checked through dither_path(): a silent fall-back to the generic kernel fails."""
    bad, n = [], 0
    own = _big_palette(oracle, kind)[1].weight
    for (w, h) in SHAPES:
        img = _image("gradient", w, h)
        gq = _cls(nq, kind)(img, mode=TILED, seed=9)
        for tile in TILES_C:
            gq.set_tile(*tile)
            for weight, fast in ((None, None), (0.008, 0), (0.008, 1)):
                n += 1
                tag = "kind %d %dx%d tile %s dither %d weight %s fast %s" % (kind, w, h, tile, dither, weight, fast)
                pal, p = _injected(oracle, kind, weight)
                oq = oracle.OracleQuantizer(kind, img, seed=9)
                oq.prescan(256)
                oq.set_params(p)
                oq.set_seed(9)
                want_argb, want_idx = oq.dither(pal, dither, tile=tile)
                oq.close()
                gq.set_params(_copy_params(p, nq.Params))
                gq.set_option(2, 1 if fast is None else fast)
                got = _gpu(nq, bad, tag, lambda: gq.dither(pal, dither))
                if got is None:
                    continue
                ran, back = gq.dither_path()
                if weight is not None and ran != _fast_expected(kind, p, dither, fast):
                    bad.append("%s: specialised kernel ran = %d" % (tag, ran))
                if weight is None and own >= .015 and ran != 0:
                    bad.append("%s: the specialised kernel has no DITHER_MAX 9 form, ran = %d" % (tag, ran))
                d = _diff(got[0], got[1], want_argb, want_idx)
                if d:
                    bad.append("%s (ran %d, handed back %d): %s" % (tag, ran, back, d))
        gq.close()
    _report(bad, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. lookups of 0, 1, 63, 64, 65 colours
# ---------------------------------------------------------------------------------------------------------------------------------
def _lookup_palettes(oracle, kind):
    """(name, image for the handle, palette, oracle quantizer holding the params): the injected palettes of (c) and a 2-entry and a
    3-entry palette of (a)."""
    out = []
    for weight in (None, 0.008):
        pal, p = _injected(oracle, kind, weight)
        img = _image("gradient", 9, 8)
        oq = oracle.OracleQuantizer(kind, img)
        oq.prescan(256)
        oq.set_params(p)
        out.append(("injected256 weight %s" % weight, img, pal, oq))
    for K in (2, 3):
        img = _image("uniform", 3, 3)
        oq, pal = _oracle_palette(oracle, kind, img, K)
        assert len(pal) == K
        out.append(("tiny K %d" % K, img, pal, oq))
    return out


@pytest.mark.parametrize("kind", [1, 0])
def test_lookups_of_very_few_colours(nq, oracle, kind):
    """nearestColorIndex and closestTuple for M in {0, 1, 63, 64, 65} colours (none, one lane, one wavefront less one, exactly one, one more)
    x 4 palettes x candidate lists on / off = 40 calls of each per kind."""
    bad, n = [], 0
    for name, img, pal, oq in _lookup_palettes(oracle, kind):
        gq = _cls(nq, kind)(img, mode=TILED)
        gq.set_params(_copy_params(oq.params, nq.Params))
        for M in (0, 1, 63, 64, 65):
            cols = ((synth.splitmix64(700 + M, M) & np.uint64(0xFFFFFF)).astype(np.uint32) | np.uint32(0xFF000000)).view(np.int32)
            want_idx, want_tup = oq.nearest_index(pal, cols), oq.closest_tuple(pal, cols)
            assert want_idx.shape == (M,) and want_tup.shape == (M, 4)
            for lists in (1, 0):
                n += 1
                tag = "kind %d %s M %d lists %d" % (kind, name, M, lists)
                gq.set_option(1, lists)
                got_idx = _gpu(nq, bad, tag + " nearest", lambda: gq.nearestColorIndex(pal, cols))
                got_tup = _gpu(nq, bad, tag + " closest", lambda: gq.closestTuple(pal, cols))
                if got_idx is not None and (got_idx.shape != want_idx.shape or (got_idx != want_idx).any()):
                    bad.append("%s: nearest %s, oracle %s" % (tag, got_idx[:6], want_idx[:6]))
                if got_tup is not None and (got_tup.shape != want_tup.shape or (got_tup != want_tup).any()):
                    bad.append("%s: %d closest tuples differ" % (tag, int((got_tup != want_tup).any(axis=1).sum())))
        gq.close()
        oq.close()
    _report(bad, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. several images at once
# ---------------------------------------------------------------------------------------------------------------------------------
def _batch_items():
    """(key, description, random seed) items of test_gpu_batch_scale.py: 1x1, 1x17, 65x1 and 3x3 images among 64x48 ones, kinds mixed."""
    descs = [(1, "gradient", 64, 48), (0, "uniform", 1, 1), (1, "uniform", 1, 1), (0, "gradient", 64, 48), (1, "gradient", 1, 17),
             (0, "uniform", 1, 17), (1, "uniform", 65, 1), (0, "gradient", 65, 1), (1, "uniform", 64, 48), (0, "uniform", 3, 3),
             (1, "gradient", 3, 3), (0, "uniform", 64, 48)]
    return [("tiny%d" % i, (kind, gen, w, h, 900 + i, False, 0), 40 + i) for i, (kind, gen, w, h) in enumerate(descs)]


_BATCH_WANT = []


def _batch_want(items):
    """The oracle's convert(256, true), tiled 8x8, of every item: computed once, shared by the two batch tests."""
    import test_gpu_batch_scale as bs
    if not _BATCH_WANT:
        _BATCH_WANT.extend(bs._oracle_one(it)[1] for it in items)
    return _BATCH_WANT


def test_batch_with_tiny_images_device_form(nq, oracle):
    """nq_convert_batch_device over 12 images, each compared with the oracle (palette, scalars, index map, ARGB)."""
    import test_gpu_batch_scale as bs
    items = _batch_items()
    want = _batch_want(items)
    b = bs._Batch(nq, items)
    pals = b.run()
    bs._check_batch(b, pals, want)


def test_batch_with_tiny_images_host_form(nq, oracle):
    """nq_convert_batch (host buffers, page-locked and pageable) over the same 12 images."""
    import torch
    import test_gpu_batch_scale as bs
    items = _batch_items()
    want = _batch_want(items)
    for pinned in (True, False):
        b = bs._Batch(nq, items)
        h_in = [torch.from_numpy(np.ascontiguousarray(im).reshape(-1).copy()) for im in b.imgs]
        h_out = [torch.zeros(t.numel(), dtype=torch.int32) for t in h_in]
        h_idx = [torch.zeros(t.numel(), dtype=torch.int16) for t in h_in]
        if pinned:
            h_in, h_out, h_idx = ([t.pin_memory() for t in ts] for ts in (h_in, h_out, h_idx))
        pals = nq.convert_batch_host(b.qs, [t.data_ptr() for t in h_in], bs.K, True, [t.data_ptr() for t in h_out], [t.data_ptr() for t in h_idx])
        for i in range(len(items)):
            bs._same(pals[i], h_idx[i].numpy().view(np.uint16), h_out[i].numpy(), want[i], "image %d (pinned %d)" % (i, pinned), b.qs[i].params)


def _tiny_frames(seed):
    return [synth.gradient_noise(40, 30, seed), synth.uniform_rgb(1, 1, seed + 1), synth.uniform_rgb(37, 29, seed + 2),
            synth.gradient_noise(1, 64, seed + 3), synth.gradient_noise(17, 23, seed + 4)]


FRAME_CASES = [  # name, kind, K, dither, frames
    ("lab256_dither", 1, 256, True, lambda: _tiny_frames(500)),
    ("lab256_bluenoise", 1, 256, False, lambda: _tiny_frames(510)),
    ("rgb64_dither", 0, 64, True, lambda: _tiny_frames(520)),
    ("lab16_dither", 1, 16, True, lambda: _tiny_frames(530)),
    ("lab256_single_1x1", 1, 256, True, lambda: [synth.uniform_rgb(1, 1, 540)]),
    ("rgb256_single_1x1", 0, 256, False, lambda: [synth.uniform_rgb(1, 1, 541)]),
    ("lab2_single_1x1", 1, 2, True, lambda: [synth.uniform_rgb(1, 1, 542)]),
]


@pytest.mark.parametrize("name,kind,K,dither,mk", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frames_with_a_1x1_and_a_1x64_frame(nq, oracle, name, kind, K, dither, mk):
    """nq_pnnquan_frames_device and nq_convert_frames_device (and the host form) with a 1x1 and a 1x64 frame between ordinary ones, and
    a sequence that is one 1x1 frame: palette and scalars equal the oracle's on the concatenation, every frame equals the oracle's
    tiled dither of that frame with the shared palette and params."""
    import test_gpu_frames as tf
    frames = mk()
    seeds = [2000 + 7 * i for i in range(len(frames))]
    if K > 2:
        oq, want_pal = tf._oracle_sequence(oracle, kind, frames, K)
    else:
        oq, want_pal = _oracle_palette(oracle, kind, np.concatenate([f.reshape(-1) for f in frames]).reshape(-1, 1), K)
    shared = oq.params
    d = tf._DevFrames(frames)
    q0 = _cls(nq, kind)(frames[0])
    got0 = nq.pnnquan_frames_device(q0, d.ptrs(d.buf), d.widths, d.heights, K)
    assert len(got0) == len(want_pal) and (got0 == want_pal).all()
    for f in (SCALARS if K > 2 else SCALARS_K2):
        want_f = len(want_pal) if f == "paletteLength" else getattr(shared, f)
        assert getattr(q0.params, f) == want_f, (f, getattr(q0.params, f), want_f)
    q = _cls(nq, kind)(frames[0], mode=TILED)
    pal = nq.convert_frames_device(q, d.ptrs(d.buf), d.widths, d.heights, K, dither, d.ptrs(d.out), d.ptrs(d.idx), seeds=seeds)
    assert len(pal) == len(want_pal) and (pal == want_pal).all()
    pal_h, imgs = nq.convert_frames(kind, frames, K, dither, seeds=seeds)
    assert len(pal_h) == len(want_pal) and (pal_h == want_pal).all()
    for i, f in enumerate(frames):
        want_argb, want_idx = tf._oracle_frame(oracle, nq, kind, f, K, shared, seeds[i], want_pal, dither, TILED)
        got_argb, got_idx = d.result(i)
        assert not _diff(got_argb, got_idx, want_argb, want_idx), "frame %d (device form): %s" % (i, _diff(got_argb, got_idx, want_argb, want_idx))
        assert not _diff(imgs[i].argb, imgs[i].index, want_argb, want_idx), "frame %d (host form)" % i
    assert d.guard_intact()


# ---------------------------------------------------------------------------------------------------------------------------------
# f. a last band of one row
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dither", [True, False])
@pytest.mark.parametrize("kind,H,tile", [(1, 65, (8, 8)), (1, 129, (8, 8)), (1, 129, None), (0, 65, (16, 16)), (0, 129, (4, 4))])
def test_last_band_of_one_row(nq, oracle, kind, H, tile, dither):
    """64x65 and 64x129 images with band starts every 64 rows: the last band is one row high (a one-row histogram partial, a band whose
    tiles are all 1 pixel high).  Compared with the oracle's banded restatement (nqo_set_bands)."""
    import test_gpu_banded as tb
    img = synth.gradient_noise(64, H, 600 + H + kind)
    starts = list(range(0, H, 64))
    assert H - starts[-1] == 1
    seed, K = 77, 256
    oq = oracle.OracleQuantizer(kind, img, seed=seed)
    oq.set_bands(starts)
    oq.prescan(K)
    want_pal = oq.pnnquan(K)
    want_argb, want_idx = oq.dither(want_pal, dither, tile=tile or (4, 4))
    pal, argb, idx, gparams = tb._bands_by_hand(nq, img, kind, K, dither, starts, seed, tile)
    assert len(pal) == len(want_pal) and (pal == want_pal).all(), "banded palette differs from the oracle's banded restatement"
    if kind == 1 and not dither and len(pal) > 32:
        assert gparams.distinctColors == oq.params.distinctColors, "image-wide distinct-colour count"
    assert not _diff(argb, idx, want_argb, want_idx), _diff(argb, idx, want_argb, want_idx)
