"""The prep stream of nq_convert_batch_device's finish phase (csrc/nq_abi.cpp finish_side_streams, dither_device):
image i's lists, Lab table, saliency map and counter clear run on a stream of their own beside the light pass of the images in front of
it, the scratch they fill rotates through S = min(4, n) sets, and the chain passes alternate over two side streams.  Only streams and
events differ from the serial order, so every palette, index map and ARGB output must be the oracle's bit for bit -- under the default,
under NQ_FINISH_PREP=0 (the lists on the launch stream again) and under every NQ_FINISH_SETS.

Setup: LAB, K = 256, dither = true, MODE_PARALLEL_TILED with 8x8 tiles.  The side streams are taken only by the split pixel form, and
convert() reaches that form only with GilbertCurve's DITHER_MAX 25, a weight = 256 / bins below 0.015: more than 17 067 occupied histogram
bins.  synth.gradient_noise of 96 x 64 to 160 x 128, the sizes first meant for this file, has 4 593 to 10 016 bins (13 757 at most with
more noise), weight 0.0256 to 0.0557: the generic kernel, no side work, an empty test.  So the images are synth.uniform_rgb of 508 x 42
and 516 x 44 (21 336 and 22 704 pixels), capped at 250 so that no tile is listed by accident: about the smallest that clear the threshold
with some margin (the builder asserts the weight), 384 and 390 tiles with partial ones at the right and bottom edges, and five of them are
the 516 x 44 fixtures the other dither files already compute.  Every case asserts through nq_get_dither_path and
the split statistics that each such image took the specialised kernel in the split form with its chain pass on a side stream, and
through the listed-tile count (the need count in d_failed, cleared on the prep stream) that the light pass listed what the oracle's
counters say; nq_get_list_counts shows the lists of every scratch set in use."""
import numpy as np
import pytest

from nquant.android_amd import synth

import test_gpu_dither_pixel as pixel
from test_gpu_dither_split import BATCH_SEED, BATCH_TILE, TILED, _cap250, _counters, _split_stats_of

pytestmark = pytest.mark.gpu

SMALL, BASE = (508, 42), (516, 44)           # 64 x 6 and 65 x 6 tiles, the right column 4 wide, the bottom row 2 / 4 high
_FIX = {}


def _oracle_convert(oracle, img, split=True):
    oq = oracle.OracleQuantizer(1, img, seed=BATCH_SEED)
    oq.prescan(256)
    pal = oq.pnnquan(256)
    if split:
        assert len(pal) == 256 and 0.0025 < oq.params.weight < 0.015, (img.shape, len(pal), oq.params.weight)
    _counters(oracle, reset=True)
    argb, idx = oq.dither(pal, True, tile=BATCH_TILE)
    cnt = _counters(oracle)
    assert not split or cnt[4] == 0, cnt
    return img, pal, argb, idx, int(cnt[6]), split


def _fixtures(oracle):
    """name -> (image, palette, ARGB, indices, tiles the light pass lists, takes the split form?), computed once and left unchanged.  The
    five 516 x 44 images of test_gpu_dither_pixel.py (shared with that file and test_gpu_dither_split.py: none and clean_b list no tile,
    one and one_corner one, all has a white pixel at step 0 of EVERY tile, so all 390 go to the chain pass; five palettes), one smaller
    clean image, and an image of 200 colours (k200: convert() returns them as the palette, weight 0.9, the generic kernel)"""
    if not _FIX:
        imgs, want = pixel._batch_images(oracle)
        for k, img in imgs.items():
            pal, argb, idx, direct = want[k]
            _FIX[k] = (img, pal, argb, idx, direct, True)
        assert _FIX["all"][4] == 390 and (_FIX["none"][4], _FIX["clean_b"][4], _FIX["one"][4]) == (0, 0, 1)
        _FIX["small"] = _oracle_convert(oracle, _cap250(synth.uniform_rgb(SMALL[0], SMALL[1], 410)))
        rng = np.random.default_rng(5)
        cols = rng.choice(1 << 24, 200, replace=False).astype(np.uint32) | np.uint32(0xFF000000)
        w, h = BASE
        _FIX["k200"] = _oracle_convert(oracle, _cap250(cols[rng.integers(0, 200, w * h)].view(np.int32).reshape(h, w)), split=False)
        assert len(_FIX["k200"][1]) == 200
    return _FIX


def _handles(nq, n):
    return [nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED, seed=BATCH_SEED, tile=BATCH_TILE) for _ in range(n)]


def _convert(nq, oracle, qs, names, sets_in_use=None):
    """one nq_convert_batch_device call of the named fixtures on the handles qs, checked against the oracle; returns the outputs"""
    import torch
    fix = _fixtures(oracle)
    for q, k in zip(qs, names):
        q.height, q.width = fix[k][0].shape
    d_in = [torch.from_numpy(np.ascontiguousarray(fix[k][0]).reshape(-1)).cuda() for k in names]
    outs = [torch.zeros_like(d) for d in d_in]
    idxs = [torch.zeros(d.numel(), dtype=torch.int16, device="cuda") for d in d_in]
    _split_stats_of()
    pals = nq.convert_batch_device(qs, [d.data_ptr() for d in d_in], 256, True, [o.data_ptr() for o in outs], [x.data_ptr() for x in idxs])
    torch.cuda.synchronize()
    n_split = sum(1 for k in names if fix[k][5])
    assert _split_stats_of() == (n_split, n_split, 0), "not the split form with the chain pass on a side stream"
    got = []
    for i, k in enumerate(names):
        img, pal, argb, idx, listed, split = fix[k]
        what = "image %d (%s)" % (i, k)
        assert len(pals[i]) == len(pal) and (pals[i] == pal).all(), what
        assert qs[i].dither_path() == ((1, 0) if split else (0, 0)), what
        assert _split_stats_of(qs[i]) == (0, 0, listed if split else 0), what
        g_idx, g_argb = idxs[i].cpu().numpy().astype(np.int32).reshape(idx.shape), outs[i].cpu().numpy().reshape(argb.shape)
        assert (g_idx == idx).all(), what + ": indices differ from the oracle"
        assert (g_argb == argb).all(), what + ": ARGB differs from the oracle"
        got.append((np.asarray(pals[i]).copy(), g_idx, g_argb))
    for k in range(sets_in_use or 0):             # (after the call a handle's own scratch is its set again)
        closest, nearest = qs[k].list_counts()
        assert closest.max() >= 1 and nearest.max() >= 1, "set %d holds no lists" % k
    return got


def _batch(nq, oracle, names, sets_in_use=None):
    qs = _handles(nq, len(names))
    try:
        return _convert(nq, oracle, qs, names, sets_in_use)
    finally:
        for q in qs:
            q.close()


NINE = ("none", "clean_b", "one", "all", "one_corner", "clean_b", "none", "all", "one")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
def test_batch_sizes_default_and_lists_on_the_launch_stream(nq, oracle, monkeypatch, n):
    """S = 1..4 and the sets' wrap-around (n = 5: set 0 once more, n = 9: every set twice and set 0 a third time); n = 1 keeps the order
    without a prep stream.  NQ_FINISH_PREP=0 must give the same outputs (both are compared with the oracle, and with each other)."""
    monkeypatch.delenv("NQ_FINISH_SETS", raising=False)
    monkeypatch.delenv("NQ_FINISH_PREP", raising=False)
    new = _batch(nq, oracle, NINE[:n], sets_in_use=min(4, n))
    monkeypatch.setenv("NQ_FINISH_PREP", "0")
    old = _batch(nq, oracle, NINE[:n], sets_in_use=min(2, n))
    for a, b in zip(new, old):
        assert all((x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("sets", ["2", "3", "4"])
def test_sets_override(nq, oracle, monkeypatch, sets):
    monkeypatch.setenv("NQ_FINISH_SETS", sets)
    _batch(nq, oracle, NINE, sets_in_use=int(sets))


@pytest.mark.parametrize("chains", ["1", "2"])
def test_chain_streams_override(nq, oracle, monkeypatch, chains):
    """NQ_FINISH_CHAIN_STREAMS: every chain pass on one side stream, or alternating over two; image 1 and 3 keep theirs busy"""
    monkeypatch.setenv("NQ_FINISH_CHAIN_STREAMS", chains)
    _batch(nq, oracle, ("none", "all", "clean_b", "all", "one", "all"), sets_in_use=4)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_sizes_change_inside_the_batch(nq, oracle, order):
    """ascending: sets 0..3 are first sized by four small images, and images 4, 5, 6 and 8 outgrow the saliency planes of sets 0, 1, 2
    and 0 while the side work of the images in front of them is in flight; descending: the reverse order, in which every set keeps its first
    size and the small images read a plane larger than they are"""
    names = ("small", "small", "small", "small", "none", "clean_b", "one", "small", "all")
    if order == "descending":
        names = names[::-1]
    _batch(nq, oracle, names, sets_in_use=4)


def test_every_second_image_has_long_side_work(nq, oracle):
    """all: a white pixel at step 0 of every tile, so every tile goes to the chain pass -- that image's side work is long, its
    neighbours have none, and the prep stream reaches the set of image i - 4 while image i - 3's chain pass may still run"""
    _batch(nq, oracle, ("none", "all", "clean_b", "all", "none", "all", "clean_b", "all", "none"), sets_in_use=4)
    _batch(nq, oracle, ("all", "none", "all", "clean_b", "all", "none"), sets_in_use=4)


@pytest.mark.parametrize("at", [0, 2, 5])
def test_one_palette_of_200(nq, oracle, at):
    """one image of 200 colours among K = 256 ones: its palette needs no merge loop, so it is uploaded in the finish phase (the prep stream
    starts behind the copy), its lists sit between those of 256-entry palettes, and its own pass is the generic kernel on the launch stream
    -- whose end the prep stream of image i + 4 waits for"""
    names = ["none", "clean_b", "one", "all", "one_corner", "clean_b", "none"]
    names[at] = "k200"
    _batch(nq, oracle, names, sets_in_use=4)


def test_same_handles_again_and_permuted(nq, oracle):
    """sets, streams and events of the handles reused across calls: the same batch twice, then the images in another order (every handle
    meets another image, of another size where the names say so)"""
    names = ("none", "all", "small", "clean_b", "small", "one")
    qs = _handles(nq, len(names))
    try:
        first = _convert(nq, oracle, qs, names, sets_in_use=4)
        again = _convert(nq, oracle, qs, names, sets_in_use=4)
        for a, b in zip(first, again):
            assert all((x == y).all() for x, y in zip(a, b))
        _convert(nq, oracle, qs, ("small", "one", "none", "small", "all", "clean_b"), sets_in_use=4)
    finally:
        for q in qs:
            q.close()
