"""The per-image plumbing of nq_convert_batch_device, bit for bit against the CPU oracle (palette, indices, ARGB; no tolerances).

What moved, and where it is held here:
  1. the packed list records of the specialised kernels are written by the LAB list builders themselves (NQ_PACK_IN_BUILDERS=0 restores
     the separate pack launch): both forms, on 1 and 4 lanes, must give the oracle's result -- on a batch with an image that runs the
     specialised dither kernel, the reader of those records;
  2. the hand-back count of the specialised dither kernel is cleared by the builders' launch in front of it: an image that hands tiles
     back followed by one that does not, and the reverse -- on one lane of a batch, and on ONE handle (the count's buffer belongs to the
     handle) -- must both be exact, the second with the count it really has;
  3. the pre-scan's two scalars land in page-locked slots of the handle, and the scan kernel of the 16-byte path clears the histogram's
     bin counters: the only transparent pixel first, last and in the last workgroup of the scan, twice in a row on one handle;
  4. every palette of a batch comes back in one block: a batch that mixes merge jobs with an image that has none, against single
     converts, and a second time on the same handles;
  5. palettes of fewer than 256 entries (K = 64, K = 255): builder-written records of shorter lists under the specialised kernel, and
     read-back slots whose palette part is shorter than 256 words and of odd length."""
import numpy as np
import pytest

from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

TILED = 1
TILE = (8, 8)
_WANT = {}


def _oracle(key, img, rng_seed, K):
    """The oracle's convert(K, true) of a LAB quantizer, tiled: (palette, indices, ARGB, transparentPixelIndex, transparentColor);
    computed once per key for the module."""
    if key not in _WANT:
        import oracle_lib
        oq = oracle_lib.OracleQuantizer(1, img, seed=rng_seed)
        oq.prescan(K)
        pal = oq.pnnquan(K)
        p = oq.params
        scan = (p.transparentPixelIndex, p.transparentColor)
        oq.set_seed(rng_seed)
        h, w = img.shape
        argb, idx = oq.dither(pal, True, tile=(min(TILE[0], w), min(TILE[1], h)))
        oq.close()
        _WANT[key] = (pal, idx.astype(np.uint16).reshape(-1), argb.reshape(-1)) + scan
    return _WANT[key]


def _quantizers(nq, imgs, seeds):
    qs = [nq.PnnLABQuantizer(np.zeros((1, 1), np.int32), mode=TILED, seed=s, tile=TILE) for s in seeds]
    for q, im in zip(qs, imgs):
        q.height, q.width = im.shape
    return qs


def _batch(nq, qs, imgs, K):
    """One nq_convert_batch_device of imgs on qs: [(palette, indices, ARGB)] per image."""
    import torch
    d_in = [torch.from_numpy(np.ascontiguousarray(im).reshape(-1)).cuda() for im in imgs]
    d_out = [torch.full_like(d, 0x5A5A5A5A) for d in d_in]
    d_idx = [torch.full((d.numel(),), 0x5A5A, dtype=torch.int16, device="cuda") for d in d_in]
    pals = nq.convert_batch_device(qs, [d.data_ptr() for d in d_in], K, True, [d.data_ptr() for d in d_out], [d.data_ptr() for d in d_idx])
    torch.cuda.synchronize()
    return [(pals[i], d_idx[i].cpu().numpy().view(np.uint16), d_out[i].cpu().numpy()) for i in range(len(imgs))]


def _single(q, img, K, seed=None):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
    d_out = torch.full_like(d_in, 0x5A5A5A5A)
    d_idx = torch.full((d_in.numel(),), 0x5A5A, dtype=torch.int16, device="cuda")
    pal = q.convert_device(d_in.data_ptr(), K, True, d_out.data_ptr(), d_idx.data_ptr(), seed=seed)
    torch.cuda.synchronize()
    return pal, d_idx.cpu().numpy().view(np.uint16), d_out.cpu().numpy()


def _same(got, want, what):
    pal, idx, argb = want[:3]
    assert len(got[0]) == len(pal), "%s: palette length %d, oracle %d" % (what, len(got[0]), len(pal))
    assert (got[0] == pal).all(), "%s: %d palette entries differ" % (what, int((got[0] != pal).sum()))
    assert got[1].shape == idx.shape and (got[1] == idx).all(), "%s: %d indices differ" % (what, int((got[1] != idx).sum()))
    assert (got[2] == argb).all(), "%s: %d ARGB pixels differ" % (what, int((got[2] != argb).sum()))


def _close(qs):
    for q in qs:
        q.close()


# ---- 1. lanes x pack form ---------------------------------------------------------------------------------------------------------------
SIZES = [(96, 64), (64, 96), (130, 70), (256, 256), (130, 70), (96, 64)]       # (130 x 70: no multiple of 4 or of the tile)
FAST_AT = 2         # where the image that runs the specialised kernel goes into the batch


def test_lanes_and_pack_forms_give_the_oracle(nq, oracle, monkeypatch):
    """Six gradient_noise images, K = 256, dither on; NQ_BATCH_LANES 1 / 4 x NQ_PACK_IN_BUILDERS 0 / 1: four runs, each the oracle's
    result (hence identical).  Those six have 4 600 to 15 100 histogram bins, a weight above .015, and take the generic dither kernel,
    which reads the byte lists; the packed records are read by the specialised kernel only, so a seventh image -- 192 x 160 uniform
    noise, 24 500 bins -- sits in the middle of the batch and must report that kernel in every run."""
    imgs = [synth.gradient_noise(w, h, 900 + i) for i, (w, h) in enumerate(SIZES)]
    seeds = [40 + i for i in range(len(imgs))]
    want = [_oracle(("lanes", i), imgs[i], seeds[i], 256) for i in range(len(imgs))]
    imgs.insert(FAST_AT, synth.uniform_rgb(192, 160, 137))
    seeds.insert(FAST_AT, 62)
    want.insert(FAST_AT, _oracle(("handback", "opaque"), imgs[FAST_AT], 62, 256))       # (shared with the hand-back test below)
    runs = {}
    for lanes in (1, 4):
        for pack in (0, 1):
            monkeypatch.setenv("NQ_BATCH_LANES", str(lanes))
            monkeypatch.setenv("NQ_PACK_IN_BUILDERS", str(pack))
            qs = _quantizers(nq, imgs, seeds)
            runs[lanes, pack] = got = _batch(nq, qs, imgs, 256)
            paths = [q.dither_path() for q in qs]
            _close(qs)
            assert paths[FAST_AT] == (1, 0), "lanes %d, pack in builders %d: the image meant for the specialised kernel ran %s" % (lanes, pack, paths[FAST_AT])
            for i in range(len(imgs)):
                _same(got[i], want[i], "lanes %d, pack in builders %d, image %d" % (lanes, pack, i))
    first = runs[1, 0]
    for key, got in runs.items():
        for a, b in zip(first, got):
            assert all((x == y).all() for x, y in zip(a, b)), key


# ---- 2. hand-back count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_first", [True, False])
def test_hand_back_count_follows_each_image(nq, oracle, monkeypatch, alpha_first):
    """One lane: an image with alpha == 0 pixels (no semi-transparency), whose tiles with such pixels the specialised dither kernel hands
    back to the generic one, next to a fully opaque image, in both orders.  Both are 192 x 160 uniform noise: about 20 000 and 24 500
    histogram bins, the smallest images whose weight (256 / bins < .015) selects the specialised kernel's configuration -- the oracle's
    merge loop over those bins is most of this test's time.  Both must be exact and report the specialised kernel, the opaque one with no
    tile handed back.  The count lives in a buffer of the HANDLE, so the handle that ran the first image then converts the second one
    alone: behind the image with hand-backs the opaque one must report none (a count that is not cleared would still hold the first
    image's), behind the opaque one the other must report exactly what it reported on its own handle."""
    monkeypatch.setenv("NQ_BATCH_LANES", "1")
    monkeypatch.delenv("NQ_PACK_IN_BUILDERS", raising=False)
    alpha = synth.with_alpha(synth.uniform_rgb(192, 160, 501), 501, p_semi=0.0)
    opaque = synth.uniform_rgb(192, 160, 137)
    assert (((alpha.view(np.uint32) >> 24) == 0).sum()) > 0 and (((alpha.view(np.uint32) >> 24) % 255) == 0).all()
    pair = [("alpha", alpha, 61), ("opaque", opaque, 62)]
    if not alpha_first:
        pair.reverse()
    imgs, seeds = [p[1] for p in pair], [p[2] for p in pair]
    want = [_oracle(("handback", p[0]), p[1], p[2], 256) for p in pair]
    qs = _quantizers(nq, imgs, seeds)
    got = _batch(nq, qs, imgs, 256)
    for i, p in enumerate(pair):
        _same(got[i], want[i], "%s image (alpha first: %s)" % (p[0], alpha_first))
        ran_fast, back = qs[i].dither_path()
        print("%s: specialised kernel %d, tiles handed back %d" % (p[0], ran_fast, back))
        assert ran_fast == 1, "%s image: the generic kernel ran" % p[0]
        if p[0] == "opaque":
            assert back == 0, "opaque image: %d tiles handed back (a stale count)" % back
        else:
            assert back > 0, "the image with transparent pixels handed no tile back: the case does not test the count"
    alpha_back = qs[0 if alpha_first else 1].dither_path()[1]
    # the same two images in the same order on ONE handle: handle 0 has just run pair[0]
    got2 = _single(qs[0], imgs[1], 256, seed=seeds[1])
    _same(got2, want[1], "%s image behind the %s image on one handle" % (pair[1][0], pair[0][0]))
    assert qs[0].dither_path() == (1, 0 if alpha_first else alpha_back), (alpha_first, qs[0].dither_path(), alpha_back)
    # ... and back again: three passes on the handle, alternating
    got3 = _single(qs[0], imgs[0], 256, seed=seeds[0])
    _same(got3, want[0], "%s image again on that handle" % pair[0][0])
    assert qs[0].dither_path() == (1, alpha_back if alpha_first else 0), (alpha_first, qs[0].dither_path(), alpha_back)
    _close(qs)


# ---- 3. scan ----------------------------------------------------------------------------------------------------------------------------
def _one_transparent(w, h, seed, pos):
    img = synth.gradient_noise(w, h, seed).copy()
    flat = img.reshape(-1).view(np.uint32)
    flat[pos] &= np.uint32(0x00FFFFFF)
    return img


SCAN_CASES = [(1, 1, 0), (3, 5, 0), (3, 5, 14), (3, 5, 9), (4096, 1, 0), (4096, 1, 4095), (4096, 1, 4096 - 100)]


@pytest.mark.parametrize("w,h,pos", SCAN_CASES)
def test_scan_reports_the_transparent_pixel(nq, oracle, w, h, pos):
    """The only transparent pixel first, last, and in the last workgroup of the scan (4096 x 1: four workgroups of the 16-byte scan;
    1 x 1 and 3 x 5: the one-pixel-per-thread scan): transparentPixelIndex and m_transparentColor equal the oracle's, and so does the
    whole convert -- twice in a row on one handle (the second convert finds the slots and counters the first one left)."""
    img = _one_transparent(w, h, 700 + w, pos)
    want = _oracle(("scan", w, h, pos), img, 9, 256)
    assert want[3] == pos
    qs = _quantizers(nq, [img], [9])
    for rnd in range(2):
        got = _single(qs[0], img, 256)
        p = qs[0].params
        assert (p.transparentPixelIndex, p.transparentColor) == (want[3], want[4]), (rnd, p.transparentPixelIndex, p.transparentColor, want[3:])
        _same(got, want, "%dx%d, transparent pixel %d, convert %d" % (w, h, pos, rnd))
    _close(qs)


# ---- 4. batched read-back ---------------------------------------------------------------------------------------------------------------
def test_batched_read_back_with_a_hole(nq, oracle, monkeypatch):
    """Merge jobs around a 40-colour image that has none (its palette is final before the merge launch): palettes and lengths per image
    equal single converts on fresh handles and the oracle; a second batch on the same handles gives the same again."""
    monkeypatch.delenv("NQ_BATCH_LANES", raising=False)
    monkeypatch.delenv("NQ_PACK_IN_BUILDERS", raising=False)
    imgs = [synth.gradient_noise(96, 64, 811), synth.few_colors(64, 64, 812, 40), synth.gradient_noise(130, 70, 813),
            synth.gradient_noise(64, 96, 814)]
    seeds = [71, 72, 73, 74]
    want = [_oracle(("hole", i), imgs[i], seeds[i], 256) for i in range(len(imgs))]
    assert len(want[1][0]) == 40
    qs = _quantizers(nq, imgs, seeds)
    first = _batch(nq, qs, imgs, 256)
    second = _batch(nq, qs, imgs, 256)
    assert [q.merge_variant()[0] for q in qs] == [512, 0, 512, 512]
    for i in range(len(imgs)):
        _same(first[i], want[i], "first batch, image %d" % i)
        _same(second[i], want[i], "second batch, image %d" % i)
        fresh = _quantizers(nq, [imgs[i]], [seeds[i]])
        alone = _single(fresh[0], imgs[i], 256)
        _close(fresh)
        assert len(alone[0]) == len(first[i][0]) and (alone[0] == first[i][0]).all(), i
        assert (alone[1] == first[i][1]).all() and (alone[2] == first[i][2]).all(), i
    # the handles know what their device palettes hold: a convert alone on a handle of the batch is exact as well
    _same(_single(qs[2], imgs[2], 256), want[2], "handle 2 alone after the batches")
    _close(qs)


# ---- 5. palettes below 256 entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 255])
def test_smaller_palettes(nq, oracle, monkeypatch, K):
    monkeypatch.delenv("NQ_BATCH_LANES", raising=False)
    monkeypatch.delenv("NQ_PACK_IN_BUILDERS", raising=False)
    imgs = [synth.uniform_rgb(192, 160, 137), synth.gradient_noise(130, 70, 821)]
    seeds = [81, 82]
    want = [_oracle(("small", K, i), imgs[i], seeds[i], K) for i in range(2)]
    qs = _quantizers(nq, imgs, seeds)
    got = _batch(nq, qs, imgs, K)
    for i in range(2):
        assert len(got[i][0]) == K
        _same(got[i], want[i], "K = %d, image %d" % (K, i))
    _close(qs)
