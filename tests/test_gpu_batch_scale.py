"""nq_convert_batch_device against the CPU oracle at every batch-size regime, bit for bit (no tolerances anywhere).

What a batch does differently from a single convert, and where each difference is held here:
  1. the merge kernel variant follows the number of merge jobs of the call (csrc/nq_kernels.hip merge_threads_for /
     merge_team_helpers): prefixes of ONE seeded list of 4C + 1 images are run unforced at 3, 60, C/2, C, C + 1, 2C + 1 and 4C + 1 jobs
     (C = compute units), the variant that ran is read back (nq_get_merge_variant) and compared with the rule restated below, and
     EVERY image of every batch is compared with the oracle;
  2. the stages in front of the merge loops run on 1..8 lanes (NQ_BATCH_LANES), lane k sharing the scratch of handle k;
  3. that scratch has to grow inside a lane, and again in a later call on the same handles;
  4. LAB and RGB jobs are sorted into two launches out of one job table, images without a merge job leave holes in it;
  5. a failure in the middle of a batch leaves every handle usable.
The oracle runs in a spawn pool of oracle-only workers (no GPU state in them); its results are cached for the module."""
import ctypes as C
import multiprocessing as mp
import time

import numpy as np
import pytest

from nquant.android_amd import synth

pytestmark = pytest.mark.gpu

TILED = 1
K = 256
TILE = (8, 8)
ORACLE_WORKERS = 12
PARAM_FIELDS = ("hasSemiTransparency", "transparentPixelIndex", "transparentColor", "maxbins", "quan_rt", "isNano", "texicab",
                "paletteLength", "PR", "PG", "PB", "PA", "ratio", "weight")
T0 = time.time()


# ---- images: a description (kind, generator, width, height, image seed, alpha, colours) is all a worker needs ---------------------
def _make(desc):
    kind, gen, w, h, seed, alpha, ncolors = desc
    if gen == "gradient":
        img = synth.gradient_noise(w, h, seed)
    elif gen == "uniform":
        img = synth.uniform_rgb(w, h, seed)
    elif gen == "few":
        img = synth.few_colors(w, h, seed, ncolors)
    else:
        raise ValueError(gen)
    return synth.with_alpha(img, seed) if alpha else img


def _oracle_one(item):
    """(key, description, random seed) -> the oracle's convert(256, true), tiled 8x8: palette, indices, ARGB, scalars."""
    import oracle_lib
    key, desc, rng_seed = item
    img = _make(desc)
    oq = oracle_lib.OracleQuantizer(desc[0], img, seed=rng_seed)
    oq.prescan(K)
    pal = oq.pnnquan(K)
    params = {f: getattr(oq.params, f) for f in PARAM_FIELDS + ("distinctColors",)}
    params["paletteLength"] = len(pal)      # (the oracle leaves the field unset on the few-colours early return: the length itself is the reference)
    oq.set_seed(rng_seed)
    argb, idx = oq.dither(pal, True, tile=TILE)
    oq.close()
    return key, (pal, idx.astype(np.uint16).reshape(-1), argb.reshape(-1), params)


_WANT = {}


def _want(items):
    """Oracle results of `items` ((key, description, random seed) triples), computed once per key for the whole module."""
    todo = [it for it in items if it[0] not in _WANT]
    if len(todo) > 4:
        ctx = mp.get_context("spawn")       # the workers only run the CPU oracle: fresh interpreters, no GPU state
        with ctx.Pool(min(ORACLE_WORKERS, len(todo))) as pool:
            for key, res in pool.imap_unordered(_oracle_one, todo, chunksize=4):
                _WANT[key] = res
    else:
        for it in todo:
            _WANT[it[0]] = _oracle_one(it)[1]
    return [_WANT[it[0]] for it in items]


# ---- GPU side -------------------------------------------------------------------------------------------------------------------
class _Batch:
    """Quantizer objects, resident inputs and outputs of a list of (key, description, random seed) items."""

    def __init__(self, nq, items, qs=None):
        import torch
        self.nq, self.items = nq, items
        cls = {0: nq.PnnQuantizer, 1: nq.PnnLABQuantizer}
        self.imgs = [_make(desc) for _, desc, _ in items]
        self.qs = qs if qs is not None else [cls[desc[0]](np.zeros((1, 1), np.int32), mode=TILED, seed=s, tile=TILE) for _, desc, s in items]
        for q, im, (_, desc, s) in zip(self.qs, self.imgs, items):
            assert q.KIND == desc[0]
            q.height, q.width = im.shape
            q.seed = s
        self.d_in = [torch.from_numpy(np.ascontiguousarray(im).reshape(-1)).cuda() for im in self.imgs]
        self.clear()

    def clear(self):
        import torch
        self.d_out = [torch.full_like(d, 0x5A5A5A5A) for d in self.d_in]
        self.d_idx = [torch.full((d.numel(),), 0x5A5A, dtype=torch.int16, device="cuda") for d in self.d_in]

    def run(self, sel=None):
        """One nq_convert_batch_device over the images `sel` (default: all); returns their palettes."""
        import torch
        sel = list(range(len(self.qs))) if sel is None else list(sel)
        pals = self.nq.convert_batch_device([self.qs[i] for i in sel], [self.d_in[i].data_ptr() for i in sel], K, True,
                                            [self.d_out[i].data_ptr() for i in sel], [self.d_idx[i].data_ptr() for i in sel])
        torch.cuda.synchronize()
        return pals

    def single(self, i, q=None):
        """nq_convert_device of image i alone, on its own quantizer or on `q`; returns (palette, indices, ARGB)."""
        import torch
        q = self.qs[i] if q is None else q
        out = torch.full_like(self.d_in[i], 0x5A5A5A5A)
        idx = torch.full((self.d_in[i].numel(),), 0x5A5A, dtype=torch.int16, device="cuda")
        pal = q.convert_device(self.d_in[i].data_ptr(), K, True, out.data_ptr(), idx.data_ptr())
        torch.cuda.synchronize()
        return pal, idx.cpu().numpy().view(np.uint16), out.cpu().numpy()

    def result(self, i):
        return self.d_idx[i].cpu().numpy().view(np.uint16), self.d_out[i].cpu().numpy()


def _same(got_pal, got_idx, got_argb, want, what, params=None):
    pal, idx, argb, wparams = want
    assert len(got_pal) == len(pal), "%s: palette length %d, oracle %d" % (what, len(got_pal), len(pal))
    assert (got_pal == pal).all(), "%s: %d palette entries differ" % (what, int((got_pal != pal).sum()))
    assert got_idx.shape == idx.shape and (got_idx == idx).all(), "%s: %d indices differ" % (what, int((got_idx != idx).sum()))
    assert (got_argb == argb).all(), "%s: %d ARGB pixels differ" % (what, int((got_argb != argb).sum()))
    if params is not None:
        for f in PARAM_FIELDS:
            assert getattr(params, f) == wparams[f], "%s: %s is %r, oracle %r" % (what, f, getattr(params, f), wparams[f])


def _check_batch(b, pals, want, sel=None, what="image"):
    sel = list(range(len(b.qs))) if sel is None else list(sel)
    for j, i in enumerate(sel):
        idx, argb = b.result(i)
        _same(pals[j], idx, argb, want[i], "%s %d (%s)" % (what, i, b.items[i][0]), b.qs[i].params)


# ---- the rule of csrc/nq_kernels.hip, restated ------------------------------------------------------------------------------------
def _rule(n_lab, n_rgb, cus):
    """(threads code, helpers of the LAB launch, helpers of the RGB launch): the thread count comes from the TOTAL number of merge
    jobs, the helper count from each kind's own number padded to 8 team slots, one 512-thread workgroup per compute unit."""
    n = n_lab + n_rgb
    threads = 512 if n <= cus else 256 if n <= 2 * cus else 128 if n <= 4 * cus else 127

    def helpers(n_kind):
        if n_kind <= 0 or threads != 512:
            return 0
        return max(0, min(7, cus // ((n_kind + 7) // 8 * 8) - 1))
    return threads, helpers(n_lab), helpers(n_rgb)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. every regime, unforced ----------------------------------------------------------------------------------------------------
SHAPES = [(64, 48), (48, 64), (80, 64), (64, 80), (96, 80), (80, 96), (72, 56)]
GENS = [("gradient", False), ("uniform", False), ("gradient", True), ("uniform", True)]


def _scale_item(i):
    """Image i of the seeded list: two thirds LAB and one third RGB, interleaved; generator, shape and kind cycle with the coprime
    periods 4, 7 and 3; its own image seed and random seed."""
    kind = 0 if i % 3 == 2 else 1
    gen, alpha = GENS[i % 4]
    w, h = SHAPES[i % 7]
    return ("scale%d" % i, (kind, gen, w, h, 10007 + 31 * i, alpha, 0), 5000 + i)


_SCALE = {}


@pytest.fixture(scope="module")
def scale(nq):
    """The 4C + 1 quantizer objects and resident images, shared by the prefixes (the same handles run batch after batch)."""
    cus = _cus()
    assert cus >= 64, "the batch sizes of this module assume at least 64 compute units"
    items = [_scale_item(i) for i in range(4 * cus + 1)]
    b = _Batch(nq, items)
    yield cus, b
    for q in b.qs:
        q.close()


ROWS = ["3", "60", "C/2", "C", "C+1", "2C+1", "4C+1"]


def _row_n(row, cus):
    return {"3": 3, "60": 60, "C/2": cus // 2, "C": cus, "C+1": cus + 1, "2C+1": 2 * cus + 1, "4C+1": 4 * cus + 1}[row]


@pytest.mark.parametrize("row", ROWS)
def test_every_regime_unforced_equals_the_oracle(nq, oracle, scale, monkeypatch, row):
    """A prefix of the seeded list as one batch, nothing forced: the merge launch must pick the variant the rule gives for the number
    of MERGE JOBS (512 threads up to C jobs -- with 7, 5, 1 and 0 helpers per LAB loop at 3, 60, C/2 and C jobs on 256 compute units --
    then 256, 128 and the dense variant 127), and every image of the batch must equal the oracle: palette, indices, ARGB, scalars."""
    for v in ("NQ_MERGE_THREADS", "NQ_MERGE_HELPERS", "NQ_BATCH_LANES"):
        monkeypatch.delenv(v, raising=False)
    cus, b = scale
    n = _row_n(row, cus)
    sel = range(n)
    want_all = _want(b.items[:n])
    want = dict(enumerate(want_all))
    for i in sel:                                       # n_in_flight counts merge jobs: every image of this list must make one
        assert want[i][3]["maxbins"] > K, "image %d has only %d bins" % (i, want[i][3]["maxbins"])
    b.clear()
    t = time.time()
    pals = b.run(sel)
    gpu_s = time.time() - t
    n_rgb = sum(1 for i in sel if b.items[i][1][0] == 0)
    n_lab = n - n_rgb
    threads, h_lab, h_rgb = _rule(n_lab, n_rgb, cus)
    lab = [i for i in sel if b.items[i][1][0] == 1]
    rgb = [i for i in sel if b.items[i][1][0] == 0]
    got = (b.qs[lab[0]].merge_variant()[0], b.qs[lab[0]].merge_variant()[1], b.qs[rgb[0]].merge_variant()[1])
    print("batch of %d (%d LAB + %d RGB merge jobs, %d CUs): (threads, helpers_lab, helpers_rgb) = %s, batch call %.2f s, phases %s, "
          "module clock %.0f s" % (n, n_lab, n_rgb, cus, got, gpu_s, b.qs[0].batch_phase_ms(), time.time() - T0))
    for i in (0, n - 1, lab[0], lab[-1], rgb[0], rgb[-1]):                # first, last, LAB and RGB handles
        kind = b.items[i][1][0]
        assert b.qs[i].merge_variant() == (threads, h_lab if kind else h_rgb), (i, kind, b.qs[i].merge_variant(), (threads, h_lab, h_rgb))
    if threads == 512:
        assert b.qs[lab[0]].team_stats()["helpers"] == h_lab and b.qs[rgb[0]].team_stats()["helpers"] == h_rgb
    want_threads = {"3": 512, "60": 512, "C/2": 512, "C": 512, "C+1": 256, "2C+1": 128, "4C+1": 127}[row]
    assert threads == want_threads and got[0] == want_threads
    if cus == 256:      # worked out by hand from the rule: a reshuffled list must not quietly lose these team sizes
        assert (h_lab, h_rgb) == {"3": (7, 7), "60": (5, 7), "C/2": (1, 4), "C": (0, 1)}.get(row, (0, 0)), (row, h_lab, h_rgb)
    if row == "C":
        assert h_lab == 0 and h_rgb > 0, "at C jobs the larger kind runs without helpers, the smaller one keeps a team"
    _check_batch(b, pals, want, sel)


def test_largest_batch_equals_single_converts_on_fresh_handles(nq, oracle, scale, monkeypatch):
    """The 4C + 1 batch image by image against one nq_convert_device on a FRESH handle (own stream, own scratch, all stage events): every
    16th image plus the first and last image of each of the four lanes.  Afterwards handles of the batch -- the first, one behind the
    sixteenth (they record only three stage events inside a batch) and the last -- convert alone again, with the oracle's result and
    all eight stage times."""
    for v in ("NQ_MERGE_THREADS", "NQ_MERGE_HELPERS", "NQ_BATCH_LANES"):
        monkeypatch.delenv(v, raising=False)
    cus, b = scale
    n = 4 * cus + 1
    want = _want(b.items[:n])
    b.clear()
    pals = b.run(range(n))
    assert b.qs[n - 1].stage_ms()["merge"] == -1.0 and b.qs[0].stage_ms()["merge"] >= 0     # (light events from handle 16 on)
    subset = sorted(set(range(0, n, 16)) | {0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1})
    assert len(subset) >= 64
    cls = {0: nq.PnnQuantizer, 1: nq.PnnLABQuantizer}
    for i in subset:
        _, desc, s = b.items[i]
        q = cls[desc[0]](np.zeros((1, 1), np.int32), mode=TILED, seed=s, tile=TILE)
        q.height, q.width = b.imgs[i].shape
        pal, idx, argb = b.single(i, q)
        assert q.merge_variant() == (512, 7)             # one job on >= 64 compute units: 512 threads, 7 helpers
        q.close()
        got_idx, got_argb = b.result(i)
        assert len(pal) == len(pals[i]) and (pal == pals[i]).all(), i
        assert (idx == got_idx).all() and (argb == got_argb).all(), i
        _same(pal, idx, argb, want[i], "single convert of image %d" % i)
    for i in (0, 17, n - 1):
        pal, idx, argb = b.single(i)
        _same(pal, idx, argb, want[i], "handle %d alone after the batch" % i, b.qs[i].params)
        ms = b.qs[i].stage_ms()
        assert all(v >= 0 for v in ms.values()) and ms["total"] > 0, (i, ms)


# ---- 2. lanes -----------------------------------------------------------------------------------------------------------------------
def _lane_items():
    descs = [(1, "gradient", 96, 80, 211, False, 0), (0, "uniform", 64, 48, 212, False, 0), (1, "gradient", 80, 120, 213, True, 0),
             (1, "few", 64, 64, 214, False, 100), (0, "gradient", 128, 64, 215, False, 0), (1, "uniform", 72, 72, 216, False, 0),
             (0, "gradient", 48, 40, 217, False, 0), (1, "gradient", 144, 112, 218, False, 0), (1, "uniform", 56, 88, 219, False, 0),
             (0, "uniform", 88, 56, 220, False, 0), (1, "gradient", 64, 48, 221, False, 0)]
    return [("lane%d" % i, d, 300 + i) for i, d in enumerate(descs)]


@pytest.mark.parametrize("lanes,count", [(1, 11), (2, 11), (3, 11), (5, 11), (8, 11), (8, 3)])
def test_lane_counts_give_the_same_batch(nq, oracle, monkeypatch, lanes, count):
    """NQ_BATCH_LANES = 1, 2, 3, 5, 8 on 11 mixed images (n not a multiple of L; kinds, sizes, alpha, a few-colours early return) and
    8 lanes on 3 images (n < L): every lane count gives the oracle's result -- hence the same one --, and each handle then converts
    its image alone with that result again."""
    monkeypatch.setenv("NQ_BATCH_LANES", str(lanes))
    items = _lane_items()[:count]
    want = _want(items)
    if count > 3:                                        # the few-colours image takes the early return: no merge job
        assert want[3][3]["maxbins"] <= K and 0 < want[3][3]["distinctColors"] <= K
    b = _Batch(nq, items)
    pals = b.run()
    _check_batch(b, pals, want, what="%d lanes, image" % lanes)
    n_jobs = sum(1 for w in want if w[3]["maxbins"] > K)
    cus = _cus()
    n_lab = sum(1 for it, w in zip(items, want) if w[3]["maxbins"] > K and it[1][0] == 1)
    threads, h_lab, h_rgb = _rule(n_lab, n_jobs - n_lab, cus)
    for i, (it, w) in enumerate(zip(items, want)):
        exp = (threads, h_lab if it[1][0] else h_rgb) if w[3]["maxbins"] > K else (0, 0)
        assert b.qs[i].merge_variant() == exp, (i, b.qs[i].merge_variant(), exp)
    monkeypatch.delenv("NQ_BATCH_LANES")
    for i in range(count):
        pal, idx, argb = b.single(i)
        _same(pal, idx, argb, want[i], "handle %d alone after %d lanes" % (i, lanes), b.qs[i].params)
    for q in b.qs:
        q.close()


# ---- 3. scratch that grows inside a lane ---------------------------------------------------------------------------------------------
GROW = [(48, 40), (64, 48), (96, 80), (128, 96), (192, 160), (256, 200)]


def _grow_items(kinds, tag, sizes, seed0):
    return [("%s%d" % (tag, i), (kinds[i % len(kinds)], "gradient", w, h, seed0 + i, i % 4 == 3, 0), 400 + seed0 + i) for i, (w, h) in enumerate(sizes)]


@pytest.mark.parametrize("kinds", [(1,), (0,), (1, 0, 0, 1, 1, 0)], ids=["lab", "rgb", "mixed"])
def test_scratch_grows_along_each_lane(nq, oracle, monkeypatch, kinds):
    """Two lanes, image sizes growing along each lane (lane 0: 48x40, 96x80, 192x160; lane 1: 64x48, 128x96, 256x200): the lane's
    shared per-pixel scratch is freed and allocated again from the lane's thread while the other lane keeps launching."""
    monkeypatch.setenv("NQ_BATCH_LANES", "2")
    items = _grow_items(kinds, "grow" + "".join(map(str, kinds)) + "_", GROW, 600)
    want = _want(items)
    b = _Batch(nq, items)
    _check_batch(b, b.run(), want)
    for q in b.qs:
        q.close()


def test_scratch_regrows_in_a_second_batch_on_the_same_handles(nq, oracle, monkeypatch):
    """A first batch sizes the scratch of both lanes and the per-handle buffers; the second batch on the SAME handles brings a small
    image and then a much larger one to each lane (lane 0: 48x40 then 256x200), so reused buffers are regrown in mid-call."""
    monkeypatch.setenv("NQ_BATCH_LANES", "2")
    kinds = (1, 0, 1, 0)
    first = _grow_items(kinds, "regrowA", [(64, 48), (48, 40), (96, 80), (64, 64)], 700)
    second = _grow_items(kinds, "regrowB", [(48, 40), (64, 48), (256, 200), (192, 160)], 720)
    want_a, want_b = _want(first), _want(second)
    a = _Batch(nq, first)
    _check_batch(a, a.run(), want_a, what="first batch, image")
    b = _Batch(nq, second, qs=a.qs)
    _check_batch(b, b.run(), want_b, what="second batch, image")
    a2 = _Batch(nq, first, qs=a.qs)                      # and the small batch once more on the grown buffers
    _check_batch(a2, a2.run(), want_a, what="first batch again, image")
    for q in a.qs:
        q.close()


# ---- 4. mixed kinds and early returns in the job table -------------------------------------------------------------------------------
def _table_items():
    items = []
    for i in range(12):
        w, h = SHAPES[i % 7]
        items.append(("tabL%d" % i, (1, GENS[i % 4][0], w, h, 800 + i, GENS[i % 4][1], 0), 900 + i))
    for i in range(9):
        w, h = SHAPES[(i + 3) % 7]
        items.append(("tabR%d" % i, (0, GENS[(i + 1) % 4][0], w, h, 830 + i, GENS[(i + 1) % 4][1], 0), 930 + i))
    for i in range(9):
        w, h = SHAPES[(i + 5) % 7]
        items.append(("tabF%d" % i, (1, "few", w, h, 860 + i, False, 40 + 24 * i), 960 + i))
    return items


def _orders():
    lab, rgb, few = list(range(12)), list(range(12, 21)), list(range(21, 30))
    alt = []
    for j in range(12):
        alt += [lab[j]] + ([rgb[j]] if j < 9 else []) + ([few[j]] if j < 9 else [])
    return {"lab_first": lab + few + rgb, "rgb_first": rgb + lab + few, "alternating": alt,
            "few_first_and_last": few[:5] + rgb[:4] + lab + rgb[4:] + few[5:]}


@pytest.mark.parametrize("order", ["lab_first", "rgb_first", "alternating", "few_first_and_last"])
def test_job_table_with_mixed_kinds_and_early_returns(nq, oracle, monkeypatch, order):
    """12 LAB, 9 RGB and 9 LAB few-colours images (no merge job) in four orders: the merge jobs are a strict subset of the images
    and are sorted LAB first, so job j of the table is not image j.  Every image's result equals the oracle's whatever its position,
    and the recorded variant follows the number of merge jobs (21), not of images (30)."""
    for v in ("NQ_MERGE_THREADS", "NQ_MERGE_HELPERS", "NQ_BATCH_LANES"):
        monkeypatch.delenv(v, raising=False)
    base = _table_items()
    want_base = _want(base)
    for i, w in enumerate(want_base):
        assert (w[3]["maxbins"] > K) == (i < 21), (i, w[3]["maxbins"])
        assert i < 21 or 0 < w[3]["distinctColors"] <= K, (i, w[3]["distinctColors"])      # early return: no merge job
    perm = _orders()[order]
    assert sorted(perm) == list(range(30))
    items = [base[i] for i in perm]
    want = [want_base[i] for i in perm]
    b = _Batch(nq, items)
    _check_batch(b, b.run(), want, what="%s, position" % order)
    cus = _cus()
    threads, h_lab, h_rgb = _rule(12, 9, cus)
    assert threads == 512
    for pos, i in enumerate(perm):
        exp = (threads, h_lab) if i < 12 else (threads, h_rgb) if i < 21 else (0, 0)
        assert b.qs[pos].merge_variant() == exp, (order, pos, i, b.qs[pos].merge_variant(), exp)
    for q in b.qs:
        q.close()


# ---- 5. a failing image in the middle of a batch -------------------------------------------------------------------------------------
def _fail_items(n, tag):
    out = []
    for i in range(n):
        w, h = SHAPES[(2 * i) % 7]
        out.append(("%s%d" % (tag, i), (0 if i % 3 == 1 else 1, GENS[i % 4][0], w, h, 1100 + i, GENS[i % 4][1], 0), 1200 + i))
    return out


def _usable_afterwards(b, want):
    """(a) the same handles run the corrected batch, (b) each handle converts alone: the oracle's results, all stage events."""
    b.clear()
    _check_batch(b, b.run(), want, what="corrected batch, image")
    for i in range(len(b.qs)):
        pal, idx, argb = b.single(i)
        _same(pal, idx, argb, want[i], "handle %d alone after the failed batch" % i, b.qs[i].params)
        ms = b.qs[i].stage_ms()
        assert all(v >= 0 for v in ms.values()) and ms["total"] > 0, (i, ms)


@pytest.mark.parametrize("fault", ["zero_width", "null_input"])
def test_invalid_image_in_the_middle_of_a_device_batch(nq, oracle, monkeypatch, fault):
    """Nine images on the default four lanes, image 5 invalid (width 0, then a null input pointer).  The device form of the batch
    does not look at sizes or pointers up front, so the image is rejected on the host by the prepare step INSIDE lane 1's thread, after
    the other lanes have queued work.  The call returns NQ_ERR_INVALID with the text on the FIRST handle; the same handles then run the
    corrected batch and convert alone with the oracle's results (stream, scratch and stage events restored).

    Regression note: the failed call used to return while the kernels the other lanes had queued could still be running -- the lane
    streams do not synchronise with the handles' own streams, so a following call on a handle could overlap them on the handle's
    buffers.  nq_convert_batch_device now waits for every lane before it reports a lane's failure."""
    monkeypatch.delenv("NQ_BATCH_LANES", raising=False)
    items = _fail_items(9, "bad")
    want = _want(items)
    b = _Batch(nq, items)
    if fault == "zero_width":
        b.qs[5].width = 0
        with pytest.raises(nq.NqError) as ei:
            b.run()
        b.qs[5].width = b.imgs[5].shape[1]
    else:
        good = b.d_in[5]

        class _Null:
            @staticmethod
            def data_ptr():
                return 0
        b.d_in[5] = _Null
        with pytest.raises(nq.NqError) as ei:
            b.run()
        b.d_in[5] = good
    assert ei.value.status == -1                       # NQ_ERR_INVALID, read from the first handle by the host mirror
    assert "bad argument" in str(ei.value)
    assert b.qs[0]._L.nq_last_error(b.qs[0]._h).decode() in str(ei.value)
    _usable_afterwards(b, want)
    for q in b.qs:
        q.close()


def test_invalid_image_behind_the_sixteenth_handle(nq, oracle, monkeypatch):
    """20 images, image 17 with height 0: handles 16..19 were switched to the three-event recording of a batch when the call failed;
    afterwards they convert alone with all eight stage times again, and the corrected batch equals the oracle."""
    monkeypatch.delenv("NQ_BATCH_LANES", raising=False)
    items = _fail_items(20, "bad")
    want = _want(items)
    b = _Batch(nq, items)
    b.qs[17].height = 0
    with pytest.raises(nq.NqError) as ei:
        b.run()
    b.qs[17].height = b.imgs[17].shape[0]
    assert ei.value.status == -1 and "bad argument" in str(ei.value)
    for i in (18, 16, 19, 17):
        pal, idx, argb = b.single(i)
        _same(pal, idx, argb, want[i], "handle %d alone after the failed batch" % i, b.qs[i].params)
        ms = b.qs[i].stage_ms()
        assert all(v >= 0 for v in ms.values()) and ms["total"] > 0, (i, ms)
    _usable_afterwards(b, want)
    for q in b.qs:
        q.close()


def test_reference_throws_in_the_middle_of_a_batch(nq, oracle, monkeypatch):
    """Position 2 of 4 holds the 4200x4200 opaque LAB image whose fullest bin saturates the float count: the reference throws
    (ColorUtils.setAlphaComponent), the merge workgroup reports it and the batch returns NQ_ERR_REFERENCE_THROWS (-4) after the palettes
    of the images in front of it have been accepted.  All four handles then convert a small image with the oracle's result."""
    import torch
    monkeypatch.delenv("NQ_BATCH_LANES", raising=False)
    items = _fail_items(4, "thr")
    want = _want(items)
    b = _Batch(nq, items)
    big = synth.flat_with_patch(4200, 0xFF, 77)
    small = (b.d_in[2], b.qs[2].width, b.qs[2].height)
    assert b.qs[2].KIND == 1
    b.d_in[2] = torch.from_numpy(big.reshape(-1)).cuda()
    b.qs[2].height, b.qs[2].width = big.shape
    b.clear()
    with pytest.raises(nq.NqError) as ei:
        b.run()
    assert ei.value.status == -4 and "setAlphaComponent" in str(ei.value)
    b.d_in[2], b.qs[2].width, b.qs[2].height = small
    for i in (2, 3, 0, 1):
        pal, idx, argb = b.single(i)
        _same(pal, idx, argb, want[i], "handle %d alone after the batch that throws" % i, b.qs[i].params)
    _usable_afterwards(b, want)
    for q in b.qs:
        q.close()


def test_host_batch_rejects_bad_arguments_before_any_work(nq, oracle):
    """nq_convert_batch (host buffers): a null input buffer, a handle listed twice and palette_stride < nMaxColors each return
    NQ_ERR_INVALID before anything is written (outputs, palettes and K keep their fill), with the text on the first handle; the corrected
    call on the same handles then equals the oracle."""
    items = _fail_items(5, "host")
    want = _want(items)
    b = _Batch(nq, items)
    n = len(items)
    L = nq.load_library()
    h_in = [np.ascontiguousarray(im).reshape(-1).copy() for im in b.imgs]
    h_out = [np.full(a.size, 0x5A5A5A5A, np.int32) for a in h_in]
    h_idx = [np.full(a.size, 0x5A5A, np.uint16) for a in h_in]
    widths = np.array([q.width for q in b.qs], np.int32)
    heights = np.array([q.height for q in b.qs], np.int32)
    seeds = np.array([q.seed for q in b.qs], np.int64)
    pal = np.full((n, K), 0x5A5A5A5A, np.int32)
    got_k = np.full(n, -7, np.int32)

    def call(handles=None, null_input=None, stride=K):
        hs = (C.c_void_p * n)(*[q._h for q in (handles or b.qs)])
        src = (C.c_void_p * n)(*[None if i == null_input else a.ctypes.data for i, a in enumerate(h_in)])
        dst = (C.c_void_p * n)(*[a.ctypes.data for a in h_out])
        idx = (C.c_void_p * n)(*[a.ctypes.data for a in h_idx])
        return L.nq_convert_batch(hs, n, src, widths.ctypes.data, heights.ctypes.data, K, 1, seeds.ctypes.data, TILED, dst, idx,
                                  pal.ctypes.data, stride, got_k.ctypes.data)

    def untouched():
        return all((a == 0x5A5A5A5A).all() for a in h_out) and all((a == 0x5A5A).all() for a in h_idx) and \
            (pal == 0x5A5A5A5A).all() and (got_k == -7).all()

    for kwargs, text in (({"null_input": 3}, "image 3"), ({"handles": b.qs[:2] + [b.qs[1]] + b.qs[3:]}, "twice"), ({"stride": K - 1}, "palette_stride")):
        assert call(**kwargs) == -1, kwargs
        assert text in L.nq_last_error(b.qs[0]._h).decode(), (kwargs, L.nq_last_error(b.qs[0]._h))
        assert untouched(), kwargs
    assert call() == 0, L.nq_last_error(b.qs[0]._h)
    for i in range(n):
        _same(pal[i, :got_k[i]], h_idx[i], h_out[i], want[i], "host batch, image %d" % i, b.qs[i].params)
    for q in b.qs:
        q.close()
