"""The scalar shortcuts of the specialised dither kernel (csrc/nq_dither_fast.hip), each on its own and over its whole input domain,
through nq_selftest_fast -- the hook calls the device functions the dither kernel calls.  References: numpy's f64 tanh and the oracle's
own statements (array exports of oracle/nq_oracle.c).  Every test prints the figures DESIGN.md quotes before it asserts."""
import ctypes as C

import numpy as np
import pytest

import fast_filters_ref as R
from nquant.android_amd import host, synth

pytestmark = pytest.mark.gpu

CHUNK = 1 << 22
CUBE = 1 << 24
NEAR_EPS = R.near_eps()          # read from the kernel source; test_fast_filters_cpu.py checks that `safe` keeps twice this margin


def _copy_params(src, dst_cls):
    p = dst_cls()
    for f, _ in dst_cls._fields_:
        setattr(p, f, getattr(src, f))
    return p


@pytest.fixture(scope="module")
def q(nq):
    return nq.PnnLABQuantizer(np.zeros((1, 1), np.int32))


_cache = {}


def _cube_quantizers(oracle):
    """Params and palettes of the two images of test_gpu_fast_dither.py's colour-cube test (256 colours)."""
    if "cube" not in _cache:
        res = []
        for img in (synth.gradient_noise(160, 160, 3), synth.with_alpha(synth.uniform_rgb(112, 112, 161), 161, p_transparent=0.02, p_semi=0.0)):
            oq = oracle.OracleQuantizer(1, img)
            oq.prescan(256)
            pal = oq.pnnquan(256)
            res.append((oq.params, pal))
        _cache["cube"] = res
    return _cache["cube"]


def _set_weights(nq, q, oracle, ratio):
    op = _cube_quantizers(oracle)[0][0]
    p = _copy_params(op, nq.Params)
    p.ratio = ratio
    q.set_params(p)
    return p.PR, p.PG, p.PB


def _opaque(lo, hi):
    return (np.arange(lo, hi, dtype=np.uint32) | np.uint32(0xFF000000)).view(np.int32)


# ---- tanh ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [0, 1])
def test_tanh_whole_shortcut_domain(q, oracle, sign):
    """Every float with 0.5 <= |x| < 9.2.  Outside the disputed set (numpy's f64 tanh -+ 1.2e-14 narrow differently; the kernel's window
    of 1.5e-14 covers that, its stated error 1e-15 and numpy's last place) the result is the narrowed f64 tanh bit for bit; on the disputed set it is the
    oracle's float (correctly rounded there, test_fast_filters_cpu.py) and the library must have decided."""
    n_disp = n_lib = 0
    for s in range(0, R.TANH_COUNT, CHUNK):
        n = min(CHUNK, R.TANH_COUNT - s)
        first = R.TANH_FIRST + s + (sign << 31)
        out = q.selftest_fast("TANH", first, n)
        bits = np.arange(first, first + n, dtype=np.uint32)
        x = bits.view(np.float32)
        want, disp = R.tanh_reference(x)
        got = out[:, 0].view(np.float32)
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~disp
        assert not bad.any(), "%d undisputed inputs differ, first x = %r (bits 0x%08x): gpu %r, reference %r, library decided %d" % (
            int(bad.sum()), float(x[bad][0]), int(bits[bad][0]), float(got[bad][0]), float(want[bad][0]), int(out[bad][0, 1]))
        if disp.any():
            ow = oracle.limiter_tanh_n(x[disp])
            assert (got[disp].view(np.uint32) == ow.view(np.uint32)).all(), (x[disp], got[disp], ow)
            assert (out[disp, 1] == 1).all(), "a disputed input was decided by the shortcut: %r" % x[disp][out[disp, 1] != 1]
        n_disp += int(disp.sum())
        n_lib += int(out[:, 1].sum())
    print("tanh sign %d: disputed %d of %d (%.3g), library decided %d (%.3g)" % (
        sign, n_disp, R.TANH_COUNT, n_disp / R.TANH_COUNT, n_lib, n_lib / R.TANH_COUNT))
    assert n_disp / R.TANH_COUNT <= 1e-6
    assert n_lib >= n_disp


def test_tanh_named_case_boundary_just_outside_1e_14(q, oracle):
    """x = 4.0137434f: tanh lies between 1e-14 and 1.2e-14 from a float boundary.  With a window of 1e-14 the shortcut decided this input
    itself (correctly, but closer to the boundary than the disputed set allows); it belongs to the library."""
    x = np.array([4.0137434, -4.0137434], np.float32)
    assert R.tanh_reference(x)[1].all()
    out = q.selftest_fast("TANH_BITS", records=x.view(np.uint32))
    assert (out[:, 0] == oracle.limiter_tanh_n(x).view(np.uint32)).all() and (out[:, 1] == 1).all()


def test_tanh_saturated_and_small_inputs(q, oracle):
    """|x| >= 9.2 gives +-1.0f (every binade edge up to FLT_MAX, the infinities, 2^20 seeded values); |x| < 0.5 takes the library
    and equals the oracle (2^20 seeded non-zero values).  Zero and NaN are not inputs of the limiter (|e| >= 25)."""
    rng = np.random.default_rng(92)
    first_sat = R.TANH_FIRST + R.TANH_COUNT
    edges = np.array([e << 23 for e in range(0x82, 0xFF)], np.uint32)                  # 2^3 (below 9.2: left out next) .. 2^127
    edges = np.concatenate([edges - 1, edges, edges + 1, [first_sat, first_sat + 1, 0x7F7FFFFF, 0x7F800000]]).astype(np.uint32)
    edges = edges[edges >= first_sat]
    big = np.concatenate([edges, rng.integers(first_sat, 0x7F800000, 1 << 20, dtype=np.int64).astype(np.uint32)])
    big = np.concatenate([big, big | np.uint32(0x80000000)])
    out = q.selftest_fast("TANH_BITS", records=big)
    want = np.where(big >> 31 == 1, np.float32(-1), np.float32(1))
    assert (out[:, 0].view(np.float32) == want).all() and (out[:, 1] == 0).all()
    small = rng.integers(1, R.TANH_FIRST, 1 << 20, dtype=np.int64).astype(np.uint32)
    small = np.concatenate([small, [1, R.TANH_FIRST - 1], small | np.uint32(0x80000000)]).astype(np.uint32)
    out = q.selftest_fast("TANH_BITS", records=small)
    ow = oracle.limiter_tanh_n(small.view(np.float32))
    bad = out[:, 0] != ow.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), small[bad][:4], out[bad][:4, 0], ow.view(np.uint32)[bad][:4])
    assert (out[:, 1] == 1).all()


# ---- closestColorIndex: floor of the quadratic form ----------------------------------------------------------------------------------
def _ratios(oracle):
    return [0.0, 1.0, 0.05, 0.3, 0.5, 0.8] + [p.ratio for p, _ in _cube_quantizers(oracle)]


@pytest.mark.parametrize("which", range(8))
def test_closest_form_all_triples(nq, q, oracle, which):
    """All 2^24 (|dr|, |dg|, |db|): F == floor(err) of the oracle's statement sequence; where the exact evaluation did not run the float32
    form lies within the kernel's delta = e32 * 2^-20 + 1e-6 of err; the signs of the differences do not matter."""
    ratio = _ratios(oracle)[which]
    PR, PG, PB = _set_weights(nq, q, oracle, ratio)
    worst = 0.0
    n_exact = 0
    for lo in range(0, CUBE, CHUNK):
        out = q.selftest_fast("CLOSEST_ERR", lo, CHUNK, a0=0)
        packed = np.arange(lo, lo + CHUNK, dtype=np.uint32)
        err = oracle.closest_err_n(PR, PG, PB, ratio, R.unpack_triples(packed, 0))
        F = out[:, 0].view(np.int32)
        bad = F != np.floor(err).astype(np.int32)
        assert not bad.any(), "ratio %r: %d triples, first 0x%06x: F %d, err %r, e32 %r, exact %d" % (
            ratio, int(bad.sum()), int(packed[bad][0]), int(F[bad][0]), float(err[bad][0]), float(out[bad][0, 1:2].view(np.float32)[0]), int(out[bad][0, 2]))
        e32 = out[:, 1].view(np.float32).astype(np.float64)
        delta = (e32 * 2.0 ** -20 + float(np.float32(1e-6))).astype(np.float32).astype(np.float64)   # the kernel's formula: one rounding, as the fma
        rel = np.abs(e32 - err) / delta
        fastpath = out[:, 2] == 0
        # the exact evaluation ran exactly where e32 lies within delta of an integer (the tuple is empty: no candidate is ruled out)
        e = out[:, 1].view(np.float32)
        frac, d32 = e - np.trunc(e), delta.astype(np.float32)
        assert ((~fastpath) == ((frac < d32) | (frac > np.float32(1) - d32))).all()
        n_exact += int((~fastpath).sum())
        worst = max(worst, float(rel[fastpath].max()))
        assert (rel[fastpath] <= 1.0).all(), "ratio %r: |e32 - err| exceeds delta at 0x%06x" % (ratio, int(packed[fastpath][np.argmax(rel[fastpath])]))
    print("closest ratio %r: max |e32 - err| / delta = %.4f, exact evaluations %d of %d" % (ratio, worst, n_exact, CUBE))
    rng = np.random.default_rng(500 + which)
    packed = rng.integers(0, CUBE, 1 << 20, dtype=np.int64).astype(np.uint32)
    base = q.selftest_fast("CLOSEST_ERR_PAIRS", records=R.unpack_triples(packed, 0))[:, 0]
    for mask in range(1, 8):
        got = q.selftest_fast("CLOSEST_ERR_PAIRS", records=R.unpack_triples(packed, mask))[:, 0]
        assert (got == base).all(), "sign mask %d changes F" % mask
    lo = int(packed.min()) & ~0xFFFF                                                       # the range form builds the same pairs
    got = q.selftest_fast("CLOSEST_ERR", lo, 1 << 16, a0=5)[:, 0]
    assert (got == q.selftest_fast("CLOSEST_ERR", lo, 1 << 16, a0=0)[:, 0]).all()


# ---- random.nextInt(32767) and the remainder ---------------------------------------------------------------------------------------
def test_nextint_fold(q):
    rng = np.random.default_rng(32767)
    k = rng.integers(0, 2 ** 31 // 32767 + 1, 1 << 16, dtype=np.int64)
    near = (k[:, None] * 32767 + np.arange(-2, 3)[None, :]).ravel()
    near = near[(near >= 0) & (near < 2 ** 31)]
    uu = np.concatenate([rng.integers(0, 2 ** 31, 1 << 22, dtype=np.int64), near, np.arange(2 ** 31 - 70000, 2 ** 31, dtype=np.int64)])
    out = q.selftest_fast("NEXTINT_LIST", records=uu.astype(np.int32))[:, 0]
    r, accept = R.nextint_ref(uu)
    assert ((out & 0xFFFF) == r).all() and ((out >> 16 == 1) == accept).all()
    assert accept[-3:].tolist() == [True, False, False] and int((~accept).sum()) == 2
    tail = q.selftest_fast("NEXTINT", 2 ** 31 - 70000, 70000)[:, 0]                          # the range form, same values
    assert (tail == out[-70000:]).all()
    bad, first = q.selftest_fast("NEXTINT_COUNT", 0, 2 ** 31)
    print("nextInt: %d disagreements over all 2^31 draws (first: %r)" % (bad, first))
    assert bad == 0 and first is None


def test_remainder(q):
    """The remainder of fast_closest_pick against Java's %: multiples of every divisor and their neighbours, seeded pairs (divisor larger
    than r, negative = a wrapped closest[2] + closest[3], and zero, which the pick never forms -- closest[2] >= 1, closest[3] >= closest[2] --
    and for which the helper leaves r as it is), and on the
    device every pair 0 <= r < 32767, 1 <= dsum <= r."""
    rs, ds = [], []
    for dsum in range(1, 32767):
        m = np.arange(0, 32767 + dsum, dsum, dtype=np.int64)
        r = np.concatenate([m - 1, m, m + 1])
        r = r[(r >= 0) & (r < 32767)]
        rs.append(r); ds.append(np.full(r.size, dsum, np.int64))
    rng = np.random.default_rng(11)
    n = 1 << 22
    r = rng.integers(0, 32767, n, dtype=np.int64)
    d = rng.integers(1, 40000, n, dtype=np.int64)
    e0 = rng.integers(1, 1 << 20, n // 4, dtype=np.int64)
    wrapped = ((e0 + np.where(rng.random(n // 4) < 0.5, 2 ** 31 - 1, rng.integers(2 ** 31 - 2 ** 20, 2 ** 31, n // 4))) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    d[:n // 4] = wrapped
    d[n // 4:n // 4 + 4096] = 0
    rs.append(r); ds.append(d)
    r, d = np.concatenate(rs), np.concatenate(ds)
    assert 900_000 < r.size - n < 1_200_000 and (d < 0).any() and (d == 0).sum() == 4096 and (d > r).any()
    out = q.selftest_fast("REM", records=np.stack([r, d], axis=1).astype(np.int32))[:, 0].view(np.int32)
    want = R.rem_ref(r, d)
    bad = out != want
    assert not bad.any(), (int(bad.sum()), r[bad][:4], d[bad][:4], out[bad][:4], want[bad][:4])
    bad, first = q.selftest_fast("REM_COUNT", 0, 1 << 30)
    print("remainder: %d disagreements over all pairs 1 <= dsum <= r < 32767 (first: %r)" % (bad, first))
    assert bad == 0 and first is None


# ---- Y_Diff threshold tests ----------------------------------------------------------------------------------------------------------
def _ydiff_thresholds(oracle):
    """(lt thresholds, gt thresholds) the kernel can pass: 2 * acceptedDiff <= 100 and (double) beta * acceptedDiff < 100.5, acceptedDiff =
    max(2, K - margin), 33 <= K <= 256; beta and margin from the oracle's GilbertCurve constructor at the weights of the DITHER_MAX = 25 rung
    that test_gpu_fast_dither.py uses: 26 and 229 values."""
    lt = sorted({2.0 * max(2, K - m) for K in range(33, 257) for m in (6, 8) if 2 * max(2, K - m) <= 100})
    gt = set()
    o = (C.c_int32 * 5)()
    for weight in (0.0115, 0.006, 0.003, 0.0026):
        for K in range(33, 257):
            beta = oracle.lib().nqo_gilbert_params(K, weight, 1, o)
            thr = float(np.float32(beta)) * max(2, K - o[0])
            if thr < 100.5:
                gt.add(thr)
    assert len(lt) == 26 and len(gt) > 200
    return np.array(lt), np.array(sorted(gt))


@pytest.mark.parametrize("c2", [0xFF000000, 0xFFFFFFFF, 0xFF808080])
def test_ydiff_every_colour_against_black_white_grey(q, oracle, c2):
    """Every opaque colour against one fixed colour under every threshold: the decision is the oracle's Y_Diff > thr (second stage) or
    < thr (first stage), and the float32 difference is within the 1e-3 switch margin of the oracle's -- the filter is right exactly then."""
    lt, gt = _ydiff_thresholds(oracle)
    c2i = np.int32(np.uint32(c2).view(np.int32))
    worst = 0.0
    for lo in range(0, CUBE, CHUNK):
        c1 = _opaque(lo, lo + CHUNK)
        yd64 = oracle.y_diff_n(c1, np.full(CHUNK, c2i, np.int32))
        # (the range form takes 32 thresholds per launch, one bit each)
        for thr, is_gt in [(lt, False)] + [(gt[i:i + 32], True) for i in range(0, gt.size, 32)]:
            out = q.selftest_fast("YDIFF_RANGE", lo, CHUNK, a0=int(c2i), thresholds=thr, gt=is_gt)
            full = (1 << thr.size) - 1
            if is_gt:
                want = (np.uint64(1) << np.searchsorted(thr, yd64, side="left").astype(np.uint64)) - np.uint64(1)
            else:
                want = np.uint64(full) & ~((np.uint64(1) << np.searchsorted(thr, yd64, side="right").astype(np.uint64)) - np.uint64(1))
            bad = out[:, 1] != want.astype(np.uint32)
            assert not bad.any(), "gt=%d: %d colours, first 0x%08x: decisions 0x%x, oracle 0x%x (Y_Diff %r)" % (
                is_gt, int(bad.sum()), int(c1[bad][0]) & 0xFFFFFFFF, int(out[bad][0, 1]), int(want[bad][0]), float(yd64[bad][0]))
            dev = np.abs(out[:, 0].view(np.float32).astype(np.float64) - yd64)
            worst = max(worst, float(dev.max()))
            assert (dev < 1e-3).all()
    print("Y_Diff against 0x%08x under %d + %d thresholds: max |yd32 - yd64| = %.3g" % (c2, lt.size, gt.size, worst))


def _block(lo, hi):
    v = np.arange(lo, hi, dtype=np.uint32)
    return (v[:, None, None] << 16 | v[None, :, None] << 8 | v[None, None, :]).ravel()


def _ydiff_threshold_pairs(oracle):
    """(records, expected decisions, pairs found per threshold).  The darker colour of a pair comes from the greys, the primary and secondary
    ramps, the dark corner of the cube and seeded colours; the brighter one from seeded colours, the same ramps and the bright corner (the
    high thresholds only have pairs between the two corners).  Candidates come from a sorted search on 100 Y; the oracle's Y_Diff of the
    pair decides whether it is kept."""
    if "ydiff_pairs" in _cache:
        return _cache["ydiff_pairs"]
    lt, gt = _ydiff_thresholds(oracle)
    rng = np.random.default_rng(215)
    ramp = np.arange(256, dtype=np.uint32)
    ramps = np.concatenate([ramp * 0x010101, ramp << 16, ramp << 8, ramp, ramp * 0x010100, ramp * 0x000101, ramp * 0x010001])
    black = np.int32(-0x1000000)

    def prepared(colours):
        colours = np.unique(colours) | np.uint32(0xFF000000)
        y = oracle.y_diff_n(colours.view(np.int32), np.full(colours.size, black, np.int32))          # 100 Y
        order = np.argsort(y, kind="stable")
        return colours[order], y[order]
    dark, yd_ = prepared(np.concatenate([ramps, _block(0, 40), rng.integers(0, CUBE, 1 << 14, dtype=np.int64).astype(np.uint32)]))
    pool, yp = prepared(np.concatenate([ramps, _block(216, 256), rng.integers(0, CUBE, 1 << 21, dtype=np.int64).astype(np.uint32)]))
    perm = rng.permutation(dark.size)
    dark, yd_ = dark[perm], yd_[perm]
    recs, wants, quota = [], [], []
    for thr, is_gt in [(t, False) for t in lt] + [(t, True) for t in gt]:
        for partners in (1 << 13, dark.size):                # a few thousand partners do, except at the high thresholds
            a, b = np.searchsorted(yp, yd_[:partners] + thr - 2.5e-3), np.searchsorted(yp, yd_[:partners] + thr + 2.5e-3)
            cnt = b - a
            if cnt.sum() >= 30000:
                break
        upto = int(np.searchsorted(np.cumsum(cnt), 30000)) + 1                  # enough partners for about 30 000 candidates
        a, cnt = a[:upto], cnt[:upto]
        which = np.repeat(np.arange(cnt.size), cnt)
        c2 = dark[:upto][which].view(np.int32)
        c1 = pool[a[which] + (np.arange(which.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))].view(np.int32)
        yd = oracle.y_diff_n(c1, c2)
        below, above = np.flatnonzero((yd < thr) & (yd > thr - 2e-3))[:1 << 12], np.flatnonzero((yd >= thr) & (yd < thr + 2e-3))[:1 << 12]
        keep = np.concatenate([below, above])
        quota.append((float(thr), is_gt, below.size, above.size))
        rec = np.zeros(keep.size, host.YDIFF_RECORD)
        rec["c1"], rec["c2"], rec["gt"], rec["thr"] = c1[keep], c2[keep], int(is_gt), thr
        recs.append(rec)
        wants.append(yd[keep] > thr if is_gt else yd[keep] < thr)
    _cache["ydiff_pairs"] = np.concatenate(recs), np.concatenate(wants), quota
    return _cache["ydiff_pairs"]


def test_ydiff_pairs_at_the_thresholds(q, oracle):
    """Per threshold at least 2^12 pairs whose oracle Y_Diff lies within 2e-3 of it, at least 2^11 on either side (the threshold 100 = 2 * 50
    excepted: no pair exceeds 100 and only a handful come within 2e-3 of it): the f64 path must decide each, as the oracle does."""
    rec, want, quota = _ydiff_threshold_pairs(oracle)
    for thr, is_gt, nb, na in quota:
        if thr < 100:
            assert nb + na >= 1 << 12 and nb >= 1 << 11 and na >= 1 << 11, (thr, is_gt, nb, na)
        else:
            assert na >= 1, "white against black is exactly 100"
    out = q.selftest_fast("YDIFF", records=rec)
    yd64 = oracle.y_diff_n(rec["c1"], rec["c2"])
    print("Y_Diff at the thresholds: %d pairs under %d thresholds, max |yd32 - yd64| = %.3g" % (
        rec.size, len(quota), float(np.abs(out[:, 1].view(np.float32) - yd64).max())))
    assert (out[:, 2] == 1).all(), "%d pairs within 2e-3 of their threshold were decided in float32" % int((out[:, 2] != 1).sum())
    bad = (out[:, 0] == 1) != want
    assert not bad.any(), (int(bad.sum()), rec[bad][:4], yd64[bad][:4])
    assert (np.abs(out[:, 1].view(np.float32) - yd64) < 1e-3).all()


def test_ydiff_named_case_between_1e_3_and_2e_3_of_the_threshold(q, oracle):
    """Two pairs whose Y_Diff lies 1e-3 .. 2e-3 from their threshold: while the switch stood at 1e-3 they were decided in float32 (correctly:
    the float32 error is 1.5e-5); they belong to the f64 statement.  0xFFC3CC99 against 0xFF2B551B is 49.99802 under the first-stage
    threshold 50 (<), 0xFF0A78C1 against 0xFF2B551B is 10.25800 under the second-stage threshold 0.18 * 57 = 10.26000040769577 (>)."""
    rec = np.zeros(2, host.YDIFF_RECORD)
    rec["c1"] = np.array([0xFFC3CC99, 0xFF0A78C1], np.uint32).view(np.int32)
    rec["c2"] = np.array([0xFF2B551B, 0xFF2B551B], np.uint32).view(np.int32)
    rec["gt"], rec["thr"] = [0, 1], [50.0, 10.26000040769577]
    yd = oracle.y_diff_n(rec["c1"], rec["c2"])
    assert ((np.abs(yd - rec["thr"]) > 1e-3) & (np.abs(yd - rec["thr"]) < 2e-3) & (yd < rec["thr"])).all()
    out = q.selftest_fast("YDIFF", records=rec)
    assert (out[:, 2] == 1).all() and out[:, 0].tolist() == [1, 0]


# ---- the two Lab conversions and the float32 distance ---------------------------------------------------------------------------------
def _oracle_lab_cube(oracle):
    """L, A, B of every opaque colour from the oracle, (2^24, 3) float32, computed once."""
    if "lab" not in _cache:
        lab = np.empty((CUBE, 3), np.float32)
        for lo in range(0, CUBE, CHUNK):
            lab[lo:lo + CHUNK] = oracle.rgb2lab_n(_opaque(lo, lo + CHUNK))[:, 1:4]
        lab.setflags(write=False)
        _cache["lab"] = lab
    return _cache["lab"]


def test_lab64_equals_oracle_and_lab32_within_its_bounds(q, oracle):
    """RGB2LAB_fast (hardware seed + Newton cube root) gives the oracle's floats for every opaque colour, bit for bit; lab32_of stays
    within the per-component bounds its comment states (1.5e-4, 1.2e-3, 5e-4)."""
    want = _oracle_lab_cube(oracle)
    mism = 0
    first = None
    worst = np.zeros(3)
    for lo in range(0, CUBE, CHUNK):
        l64 = q.selftest_fast("LAB64", lo, CHUNK)
        bad = (l64 != want[lo:lo + CHUNK].view(np.uint32)).any(axis=1)
        if bad.any() and first is None:
            j = int(np.flatnonzero(bad)[0])
            first = (hex(lo + j), l64[j].view(np.float32).tolist(), want[lo + j].tolist())
        mism += int(bad.sum())
        l32 = q.selftest_fast("LAB32", lo, CHUNK).view(np.float32)
        worst = np.maximum(worst, np.abs(l32.astype(np.float64) - l64.view(np.float32).astype(np.float64)).max(axis=0))
    print("LAB64 mismatches against the oracle: %d of %d; LAB32 against LAB64: max |dL| %.3g, |dA| %.3g, |dB| %.3g" % (
        mism, CUBE, worst[0], worst[1], worst[2]))
    assert mism == 0, "first %s" % (first,)
    assert worst[0] <= 1.5e-4 and worst[1] <= 1.2e-3 and worst[2] <= 5e-4


def _near_reference(lab_colour, lab_entry):
    """(double) fabsf(dL) + sqrt(dA^2 + dB^2) on float Lab values, the statement of fast_nearest_exact (differences in float32)."""
    dL = np.abs(lab_entry[..., 0] - lab_colour[..., 0]).astype(np.float64)
    dA = (lab_entry[..., 1] - lab_colour[..., 1]).astype(np.float64)
    dB = (lab_entry[..., 2] - lab_colour[..., 2]).astype(np.float64)
    return dL + np.sqrt(dA * dA + dB * dB)


HAND_PALETTE = np.array([0xFF000000, 0xFFFFFFFF, 0xFF808080, 0xFFFF0000, 0xFF00FF00, 0xFF0000FF, 0xFFFFFF00, 0xFF00FFFF, 0xFFFF00FF], np.uint32).view(np.int32)


@pytest.mark.parametrize("entry", range(9))
def test_near_d32_every_colour_against_the_hand_palette(q, oracle, entry):
    """The float32 distance of fast_nearest32 between every opaque colour and black, white, mid grey, the primaries and secondaries lies
    within NQ_FAST_NEAR_EPS of the exact statement on the oracle's Lab values."""
    lab = _oracle_lab_cube(oracle)
    q.nearestColorIndex(HAND_PALETTE, HAND_PALETTE[:1])              # puts the palette on the device
    pal_lab = oracle.rgb2lab_n(HAND_PALETTE)[:, 1:4]
    worst = 0.0
    for lo in range(0, CUBE, CHUNK):
        d32 = q.selftest_fast("NEAR_D32", lo, CHUNK, a0=entry)[:, 0].view(np.float32).astype(np.float64)
        dev = np.abs(d32 - _near_reference(lab[lo:lo + CHUNK], pal_lab[entry]))
        worst = max(worst, float(dev.max()))
        assert (dev <= NEAR_EPS).all(), "entry %d: |d32 - d64| = %.3g at colour 0x%06x" % (entry, float(dev.max()), lo + int(np.argmax(dev)))
    print("near entry %d (0x%08x): max |d32 - d64| = %.3g (NQ_FAST_NEAR_EPS %.3g)" % (entry, int(HAND_PALETTE[entry]) & 0xFFFFFFFF, worst, NEAR_EPS))


def test_near_d32_seeded_pairs_against_an_oracle_palette(q, oracle):
    lab = _oracle_lab_cube(oracle)
    pal = _cube_quantizers(oracle)[0][1]
    assert len(pal) == 256
    q.nearestColorIndex(pal, pal[:1])
    pal_lab = oracle.rgb2lab_n(pal)[:, 1:4]
    rng = np.random.default_rng(33)
    rgb = rng.integers(0, CUBE, 1 << 22, dtype=np.int64)
    k = rng.integers(0, 256, 1 << 22, dtype=np.int64)
    rec = np.stack([(rgb | 0xFF000000).astype(np.uint32).view(np.int32), k.astype(np.int32)], axis=1)
    d32 = q.selftest_fast("NEAR_D32_PAIRS", records=rec)[:, 0].view(np.float32).astype(np.float64)
    dev = np.abs(d32 - _near_reference(lab[rgb], pal_lab[k]))
    print("near, 2^22 seeded pairs against a 256-colour oracle palette: max |d32 - d64| = %.3g" % float(dev.max()))
    assert (dev <= NEAR_EPS).all()


def test_near_safe_means_the_float32_argmin_is_the_exact_one(q, oracle):
    """fast_nearest32 over two entries of an oracle palette, 2^22 seeded (colour, entry, entry): it reports `safe` exactly when its two
    float32 distances are more than 2 NQ_FAST_NEAR_EPS apart, and wherever it does, its pick is the argmin of the exact statement."""
    lab = _oracle_lab_cube(oracle)
    pal = _cube_quantizers(oracle)[0][1]
    q.nearestColorIndex(pal, pal[:1])
    pal_lab = oracle.rgb2lab_n(pal)[:, 1:4]
    rng = np.random.default_rng(34)
    n = 1 << 22
    rgb = rng.integers(0, CUBE, n, dtype=np.int64)
    ka = rng.integers(0, 256, n, dtype=np.int64)
    kb = (ka + rng.integers(1, 256, n, dtype=np.int64)) % 256
    # half of the pairs are neighbours in the palette, where the two distances often come close
    kb[::2] = np.minimum(ka[::2] + 1, 255) - (ka[::2] == 255) * 2
    col = (rgb | 0xFF000000).astype(np.uint32).view(np.int32)
    out = q.selftest_fast("NEAR_SAFE", records=np.stack([col, (ka | kb << 8).astype(np.int32)], axis=1))[:, 0]
    k1, safe = (out & 0xFFFF).astype(np.int64), (out >> 16) == 1
    da = q.selftest_fast("NEAR_D32_PAIRS", records=np.stack([col, ka.astype(np.int32)], axis=1))[:, 0].view(np.float32)
    db = q.selftest_fast("NEAR_D32_PAIRS", records=np.stack([col, kb.astype(np.int32)], axis=1))[:, 0].view(np.float32)
    assert (k1 == np.where(db < da, kb, ka)).all()
    want_safe = np.abs(da - db) > np.float32(2) * np.float32(NEAR_EPS)
    assert (safe == want_safe).all(), "%d pairs" % int((safe != want_safe).sum())
    ea, eb = _near_reference(lab[rgb], pal_lab[ka]), _near_reference(lab[rgb], pal_lab[kb])
    exact = np.where(eb < ea, kb, ka)
    ties = ea == eb
    print("near safe: %d of %d pairs unsafe, %d of them within NQ_FAST_NEAR_EPS..2 NQ_FAST_NEAR_EPS" % (
        int((~safe).sum()), n, int((~safe & (np.abs(da - db) > np.float32(NEAR_EPS))).sum())))
    assert (k1[safe & ~ties] == exact[safe & ~ties]).all()
    assert (~safe & (np.abs(da - db) > np.float32(NEAR_EPS))).sum() >= 16          # the band a halved margin would give away is populated


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def test_selftest_fast_refuses_bad_arguments(nq, q):
    L = nq.load_library()
    out = np.zeros(16, np.uint32)
    hdr = np.array([R.TANH_FIRST, 4, 0, 0], np.int64)
    call = lambda h, which, n: L.nq_selftest_fast(h, which, hdr.ctypes.data, n, out.ctypes.data)
    assert call(None, 0, 4) == -1
    for which in (-1, len(host.FAST_ST), 1000):
        assert call(q._h, which, 4) == -1
    assert call(q._h, 0, -4) == -1 and call(q._h, 0, 0) == -1
    assert call(q._h, 0, 5) == -1                                        # count of the header != n
    assert L.nq_selftest_fast(q._h, 0, None, 4, out.ctypes.data) == -1 and L.nq_selftest_fast(q._h, 0, hdr.ctypes.data, 4, None) == -1
    with pytest.raises(nq.NqError):
        q.selftest_fast("LAB64", CUBE - 2, 4)                            # a range past its domain
    with pytest.raises(nq.NqError):
        q.selftest_fast("CLOSEST_ERR", 0, 4, a0=8)
    got = q.selftest_fast("TANH", R.TANH_FIRST, 4)                       # and a valid call afterwards still works
    assert got[0, 0] == np.float32(np.tanh(0.5)).view(np.uint32)
