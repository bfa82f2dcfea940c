"""What tests/test_gpu_fast_filters.py rests on, checked without a GPU: the tanh domain and its disputed inputs, the oracle's array
exports, the host references of nextInt(32767), and the constants read from csrc/nq_dither_fast.hip."""
import ctypes as C
import decimal
import math
import os
import re

import numpy as np

import fast_filters_ref as R
from conftest import ROOT


def test_tanh_domain_and_disputed_share():
    """The shortcut of tanh_to_float runs for 0.5 <= |x| < 9.2 (compared in f64): 34 812 724 floats per sign, the last one the float nearest
    to 9.2, which lies below it (34 812 723 is the distance between the bit patterns of 0.5f and 9.2f).  An input is disputed when numpy's f64
    tanh -+ 1.2e-14 narrow to different floats; at most 1e-6 of the domain may be (the kernel's comment says 3e-7 of the calls)."""
    assert R.TANH_COUNT == 34_812_724
    assert float(R.bits_to_f32(R.TANH_FIRST)) == 0.5
    assert float(R.bits_to_f32(R.TANH_FIRST + R.TANH_COUNT - 1)) < 9.2 <= float(R.bits_to_f32(R.TANH_FIRST + R.TANH_COUNT))
    disputed = R.tanh_disputed_bits()
    share = disputed.size / R.TANH_COUNT
    print("tanh: %d disputed inputs of %d, share %.3g" % (disputed.size, R.TANH_COUNT, share))
    assert 0 < share <= 1e-6


def test_tanh_disputed_inputs_resolved_exactly(oracle):
    """Every disputed input at 60 digits: the oracle's float is the correctly rounded one, and the true value stays 4.5e-16 clear of the
    midpoint of the two candidate floats -- so a device library that is a few ulps of the double off still has to give the same float."""
    decimal.getcontext().prec = 60
    bits = R.tanh_disputed_bits()
    x = R.bits_to_f32(bits)
    got = oracle.limiter_tanh_n(x)
    v = np.tanh(x.astype(np.float64))
    lo, hi = (v - R.TANH_WINDOW).astype(np.float32), (v + R.TANH_WINDOW).astype(np.float32)
    for i in range(bits.size):
        t = (-2 * decimal.Decimal(float(x[i]))).exp()
        true = (1 - t) / (1 + t)
        mid = (decimal.Decimal(float(lo[i])) + decimal.Decimal(float(hi[i]))) / 2
        assert np.nextafter(lo[i], np.float32(2)) == hi[i]
        assert abs(true - mid) >= decimal.Decimal("4.5e-16"), "x = %r: tanh lies %s from a float midpoint" % (float(x[i]), abs(true - mid))
        want = lo[i] if true < mid else hi[i]
        assert got[i] == want, "x = %r: oracle %r, correctly rounded %r" % (float(x[i]), float(got[i]), float(want))
        assert oracle.limiter_tanh_n(-x[i:i + 1])[0] == -want


def test_oracle_array_exports_match_the_scalar_ones(oracle):
    rng = np.random.default_rng(20261)
    n = 10_000
    c1 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    c2 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    L = oracle.lib()
    yd = oracle.y_diff_n(c1, c2)
    lab = oracle.rgb2lab_n(c1)
    for i in range(n):
        assert yd[i] == L.nqo_y_diff(int(c1[i]), int(c2[i]))
        assert tuple(lab[i]) == oracle.rgb2lab(int(c1[i]))
    # (float) Math.tanh((double) x): the C library's tanh behind Python's math.tanh is the one the oracle links
    x = np.concatenate([rng.uniform(-12, 12, n - 4), [0.5, -0.5, 9.2, 1e30]]).astype(np.float32)
    t = oracle.limiter_tanh_n(x)
    assert (t == np.array([math.tanh(float(v)) for v in x], np.float32)).all()
    # err of closestColorIndex: the statement sequence restated in numpy (float32 coefficient times difference, f64 everywhere else) ...
    pairs = np.stack([c1, c2], axis=1)
    PR, PG, PB = 0.299, 0.587, 0.114
    for ratio in (0.0, 1.0, 0.3, 0.7615):
        err = oracle.closest_err_n(PR, PG, PB, ratio, pairs)
        assert (err == R.closest_err_numpy(PR, PG, PB, ratio, pairs)).all()
    # ... and the scalar path through closestColorIndex itself: closest[2] of a one-entry palette is (int) err
    img = np.full((1, 1), -1, np.int32)
    q = oracle.OracleQuantizer(oracle.OracleQuantizer.LAB, img)
    p = q.params
    p.PR, p.PG, p.PB, p.ratio = PR, PG, PB, 0.3
    q.set_params(p)
    opaque = pairs | np.int32(-0x1000000)
    err = oracle.closest_err_n(PR, PG, PB, 0.3, opaque)
    for i in range(0, n, 50):
        tup = q.closest_tuple(opaque[i, 1:2], opaque[i:i + 1, 0])
        assert tup[0, 2] == int(err[i])


def test_nextint_host_reference_is_java_nextint(oracle):
    """The int64 restatement the GPU test compares with, against the oracle's nextInt(32767) on 10^5 generator states."""
    rng = np.random.default_rng(7)
    states = rng.integers(0, 1 << 48, 100_000, dtype=np.int64)
    uu = ((states * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)) >> 17          # next(31) of the state after one step
    r, accept = R.nextint_ref(uu)
    L = oracle.lib()
    st = C.c_int64()
    for i in range(states.size):
        st.value = int(states[i])
        want = L.nqo_jrandom_next_int_bound(C.byref(st), 32767)
        if accept[i]:
            assert want == r[i]
    assert accept.all()          # (a rejection has probability 1e-9)
    # the two draws the bound rejects: 2^31 = 2 (mod 32767), so the last block of 32767 values is two short
    r, accept = R.nextint_ref(np.array([2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1], np.int64))
    assert accept.tolist() == [True, False, False] and r.tolist() == [32766, 0, 1]


def test_constants_read_from_the_kernel_source():
    """The GPU test's bounds are the kernel's own: the EPS constant, the factor of the `safe` test (the runner-up must be twice EPS
    behind, so an error of EPS on each of two distances cannot swap them), delta, the Y_Diff switch and the tanh window, and they cover what that test demands of them."""
    k = R.kernel_constants()
    assert k["near_eps"] == 3.0e-3
    assert k["safe_factor"] == 2.0
    assert k["delta_rel"] == 2.0 ** -20 and k["delta_abs"] == 1e-6
    # every pair within 2e-3 of a threshold must reach the f64 path: the float32 difference is within 1e-4 (the kernel's own bound), the
    # float32 threshold within 4e-6 (half an ulp below 128)
    assert k["ydiff_switch"] == 2.2e-3 and k["ydiff_switch"] >= 2e-3 + 1e-4 + 4e-6
    # every input the reference disputes (numpy's tanh -+ 1.2e-14) must reach the library: the kernel's v is within 1e-15 of tanh (its
    # own bound), numpy's within one place (1.2e-16)
    assert k["tanh_window"] == 1.5e-14 and k["tanh_window"] >= R.TANH_WINDOW + 1e-15 + 1.2e-16


def test_export_and_wrapper_exist(nq):
    L = nq.load_library()
    assert hasattr(L, "nq_selftest_fast") and "nq_selftest_fast" in nq.abi_symbols()
    assert callable(nq.PnnLABQuantizer.selftest_fast)
    hdr = open(os.path.join(ROOT, "include", "nquant_abi.h")).read()
    from nquant.android_amd import host
    for name, (code, _) in host.FAST_ST.items():
        assert re.search(r"^#define NQ_FAST_ST_%s %d$" % (name, code), hdr, re.M), name
    assert re.search(r"^#define NQ_FAST_ST_MODES %d$" % len(host.FAST_ST), hdr, re.M)
    assert sorted(code for code, _ in host.FAST_ST.values()) == list(range(len(host.FAST_ST)))
    # a null handle is refused before anything touches a device
    out = np.zeros(4, np.uint32)
    src = np.array([0, 1, 0, 0], np.int64)
    assert L.nq_selftest_fast(None, 0, src.ctypes.data, 1, out.ctypes.data) == -1
