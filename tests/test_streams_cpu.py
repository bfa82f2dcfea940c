"""What keeps tests/test_gpu_streams.py meaningful, checked without a GPU on the inputs its cases are built from (stream_gate.py):
  * the poison of every case is a valid input of the case's class -- same shapes and types, ARGB with the alpha kept, planes of
    bytes, indices below K;
  * for the quantizer cases the oracle's pre-scan scalars agree for the true and the poisoned image (opaque, far more than K colours),
    so only colours differ and both take the same path through the call;
  * the reference of the poison differs from the reference of the true input in EVERY output of the case, for per-pixel outputs in at
    least a quarter of the elements: a call that read the poison cannot pass;
  * an in-place case changes at least a quarter of what it is given, so a call whose writes were overwritten by the producer cannot
    pass either.
Two exceptions are stated, not hidden, and asserted as such.  Inverting a channel (v -> 255 - v in every frame) keeps every difference
of two values of that channel up to its sign, so no poison of the ARGB class moves (a) the scores of nq_detect_shots, 1-D earth mover's
distances per channel -- the signatures they are computed from go through the same kernel and table, and the signatures case does
tell the two apart -- and (b) the held COUNTS of the temporal hold, which depend on |differences| only; the held index maps and
outputs of the same call do change."""
import numpy as np
import pytest

import stream_gate as G

CASES = G.cases()
SYMMETRIC = {"detect_shots": ("starts", "scores"), "hold_counts": ("held",)}      # case prefix -> results the poison cannot move


def _u(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _valid(case, group, true, poison):
    assert len(true) == len(poison)
    for t, p in zip(true, poison):
        if "yuv" in group:
            assert all(a.dtype == np.uint8 and a.shape == b.shape and a.dtype == b.dtype and (a != b).all() for a, b in zip(t, p))
        elif "index" in group:
            assert p.dtype == np.uint16 and p.shape == t.shape and int(t.max()) < case.K and int(p.max()) < case.K and (p != t).all()
        else:
            assert p.dtype == np.int32 and p.shape == t.shape
            assert ((_u(p) >> 24) == (_u(t) >> 24)).all() and ((_u(p) ^ _u(t)) == 0x00FFFFFF).all()


def _differs(name, a, b):
    """Whether result `name` differs; per-pixel results must differ in a quarter of their elements."""
    if name.startswith(("out_", "io_")):
        for x, y in zip(a, b):
            share = float((_u(x) != _u(y)).mean())
            assert share >= 0.25, (name, share)
        return True
    if isinstance(a, (bytes, int)):
        return a != b
    if isinstance(a, list) and a and isinstance(a[0], bytes):
        return all(x != y for x, y in zip(a, b))
    return not np.array_equal(_u(a), _u(b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_poison_is_valid_and_changes_every_output(name):
    case = CASES[name]
    true, poison = case.inputs(False), case.inputs(True)
    assert sorted(true) == sorted(poison)
    for group in true:
        _valid(case, group, true[group], poison[group])
    if case.quant:
        kind, K = case.quant
        for t, p in zip(true["argb"], poison["argb"]):
            assert len(np.unique(t)) > 4 * K and len(np.unique(p)) > 4 * K
            assert G.oracle_scalars(kind, t, K) == G.oracle_scalars(kind, p, K) and G.oracle_scalars(kind, t, K)[:2] == (0, -1)
    good, bad = G.want(case), case.reference(poison)
    assert sorted(good) == sorted(bad)
    for key in good:
        if key in SYMMETRIC.get(name.split("-")[0], ()):
            assert not _differs(key, good[key], bad[key]), "no longer symmetric: drop the exception"
        elif key == "rects":
            assert good[key] == bad[key]                # (K - 1 - index keeps what is equal equal: the rectangles stay, the bodies change)
        elif key == "passes":
            continue                                    # (a count of passes, equal by chance or not)
        else:
            assert _differs(key, good[key], bad[key]), key
    for key in good:
        if key.startswith("io_"):                       # in place: the call changes what it is given
            assert any(float((_u(x) != _u(y)).mean()) >= 0.25 for x, y in list(zip(true[key], good[key]))[1:]), key


def test_batch_images_and_their_poisons():
    """Part B's six images: opaque with far more than K colours, like their poisons, with the pre-scan's scalars in agreement; and the
    oracle's result for the poison is another palette and another picture."""
    imgs = G.batch_images()
    good = G.batch_want()
    for (kind, w, h), img, seed, g in zip(G.BATCH, imgs, G.BATCH_SEEDS, good):
        assert img.shape == (h, w)
        p = G.invert_rgb(img)
        assert len(np.unique(img)) > 4 * G.BATCH_K and len(np.unique(p)) > 4 * G.BATCH_K
        assert G.oracle_scalars(kind, img, G.BATCH_K) == G.oracle_scalars(kind, p, G.BATCH_K)
        assert G.oracle_scalars(kind, img, G.BATCH_K)[:2] == (0, -1)
        bad = G.oracle_convert(kind, p, G.BATCH_K, seed)
        assert len(g[0]) == G.BATCH_K                   # (a merge job: the palette is full)
        assert not np.array_equal(bad[0], g[0]) and (bad[1] != g[1]).mean() >= 0.25 and (bad[2] != g[2]).mean() >= 0.25


def test_part_c_inputs_differ_between_the_two_calls():
    """Part C runs two calls back to back: their inputs (and so their pointer tables and results) are unrelated."""
    for kind in G.PAIR_KINDS:
        (_, wa, _), (_, wb, _) = G.pair_case(kind, 2), G.pair_case(kind, 9)
        for key in wa:
            assert len(wa[key]) == 2 and len(wb[key]) == 9
            assert all(float((_u(x) != _u(y)).mean()) >= 0.25 for x, y in zip(wa[key], wb[key])), (kind, key)
