"""CPU-side checks of the temporal hold (include/nquant_abi.h "temporal hold"): properties of the restatement in hold_ref.py that the
GPU tests compare against (what t = 0 holds, where a ramp is released and re-anchored, that an alpha flip is never held), the condition
the end-to-end tests put on their input (outside the sprite's old and new place everything is held), and the interface: both symbols
in the built library, the Python entry points, and the argument check that needs no device."""
import numpy as np
import pytest

import hold_ref


def _grey(v, alpha=255):
    v = np.asarray(v).astype(np.int64)
    return ((alpha << 24) | (v << 16) | (v << 8) | v).astype(np.uint32).view(np.int32)


def test_threshold_zero_on_identical_frames_holds_everything():
    rng = np.random.default_rng(1)
    f = rng.integers(-2**31, 2**31, (5, 7)).astype(np.int32)
    idx = [rng.integers(0, 256, (5, 7)).astype(np.uint16) for _ in range(4)]
    outs = [rng.integers(-2**31, 2**31, (5, 7)).astype(np.int32) for _ in range(4)]
    got, held, gout = hold_ref.hold([f] * 4, idx, 0, outs)
    assert held == [0, 35, 35, 35]
    for i in range(4):
        assert (got[i] == idx[0]).all() and (gout[i] == outs[0]).all()
    # one bit of difference in one channel of one pixel releases exactly that pixel
    g = f.copy()
    g[2, 3] ^= 1 << 8
    got, held, _ = hold_ref.hold([f, g, g], idx[:3], 0)
    assert held == [0, 34, 35] and got[1][2, 3] == idx[1][2, 3] and got[2][2, 3] == idx[1][2, 3]
    assert ((got[1] == idx[0]) | (np.arange(35).reshape(5, 7) == 17)).all()


def test_ramp_is_held_until_it_exceeds_the_threshold_and_re_anchors_there():
    frames = [_grey(np.full((2, 3), 100 + i)) for i in range(10)]
    idx = [np.full((2, 3), i, np.uint16) for i in range(10)]
    got, held, _ = hold_ref.hold(frames, idx, 3)
    # anchor 100 holds 101..103, 104 is released and becomes the anchor, holds 105..107, 108 is released
    assert [int(g[0, 0]) for g in got] == [0, 0, 0, 0, 4, 4, 4, 4, 8, 8]
    assert held == [0, 6, 6, 6, 0, 6, 6, 6, 0, 6]
    assert all((g == g[0, 0]).all() for g in got)


def test_alpha_flip_is_never_held_below_255():
    a, b = _grey(np.full((1, 4), 50), 0), _grey(np.full((1, 4), 50), 255)
    idx = [np.full((1, 4), i, np.uint16) for i in range(4)]
    for t in (0, 3, 254):
        got, held, _ = hold_ref.hold([a, b, a, b], idx, t)
        assert held == [0, 0, 0, 0] and all((g == i).all() for i, g in enumerate(got)), t
    got, held, _ = hold_ref.hold([a, b, a, b], idx, 255)
    assert held == [0, 4, 4, 4] and all((g == 0).all() for g in got)


@pytest.mark.parametrize("seed", [3, 11])
def test_noisy_sequence_is_held_outside_the_sprite(seed):
    h, w, n = 80, 96, 4
    frames, boxes = hold_ref.noisy_sprite_sequence(h, w, n, seed)
    assert len(frames) == n and all(f.shape == (h, w) and f.dtype == np.int32 for f in frames)
    assert any((frames[i] != frames[i - 1]).mean() > 0.9 for i in range(1, n))         # the noise is everywhere
    rng = np.random.default_rng(seed)
    idx = [rng.integers(0, 32, (h, w)).astype(np.uint16) for _ in range(n)]
    got, held, _ = hold_ref.hold(frames, idx, 4)
    for i in range(1, n):
        outside = ~hold_ref.union_mask(h, w, boxes[i - 1], boxes[i])
        assert (got[i][outside] == got[i - 1][outside]).all(), i
        assert held[i] >= int(outside.sum())
        # the sprite is 64 away from what it covers and uncovers: where it arrives, and where it left, nothing is held
        moved = hold_ref.union_mask(h, w, boxes[i]) ^ hold_ref.union_mask(h, w, boxes[i - 1])
        assert (hold_ref.distance(frames[i], frames[i - 1])[moved] >= 64).all()


def test_hold_symbols_and_wrappers_are_exported(nq):
    L = nq.load_library()
    for name in ("nq_hold_frames_device", "nq_hold_frames"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
    for name in ("hold_frames", "hold_frames_device"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    import inspect
    assert inspect.signature(nq.convert_frames_to_gif).parameters["hold"].default is None
    assert inspect.signature(nq.convert_frames_to_apng).parameters["hold"].default is None


def test_hold_python_argument_checks_need_no_device(nq):
    frames = [np.zeros((4, 4), np.int32)] * 2
    with pytest.raises(ValueError):
        nq.convert_frames_to_gif(0, frames, 16, True, delta=False, hold=3)
    with pytest.raises(ValueError):
        nq.convert_frames_to_gif(0, frames, 16, True, hold=3)
    for bad in (-1, 256, 2.5):
        with pytest.raises(ValueError):
            nq.convert_frames_to_gif(0, frames, 16, True, delta=True, hold=bad)
        with pytest.raises(ValueError):
            nq.convert_frames_to_apng(0, frames, 16, True, hold=bad)
        with pytest.raises(ValueError):
            nq.hold_frames(frames, [np.zeros((4, 4), np.uint16)] * 2, bad)
    with pytest.raises(ValueError):
        nq.hold_frames(frames, [np.zeros((4, 5), np.uint16)] * 2, 3)
    with pytest.raises(ValueError):
        nq.hold_frames(frames, [np.zeros((4, 4), np.uint16)], 3)
    with pytest.raises(ValueError):
        nq.hold_frames_device(None, [], [], 4, 4, 3)


def test_null_handle_is_refused_without_a_device(nq):
    L = nq.load_library()
    assert L.nq_hold_frames(None, 1, None, None, None, 4, 4, 3, None) == -1
    assert L.nq_hold_frames_device(None, 1, None, None, None, 4, 4, 3, None) == -1
