"""CPU-side checks of shot detection (include/nquant_abi.h "shot detection"): nq_shots_from_signatures -- host arithmetic, no device --
driven through the built library on signatures computed with numpy and compared with the restatement in shots_ref.py: the two clips
with the starts and scores the definition gives, the late cut under min_shot, the extreme scores, the graded score of a brightness
shift, a slow fade cut by the anchor, rejected signatures and arguments with untouched outputs; and the interface: the five symbols,
the Python entry points and their argument checks that need no device."""
import ctypes as C
import inspect

import numpy as np
import pytest

import shots_ref


def _call(L, sig, n, npix, cut, min_shot, starts=0, count=0, scores=0):
    """The raw call with sentinel-filled outputs; starts / count / scores = None passes NULL.  Returns (rc, starts, count, scores)."""
    sig = None if sig is None else np.ascontiguousarray(sig, np.uint32)
    o_starts = np.full(max(n, 1) + 2, -5, np.int32)
    o_scores = np.full(max(n, 1) + 2, -5, np.int32)
    o_count = C.c_int32(-5)
    rc = L.nq_shots_from_signatures(None if sig is None else sig.ctypes.data, n, npix, cut, min_shot,
                                    None if starts is None else o_starts.ctypes.data, None if count is None else C.byref(o_count),
                                    None if scores is None else o_scores.ctypes.data)
    return rc, o_starts, o_count.value, o_scores


def _library(L, frames, cut, min_shot):
    n, npix = len(frames), np.asarray(frames[0]).size
    rc, starts, count, scores = _call(L, shots_ref.signatures(frames), n, npix, cut, min_shot)
    assert rc == 0
    assert (starts[count:] == -5).all() and (scores[n:] == -5).all()           # nothing behind what was asked for
    return starts[:count].tolist(), scores[:n].tolist()


@pytest.fixture(scope="module")
def L(nq):
    return nq.load_library()


def test_sprite_clip_has_one_cut_where_the_channels_rotate(nq, L):
    clip = shots_ref.sprite_cut_clip()
    assert len(clip) == 8 and clip[0].shape == (96, 128)
    assert _library(L, clip, 60, 1) == ([0, 4], [0, 1, 1, 1, 94, 1, 1, 1])
    assert _library(L, clip, 60, 8)[0] == [0]
    assert _library(L, clip, 1000, 1)[0] == [0]
    for cut, min_shot in ((60, 1), (60, 8), (1000, 1), (0, 1), (93, 1), (94, 1), (0, 3)):
        assert _library(L, clip, cut, min_shot) == shots_ref.detect(clip, cut, min_shot), (cut, min_shot)
    # the Python entry point is the same call
    starts, scores = nq.shots_from_signatures(shots_ref.signatures(clip), 96 * 128, cut=60, min_shot=1)
    assert starts == [0, 4] and scores.tolist() == [0, 1, 1, 1, 94, 1, 1, 1]
    assert nq.shots_from_signatures(shots_ref.signatures(clip), 96 * 128)[0] == [0]       # the defaults: min_shot = 8


def test_a_cut_suppressed_by_min_shot_is_taken_late(L):
    show = shots_ref.slide_show()
    assert len(show) == 7 and all(f.shape == (96, 128) for f in show)
    assert _library(L, show, 60, 1)[0] == [0, 2, 4, 5]
    assert _library(L, show, 60, 2)[0] == [0, 2, 4, 6]
    assert _library(L, show, 60, 3)[0] == [0, 3, 6]
    for min_shot in (1, 2, 3, 4, 7, 8):
        assert _library(L, show, 60, min_shot) == shots_ref.detect(show, 60, min_shot), min_shot


def test_extreme_and_graded_scores(L):
    black, white = np.full((1, 1), 0xFF000000, np.uint32), np.full((1, 1), 0xFFFFFFFF, np.uint32)
    assert _library(L, [black, white], 999, 1) == ([0, 1], [0, 1000])
    assert _library(L, [black, white], 1000, 1) == ([0], [0, 1000])           # 1000 never cuts
    rng = np.random.default_rng(4)
    f = rng.integers(0, 2**32, (9, 13), dtype=np.uint64).astype(np.uint32)
    assert _library(L, [f, f, f], 0, 1) == ([0], [0, 0, 0])                   # identical frames score 0; a cut needs score > threshold
    # a brightness shift of d levels scores floor(1000 d / 255), whatever the picture
    g = np.full((5, 7), 0xFF000000, np.uint32) | rng.integers(0, 100, (5, 7)).astype(np.uint32) * 0x010101
    for d in (1, 3, 50, 155):
        assert _library(L, [g, g + np.uint32(d * 0x010101)], 1000, 1)[1] == [0, 1000 * d // 255], d
    # alpha is the fourth channel and counts like the others
    assert _library(L, [g, g & np.uint32(0x00FFFFFF)], 1000, 1)[1] == [0, 1000]


def test_slow_fade_accumulates_against_the_anchor(L):
    """8 levels (about 3 %) per frame: 31, 62, 94 per mille against the shot's first frame -- a cut every third frame at threshold
    60.  Against the frame before, every step would score 31 and nothing would ever be cut."""
    frames = [np.full((4, 6), 0xFF000000 | (10 + 8 * i) * 0x010101, np.uint32) for i in range(8)]
    starts, scores = _library(L, frames, 60, 1)
    assert scores == [0, 31, 62, 31, 62, 31, 62, 31] and starts == [0, 2, 4, 6]
    assert (starts, scores) == shots_ref.detect(frames, 60, 1)
    assert _library(L, frames, 60, 3) == ([0, 3, 6], [0, 31, 62, 94, 31, 62, 94, 31])


def test_random_signatures_equal_the_restatement(L):
    rng = np.random.default_rng(12)
    for w, h, n in ((1, 1, 3), (7, 3, 9), (33, 20, 12)):
        frames = []
        for i in range(n):
            lo = int(rng.integers(0, 200))
            frames.append(rng.integers(lo, lo + int(rng.integers(1, 56)), (h, w, 4)).astype(np.uint32))
        frames = [f[..., 0] << 24 | f[..., 1] << 16 | f[..., 2] << 8 | f[..., 3] for f in frames]
        for cut in (0, 20, 100, 400):
            for min_shot in (1, 2, 5):
                assert _library(L, frames, cut, min_shot) == shots_ref.detect(frames, cut, min_shot), (w, h, n, cut, min_shot)


def test_rejected_signatures_and_arguments_leave_the_outputs_alone(L):
    clip = shots_ref.sprite_cut_clip()[2:6]
    sig, n, npix = shots_ref.signatures(clip), 4, 96 * 128
    assert _call(L, sig, n, npix, 60, 1)[0] == 0
    short = sig.copy()
    short[3, 2, 17] -= 1                            # one row of the last frame no longer sums to npix
    moved = sig.copy()
    moved[1, 0, 255] += 1
    bad = [dict(sig=short), dict(sig=moved), dict(npix=npix + 1), dict(npix=0), dict(npix=-1), dict(npix=2**31), dict(sig=None),
           dict(n=0), dict(n=-1), dict(cut=-1), dict(cut=1001), dict(min_shot=0), dict(min_shot=-3), dict(starts=None), dict(count=None)]
    for kw in bad:
        a = dict(sig=sig, n=n, npix=npix, cut=60, min_shot=1)
        a.update(kw)
        rc, starts, count, scores = _call(L, a.pop("sig"), a.pop("n"), a.pop("npix"), a.pop("cut"), a.pop("min_shot"), **a)
        assert rc == -1, kw
        assert (starts == -5).all() and count == -5 and (scores == -5).all(), kw
    # out_scores NULL is the form without scores
    rc, starts, count, scores = _call(L, sig, n, npix, 60, 1, scores=None)
    assert rc == 0 and starts[:count].tolist() == [0, 2] and (scores == -5).all()


def test_shots_symbols_and_wrappers_are_exported(nq, L):
    for name in ("nq_frame_signatures_device", "nq_frame_signatures", "nq_shots_from_signatures", "nq_detect_shots_device", "nq_detect_shots"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
    for name in ("frame_signatures", "frame_signatures_device", "shots_from_signatures", "detect_shots", "detect_shots_device",
                 "convert_clip_to_gif"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    for fn in (nq.shots_from_signatures, nq.detect_shots, nq.detect_shots_device, nq.convert_clip_to_gif):
        p = inspect.signature(fn).parameters
        assert p["cut"].default == 60 and p["min_shot"].default == 8, fn
    clip, shots = inspect.signature(nq.convert_clip_to_gif).parameters, inspect.signature(nq.convert_shots_to_gif).parameters
    assert [k for k in clip if k not in ("cut", "min_shot")] == [k for k in shots if k != "shot_starts"]
    assert all(clip[k].default == shots[k].default for k in shots if k != "shot_starts")


def test_python_argument_checks_need_no_device(nq, L):
    frames = [np.zeros((4, 4), np.int32)] * 2
    with pytest.raises(ValueError):
        nq.detect_shots([])
    with pytest.raises(ValueError):
        nq.frame_signatures([np.zeros((4, 4), np.int32), np.zeros((4, 5), np.int32)])
    with pytest.raises(TypeError):
        nq.detect_shots([np.zeros((4, 4), np.float32)])
    with pytest.raises(ValueError):
        nq.detect_shots_device(None, [], 4, 4)
    with pytest.raises(ValueError):
        nq.frame_signatures_device(None, [], 4, 4)
    with pytest.raises(ValueError):
        nq.shots_from_signatures(np.zeros(1000, np.uint32), 16)
    with pytest.raises(nq.NqError) as e:
        nq.shots_from_signatures(shots_ref.signatures(frames), 16, cut=1001)
    assert e.value.status == -1
    with pytest.raises(ValueError):
        nq.convert_clip_to_gif(0, frames, 257, True)
    with pytest.raises(ValueError):
        nq.convert_clip_to_gif(0, frames, 16, True, delta=False, hold=3)
    with pytest.raises(ValueError):
        nq.convert_clip_to_gif(0, [np.zeros((4, 4), np.int32), np.zeros((4, 5), np.int32)], 16, True, delta=False)
    with pytest.raises(ValueError):
        nq.convert_clip_to_gif(0, frames, 16, True, seeds=[1])
    # a null handle is refused without a device
    assert L.nq_frame_signatures(None, 1, None, 4, 4, None) == -1 and L.nq_frame_signatures_device(None, 1, None, 4, 4, None) == -1
    assert L.nq_detect_shots(None, 1, None, 4, 4, 60, 8, None, None, None) == -1
    assert L.nq_detect_shots_device(None, 1, None, 4, 4, 60, 8, None, None, None) == -1
