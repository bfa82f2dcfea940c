"""Orientation without a device: the restatement in orient_ref.py equals the per-pixel formulas of the header's table; the codes form
the dihedral group of the square; nq.orientation, nq.oriented_size and nq.source_rect equal the restatement; orienting commutes with
the reducer (ARGB and YUV sources, crops of every parity, both modes, a non-square source), which is what the reducing *_oriented
calls are built on; the new names are exported and declared; and the Python argument checks."""
import inspect
import os
import re

import numpy as np
import pytest

import orient_ref as O
import resample_ref as R
import yuv_ref as Y
from conftest import ROOT

ENTRY_POINTS = ("nq_orient_frames", "nq_frames_from_yuv_oriented", "nq_resample_frames_oriented", "nq_resample_frames_yuv_oriented")

# TABLE[a - 1][b - 1]: the code of orienting by a and the result by b.  With code = (r quarter turns clockwise, then m mirrors
# left-right), 1, 6, 3, 8 = (0..3, 0) and 2, 5, 4, 7 = (0..3, 1): (r1, m1) then (r2, m2) is (r1 + r2, m2) for m1 = 0 and
# (r1 - r2, 1 - m2) for m1 = 1 (a mirror turns a clockwise turn into a counterclockwise one).
TABLE = [[1, 2, 3, 4, 5, 6, 7, 8],
         [2, 1, 4, 3, 8, 7, 6, 5],
         [3, 4, 1, 2, 7, 8, 5, 6],
         [4, 3, 2, 1, 6, 5, 8, 7],
         [5, 6, 7, 8, 1, 2, 3, 4],
         [6, 5, 8, 7, 4, 3, 2, 1],
         [7, 8, 5, 6, 3, 4, 1, 2],
         [8, 7, 6, 5, 2, 1, 4, 3]]


def _coordinates(w, h):
    """A frame whose words are their own coordinates: y << 16 | x."""
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys << 16 | xs).astype(np.int32)


@pytest.mark.parametrize("size", [(1, 1), (1, 5), (5, 1), (4, 3), (7, 7), (3, 8)], ids=lambda s: "%dx%d" % s)
def test_restatement_equals_the_formulas_of_the_table(size):
    W, H = size
    src = _coordinates(W, H)
    for code in O.CODES:
        out = O.orient(src, code)
        ow, oh = O.oriented_size(W, H, code)
        assert out.shape == (oh, ow) and out.flags.c_contiguous and (ow, oh) == ((H, W) if code >= 5 else (W, H))
        for y in range(oh):
            for x in range(ow):
                sx, sy = O.FORMULAS[code](x, y, W, H)
                assert 0 <= sx < W and 0 <= sy < H and out[y, x] == (sy << 16 | sx), (code, x, y)


def test_codes_form_the_dihedral_group():
    for a in O.CODES:
        for b in O.CODES:
            assert O.compose(a, b) == TABLE[a - 1][b - 1], (a, b)
    src = _coordinates(5, 3)
    for a in O.CODES:
        for b in O.CODES:
            assert (O.orient(O.orient(src, a), b) == O.orient(src, TABLE[a - 1][b - 1])).all(), (a, b)
    assert O.compose(6, 8) == 1 and O.compose(8, 6) == 1
    assert [c for c in O.CODES if O.compose(c, c) == 1] == [1, 2, 3, 4, 5, 7]
    assert O.compose(6, 6) == 3 and O.compose(8, 8) == 3
    for row in TABLE:                                             # a group table: every row and column is a permutation
        assert sorted(row) == list(O.CODES)
    for col in zip(*TABLE):
        assert sorted(col) == list(O.CODES)


def test_orientation_of_a_rotation_and_a_mirror(nq):
    want = {(0, False): 1, (90, False): 6, (180, False): 3, (270, False): 8, (0, True): 2, (90, True): 5, (180, True): 4, (270, True): 7}
    for (rotation, mirror), code in want.items():
        assert nq.orientation(rotation, mirror) == code == O.orientation(rotation, mirror)
        assert nq.orientation(rotation, mirror=mirror) == code
    assert [nq.orientation(r) for r in (0, 90, 180, 270)] == [1, 6, 3, 8]
    for bad in (45, -90, 360, 1, 91, None, "90", True):
        with pytest.raises(ValueError):
            nq.orientation(bad)
        with pytest.raises(ValueError):
            nq.orientation(bad, True)


def test_oriented_size_and_source_rect_equal_the_restatement(nq):
    for w, h in ((1, 1), (5, 3), (4, 7)):
        for code in O.CODES:
            ow, oh = O.oriented_size(w, h, code)
            assert nq.oriented_size(w, h, code) == (ow, oh)
            for x in range(ow):
                for y in range(oh):
                    for rw in range(1, ow - x + 1):
                        for rh in range(1, oh - y + 1):
                            got = nq.source_rect(w, h, code, (x, y, rw, rh))
                            assert got == O.source_rect(w, h, code, (x, y, rw, rh)), (w, h, code, x, y, rw, rh)
    for bad in (0, 9, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            nq.oriented_size(4, 4, bad)
        with pytest.raises((ValueError, TypeError)):
            nq.source_rect(4, 4, bad, (0, 0, 1, 1))


def _swapped(size, code):
    return size[::-1] if code >= 5 else size


# (source width, height), crop in ORIENTED coordinates per code family, target: crops of every parity, a non-integer ratio, 1:1
GEOMETRIES = [((13, 9), (cx, cy, 6, 5), (4, 3)) for cx in (2, 3) for cy in (0, 1)] + [((13, 9), (1, 2, 7, 6), (7, 6)), ((8, 8), None, (3, 5))]


def _crop_for(code, crop):
    """The crop as given for codes 1..4; for the turning codes the same numbers with x and y swapped, so that it fits."""
    if crop is None:
        return None
    return (crop[1], crop[0], crop[3], crop[2]) if code >= 5 else crop


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d-%s" % (g[0][0], g[0][1], "full" if g[1] is None else "crop%d-%d" % g[1][:2]))
def test_orienting_commutes_with_the_reducer(nq, geometry):
    """orient(resample(f, mapped crop, swapped size)) == resample(orient(f), crop, size), word for word: the identity the reducing
    *_oriented calls are built on.  The frames hold transparent and translucent pixels."""
    (w, h), crop, size = geometry
    frames = [R.random_argb(w, h, 40 + i) for i in range(2)]
    for code in O.CODES:
        c = _crop_for(code, crop)
        s = _swapped(size, code) if crop is not None else size
        ow, oh = O.oriented_size(w, h, code)
        whole = (0, 0, ow, oh) if c is None else c
        mapped = nq.source_rect(w, h, code, whole)
        assert mapped == O.source_rect(w, h, code, whole)
        for flags in (R.LINEAR, 0):
            want = O.resample_oriented(frames, code, s, c, flags)
            got = O.orient_all(R.resample(frames, _swapped(s, code), mapped, flags), code)
            assert all(a.shape == b.shape == (s[1], s[0]) and (a == b).all() for a, b in zip(got, want)), (code, flags)


@pytest.mark.parametrize("origin", [(1, 1), (3, 2), (2, 3)], ids=lambda o: "crop%d-%d" % o)
def test_chroma_pairing_stays_in_source_coordinates(nq, origin):
    """The same through yuv_ref, with odd crop origins in oriented coordinates: converting the SOURCE frame (chroma sample
    (x >> 1, y >> 1) of the source pixel), reducing the mapped crop and orienting equals convert, orient, reduce.  Converting after
    orienting the planes would pair other samples: the test shows that this differs."""
    w, h = 13, 9
    frames = [Y.random_planes(w, h, 7 + i) for i in range(2)]
    for code in O.CODES:
        ow, oh = O.oriented_size(w, h, code)
        crop = origin + (ow - 4, oh - 4)
        size = (3, 2) if code < 5 else (2, 3)
        mapped = nq.source_rect(w, h, code, crop)
        for flags in (R.LINEAR, 0):
            want = O.resample_yuv_oriented(frames, code, size, crop, Y.BT709, flags)
            got = O.orient_all(Y.resample(frames, _swapped(size, code), mapped, Y.BT709, flags), code)
            assert all((a == b).all() for a, b in zip(got, want)), (code, flags)
    # an odd-sided frame mirrored: the pairs of the oriented planes are not the source's
    y, u, v = frames[0]
    wrong = Y.convert_one(y[:, ::-1], u[:, ::-1], v[:, ::-1], Y.BT709)
    assert (wrong != O.yuv_oriented(frames[:1], 2, Y.BT709)[0]).any()


def test_orient_symbols_and_wrappers_are_exported(nq):
    L = nq.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nquant_abi.h")).read(), flags=re.S)
    for base in ENTRY_POINTS:
        for name in (base, base + "_device"):
            assert name in nq.abi_symbols() and hasattr(L, name), name
            assert re.search(r"\bint %s\s*\(" % name, header), name
    assert L.nq_abi_version() == 1
    for name in ("orientation", "oriented_size", "source_rect", "orient_frames", "orient_frames_device"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    for fn in (nq.frames_from_yuv, nq.frames_from_yuv_device, nq.resample_frames, nq.resample_frames_device, nq.resample_frames_yuv,
               nq.resample_frames_yuv_device, nq.convert_frames_to_gif, nq.convert_shots_to_gif, nq.convert_clip_to_gif,
               nq.convert_frames_to_apng, nq.convert_frames_refined, nq.convert_frames_ordered):
        assert inspect.signature(fn).parameters["orient"].default == 1, fn.__name__
    assert list(inspect.signature(nq.convert_frames_to_gif).parameters)[-1] == "delta"
    # a null handle is refused by all eight
    assert L.nq_orient_frames(None, 1, None, 4, 4, 6, None) == -1
    assert L.nq_orient_frames_device(None, 1, None, 4, 4, 6, None) == -1
    assert L.nq_frames_from_yuv_oriented(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, 6, None) == -1
    assert L.nq_frames_from_yuv_oriented_device(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, 6, None) == -1
    assert L.nq_resample_frames_oriented(None, 1, None, 4, 4, 6, 0, 0, 4, 4, None, 2, 2, 1) == -1
    assert L.nq_resample_frames_oriented_device(None, 1, None, 4, 4, 6, 0, 0, 4, 4, None, 2, 2, 1) == -1
    assert L.nq_resample_frames_yuv_oriented(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, 6, 0, 0, 4, 4, None, 2, 2, 1) == -1
    assert L.nq_resample_frames_yuv_oriented_device(None, 1, None, None, None, 4, 4, 4, 2, 1, 0, 6, 0, 0, 4, 4, None, 2, 2, 1) == -1


def test_python_argument_errors_need_no_device(nq):
    frames = [np.zeros((4, 6), np.int32)]
    for bad in (0, 9, -1, 2.5, True, None, "6"):
        for call in (lambda: nq.orient_frames(frames, bad), lambda: nq.resample_frames(frames, (2, 2), orient=bad),
                     lambda: nq.frames_from_yuv([Y.random_planes(4, 4, 1)], orient=bad),
                     lambda: nq.convert_frames_to_gif(1, frames, 16, True, orient=bad),
                     lambda: nq.convert_frames_to_apng(1, frames, 16, True, orient=bad),
                     lambda: nq.convert_frames_ordered(1, frames, 16, 8, orient=bad)):
            with pytest.raises((ValueError, TypeError)):
                call()
    with pytest.raises(ValueError):
        nq.orient_frames_device(None, [], 4, 4, [], 6)
