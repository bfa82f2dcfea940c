"""The lossy mode of the GIF encoders without a GPU: the restatement in gif_lossy_ref.py is the lossless restatement at lossy = 0, its
files decode (own decoder and Pillow) to colours within `lossy` of the source, transparent pixels are left alone, the exact index and
the smaller index win among duplicate colours, a dithered map shrinks, and the library exports the four calls."""
import io

import numpy as np
import pytest

import gif_delta_ref
import gif_lossy_ref as R
import gif_ref
from gif_delta_cases import palette_of, sequence

LOSSY = (1, 8, 40, 255)


def _maps():
    rng = np.random.default_rng(11)
    out = []
    for K in (3, 17, 256):
        out.append(("ramp dither", R.dithered(37, 91, K, rng), R.ramp_palette(K)))
        out.append(("random noise", rng.integers(0, K, (37, 91)), palette_of(K, rng)))
    idx, pal = R.noisy_gradient_map(48, 64, 64, 3)
    out.append(("sampled", idx, pal))
    return out


MAPS = _maps()


def test_lossy_zero_is_the_lossless_restatement():
    rng = np.random.default_rng(1)
    for _, idx, pal in MAPS:
        for S in (0, 7, 1000):
            assert R.encode(idx, pal, segment_pixels=S, lossy=0) == (gif_ref.encode(idx, pal, segment_pixels=S), 0)
    two = [MAPS[0][1], MAPS[0][1][::-1]]
    assert R.encode(two, MAPS[0][2], [3, 4], 5, 0, 0)[0] == gif_ref.encode(two, MAPS[0][2], [3, 4], 5, 0)
    for K in (3, 17, 255, 256):
        frames, pal = sequence(23, 31, K, rng), palette_of(K, rng)
        for S in (0, 7):
            assert R.encode_delta(frames, pal, segment_pixels=S, lossy=0) == (gif_delta_ref.encode(frames, pal, segment_pixels=S), 0)
    assert R.encode_delta(frames[:1], pal, lossy=0)[0] == gif_ref.encode(frames[0], pal)


@pytest.mark.parametrize("lossy", LOSSY)
def test_every_decoded_pixel_is_within_the_threshold(lossy):
    substituted = 0
    for name, idx, pal in MAPS:
        for S in (0, 7, 1000):
            data, subs = R.encode(idx, pal, segment_pixels=S, lossy=lossy)
            _, _, frames = gif_ref.parse(data)
            dec = frames[0]["index"]
            assert dec.shape == idx.shape and R.within(dec, idx, pal, lossy).all(), (name, S)
            assert int((dec != idx).sum()) == subs, (name, S)       # a substitute is never the exact index
            assert len(data) <= gif_ref.max_bytes([idx.shape], S)
            substituted += subs
    assert substituted > 0
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    name, idx, pal = MAPS[4]
    im = Image.open(io.BytesIO(R.encode(idx, pal, lossy=lossy)[0]))
    im.load()
    assert R.within(np.array(im), idx, pal, lossy).all()


@pytest.mark.parametrize("lossy", LOSSY)
def test_delta_mode_composes_within_the_threshold(lossy):
    rng = np.random.default_rng(5)
    for K in (17, 256):                                  # mark mode (u = 17) and crop only
        pal = R.ramp_palette(K)
        frames = [R.dithered(48, 64, K, rng)]
        for i in range(2):
            f = frames[-1].copy()
            f[10 + 9 * i:30 + 9 * i, 8 + 13 * i:40 + 13 * i] = R.dithered(20, 32, K, rng)
            frames.append(f)
        for S in (0, 50):
            data, subs = R.encode_delta(frames, pal, segment_pixels=S, lossy=lossy)
            _, _, parsed = gif_delta_ref.parse(data)
            assert [(p["x"], p["y"], p["w"], p["h"]) for p in parsed] == gif_delta_ref.rectangles(frames)
            for i, (c, f) in enumerate(zip(gif_delta_ref.compose(data), frames)):
                assert (c >= 0).all() and (c < K).all() and R.within(c, f, pal, lossy).all(), (K, S, i)
            if S == 0 and lossy >= 255 // (K - 1):               # the ramp's neighbours are candidates of each other
                assert subs > 0, K


def test_transparent_pixels_are_neither_replaced_nor_substituted():
    """Entries 7 and 9 have alpha 0: 7 is T, 9 an ordinary colour.  At lossy = 255 every other colour is a candidate for every pixel,
    and still the decoded map equals T exactly where the source does."""
    rng = np.random.default_rng(7)
    K = 16
    pal = palette_of(K, rng)
    pal[7] &= 0x00FFFFFF
    pal[9] &= 0x00FFFFFF
    assert gif_ref.transparent_index(pal) == 7
    idx = rng.integers(0, K, (64, 64))
    idx[20:30, :] = 7
    idx[rng.random(idx.shape) < 0.3] = 7
    for S in (0, 100):
        data, subs = R.encode(idx, pal, segment_pixels=S, lossy=255)
        assert subs > 0
        _, _, frames = gif_ref.parse(data)
        dec = frames[0]["index"]
        assert ((dec == 7) == (idx == 7)).all()
        assert (dec[idx == 9] != 7).all() and (dec != idx).any()
        assert frames[0]["transparency"] == 7


def _decoded(seq, pal, lossy):
    data, subs = R.encode(np.array([seq]), np.array(pal, np.int64), lossy=lossy)
    return gif_ref.parse(data)[2][0]["index"].tolist()[0], subs


def test_exact_index_first_then_the_smaller_index_among_duplicates():
    """Entry 0 is far from everything; entries 3 and 4 show one colour, 20 from entry 0's red; entries 1 and 2 are 10 to either side."""
    far, lo, hi, mid = 0xFFC8C8C8, 0xFF0A0000, 0xFF1E0000, 0xFF140000
    pal = [far, hi, lo, mid, mid]
    # (0, 3) enters the dictionary; 0, 4 then finds it at distance 0 and decodes as 3
    assert _decoded([0, 3, 0, 4], pal, 1) == ([0, 3, 0, 3], 1)
    # the exact pair wins: (0, 4) is in the dictionary, so 0, 4 stays 4 although entry 3 shows the same colour and is smaller;
    # 0, 3 is then a miss with the candidate 4
    assert _decoded([0, 4, 0, 4, 0, 3], pal, 1) == ([0, 4, 0, 4, 0, 4], 1)
    assert _decoded([0, 4, 0, 4, 0, 3], pal, 0) == ([0, 4, 0, 4, 0, 3], 0)
    # a tie on the distance: (0, 1) and (0, 2) both enter (20 apart, threshold 10), both are 10 from entry 3: the smaller index wins,
    # whichever colour it shows
    assert _decoded([0, 1, 0, 2, 0, 3], pal, 10) == ([0, 1, 0, 2, 0, 1], 1)
    assert _decoded([0, 2, 0, 1, 0, 3], [far, lo, hi, mid, mid], 10) == ([0, 2, 0, 1, 0, 1], 1)
    # the nearer colour wins over the smaller index: entry 2 is 4 from entry 3 now, entry 1 still 10
    assert _decoded([0, 1, 0, 2, 0, 3], [far, hi, 0xFF100000, mid, mid], 10) == ([0, 1, 0, 2, 0, 2], 1)
    # one short of the distance: no candidate, the exact index is written
    assert _decoded([0, 1, 0, 2, 0, 3], pal, 9) == ([0, 1, 0, 2, 0, 3], 0)
    # the metric is the largest channel difference: (10, 10, 10) away passes a threshold of 10
    assert _decoded([0, 1, 0, 2], [far, 0xFF141414, 0xFF0A0A0A], 10) == ([0, 1, 0, 1], 1)
    assert _decoded([0, 1, 0, 2], [far, 0xFF141414, 0xFF0A0A09], 10) == ([0, 1, 0, 2], 0)


def test_a_dithered_map_shrinks():
    """A 128 x 128 noisy gradient, randomly dithered onto 256 colours sampled from it (gif_lossy_ref.noisy_gradient_map, seed 1), one
    segmented frame.  Measured with the restatement: lossy = 32 gives 7127 bytes against 13443 lossless, ratio 0.5302 (56.6 % of the
    pixels substituted); 0.957 at lossy = 8 and 0.795 at 16.  The bound is that ratio rounded up to the next 0.05."""
    idx, pal = R.noisy_gradient_map(128, 128, 256, 1)
    lossless = gif_ref.encode(idx, pal)
    data, subs = R.encode(idx, pal, lossy=32)
    ratio = len(data) / len(lossless)
    print("lossy 32 / lossless: %d / %d = %.4f, %.3f of the pixels substituted" % (len(data), len(lossless), ratio, subs / idx.size))
    assert ratio < 0.55 and ratio < 1
    dec = gif_ref.parse(data)[2][0]["index"]
    assert R.within(dec, idx, pal, 32).all()


def test_the_library_exports_the_lossy_calls(nq):
    L = nq.load_library()
    for name in ("nq_encode_gif_lossy_device", "nq_encode_gif_lossy", "nq_encode_gif_delta_lossy_device", "nq_encode_gif_delta_lossy"):
        assert name in nq.abi_symbols() and hasattr(L, name), name
    import inspect
    for fn in (nq.encode_gif, nq.encode_gif_device, nq.encode_gif_delta, nq.encode_gif_delta_device):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "lossy" and last.default == 0, fn.__name__
    for fn in (nq.write_gif, nq.convert_frames_to_gif):          # these two keep `delta` last; lossy is a keyword before it
        p = inspect.signature(fn).parameters["lossy"]
        assert p.default == 0, fn.__name__
    with pytest.raises(TypeError):
        nq.write_gif("unused.gif", np.zeros((2, 2), np.uint16), [0xFF000000, 0xFFFFFFFF], None, 0, 0, 0, True)
