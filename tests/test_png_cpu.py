"""CPU-side checks of the PNG encoder (include/nquant_abi.h "PNG encoding"): the restatement in png_ref.py writes files whose IDAT
Python's zlib inflates to the expected raw stream, whose chunk CRCs verify and which Pillow opens as the same palette image (so the
bytes the GPU tests compare against are right); nq_png_max_bytes bounds them; the Python wrappers exist; without a HIP device the host
form refuses to compute (no CPU fallback)."""
import io
import zlib

import numpy as np
import pytest

import png_cases
import png_ref
from conftest import HAS_GPU

try:
    from PIL import Image
except ImportError:                                  # the zlib checks still run
    Image = None

KS = (2, 3, 4, 5, 16, 17, 256)
SHAPES = ((1, 1), (1, 333), (37, 91), (256, 256))
KINDS = ("noise", "flat", "gradient")


def content(kind, h, w, K, rng):
    if kind == "noise":
        return rng.integers(0, K, (h, w))
    if kind == "flat":
        return np.full((h, w), K - 1)
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) * K // (h + w)) % K


def segment_lengths(h, w, K):
    """1, 7, 4096, the default and the whole raw stream (the longest segment the interface takes, 65535 bytes, where the stream is
    longer: 256 x 256 at 8 bits is 65792 bytes)."""
    return (1, 7, 4096, 0, min(65535, len(png_ref.raw_stream(np.zeros((h, w), np.uint8), K))))


def skewed_map():
    """Index counts that grow like Fibonacci numbers.  The counts of the INDICES would make a tree deeper than 15, but a block encodes
    tokens: the parse turns the frequent indices into matches, and no tree of this map's blocks reaches a limit
    (test_skewed_map_reaches_no_limit has the depths).  The limiters are reached by png_cases.limit_cases()."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(f, i, np.int64) for i, f in enumerate(fib)])
    rng = np.random.default_rng(8)
    rng.shuffle(vals)
    w = 151
    vals = np.concatenate([vals, np.full(-vals.size % w, len(fib) - 1, np.int64)])
    return vals.reshape(-1, w)


def check_file(png, idx, pal):
    K = len(pal)
    got, K2, plte, trns = png_ref.decode(png)
    assert K2 == K and (got == idx).all()
    assert plte == b"".join(bytes(((int(c) >> 16) & 255, (int(c) >> 8) & 255, int(c) & 255)) for c in pal)
    alpha = [(int(c) >> 24) & 255 for c in pal]
    nt = max((i + 1 for i, a in enumerate(alpha) if a != 255), default=0)
    assert trns == (bytes(alpha[:nt]) if nt else None)
    idat = dict(png_ref.parse(png))[b"IDAT"]
    assert zlib.decompress(idat) == png_ref.raw_stream(idx, K)
    if Image is not None:
        im = Image.open(io.BytesIO(png))
        im.load()
        assert im.mode == "P" and (np.array(im) == idx).all()
        assert im.getpalette()[:3 * K] == list(plte)
        if nt:
            t = im.info["transparency"]
            assert (bytes(t) if isinstance(t, bytes) else t) in (bytes(alpha[:nt]), alpha.index(0) if 0 in alpha else None)


@pytest.mark.parametrize("K", KS)
def test_restatement_is_a_png_of_the_index_map(K):
    rng = np.random.default_rng(K)
    for h, w in SHAPES:
        for S in segment_lengths(h, w, K):
            for kind in KINDS:
                idx = content(kind, h, w, K, rng)
                pal = (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.int64)
                check_file(png_ref.encode(idx, pal, S), idx, pal)


def test_restatement_alpha_and_length_limit():
    rng = np.random.default_rng(1)
    idx = content("noise", 37, 91, 17, rng)
    pal = (0xFF000000 | rng.integers(0, 1 << 24, 17)).astype(np.int64)
    pal[3] &= 0x00FFFFFF
    pal[9] = (pal[9] & 0x00FFFFFF) | 0x80000000
    png = png_ref.encode(idx, pal)
    check_file(png, idx, pal)
    assert dict(png_ref.parse(png))[b"tRNS"] == bytes([255, 255, 255, 0, 255, 255, 255, 255, 255, 0x80])
    idx = skewed_map()
    freq = np.bincount(idx.reshape(-1)).tolist()
    assert max(png_ref.code_lengths(freq, 15)) == 15 and max(png_ref.code_lengths(freq[:12], 7)) == 7
    check_file(png_ref.encode(idx, 0xFF000000 | np.arange(256), 65535), idx, 0xFF000000 | np.arange(256))


def test_skewed_map_reaches_no_limit():
    """What skewed_map() reaches at the segment lengths test_gpu_png.py::test_length_limited_codes uses: the largest depth, over the
    blocks, that each tree would have without a limit.  None is past its limit (15, 15, 7): the cut-and-repair loop does not run."""
    idx = skewed_map()
    pal = 0xFF000000 | np.arange(256)
    for S, want in ((65535, (13, 8, 6)), (0, (11, 8, 6)), (5000, (11, 9, 6))):
        stats = []
        assert png_ref.encode(idx, pal, S, stats=stats) == png_ref.encode(idx, pal, S)
        got = tuple(max(getattr(B, name) for B in stats) for name in ("lit_depth", "dist_depth", "cl_depth"))
        print(S, got)
        assert got == want, (S, got)
        assert all(max(B.lit_lens) == B.lit_depth and max(B.dist_lens) == B.dist_depth and max(B.cl_lens) == B.cl_depth for B in stats)


# ---- the limit cases (png_cases.py; DESIGN.md 5c "limit cases") ----
def _kraft_is_one(lens, limit):
    return sum(1 << (limit - l) for l in lens if l) == 1 << limit


def _matches(B):
    return [t for t in B.tokens if isinstance(t, tuple)]


def _third_word(B):
    """The items whose bits reach the third word of the emit window, and those of them with a set bit there."""
    reach = [it for it in B.items if (it[0] & 31) + it[1] > 64]
    return reach, [it for it in reach if it[2] >> (64 - (it[0] & 31))]


@pytest.mark.parametrize("name", png_cases.names())
def test_limit_case_is_a_png_within_the_bound(nq, name):
    _, idx, pal, S = png_cases.case(name)
    png, stats = png_cases.restated(name)
    assert png == png_ref.encode(idx, pal, S)                                # the statistics change no byte
    check_file(png, idx, pal)
    h, w = idx.shape
    assert nq.png_max_bytes([w], [h], len(pal), S) >= len(png)
    assert len(stats) == -(-len(png_ref.raw_stream(idx, len(pal))) // S)
    if name != "pooled":
        assert idx.size <= 65535


def test_len_limit_cuts_the_literal_length_code():
    B, = png_cases.restated("len_limit")[1]
    assert (B.length, len(B.tokens)) == (55035, 9574)
    assert B.lit_depth == 17 and max(B.lit_lens) == 15 and _kraft_is_one(B.lit_lens, 15)
    assert sorted(B.lit_lens) != sorted(min(l, 15) for l in png_ref.code_lengths(B.lit_hist, 286))      # the repair moved lengths
    assert B.hclen == 19                                                     # a length of 15 is in use: the last place of the order


def test_dist_limit_cuts_the_distance_code():
    B, = png_cases.restated("dist_limit")[1]
    print("dist_limit: depth", B.dist_depth, "of", sum(1 for c in B.dist_hist if c), "used symbols")
    assert B.dist_depth == 16 and max(B.dist_lens) == 15 and _kraft_is_one(B.dist_lens, 15)
    assert all(B.dist_hist[12:]) and sum(B.dist_hist[:12]) < 8               # the chain over symbols 12 .. 29, hardly anything else


def test_clc_limit_cuts_the_code_length_code():
    B, = png_cases.restated("clc_limit")[1]
    assert sorted(c for c in B.cl_hist if c) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55]
    assert B.cl_depth == 9 and max(B.cl_lens) == 7 and _kraft_is_one(B.cl_lens, 7)
    assert not _matches(B) and not any(B.dist_hist) and (B.hlit, B.hdist) == (257, 1)   # a block with no used distance symbol


def test_wide_items_reach_the_third_word_of_the_emit_window():
    B, = png_cases.restated("wide_items")[1]
    reach, with_bits = _third_word(B)
    longest = max(it[1] for it in B.items)
    print("wide_items: longest item %d bits, %d items reach the third word, %d with a set bit there" % (longest, len(reach), len(with_bits)))
    assert longest == 43                                                     # 48 is the format's maximum
    assert (len(reach), len(with_bits)) == (3, 2)
    widest = [(t, it[1]) for t, it in zip(B.tokens, B.items) if isinstance(t, tuple) and 227 <= t[0] <= 257 and t[1] >= 16385]
    assert widest == [((257, 32070), 43)]                                    # 5 and 13 extra bits
    # the inputs of the suite before these cases: no item longer than 27 bits, none past the second word
    old = []
    png_ref.encode(skewed_map(), 0xFF000000 | np.arange(256), 65535, stats=old)
    assert max(it[1] for B0 in old for it in B0.items) <= 27 and not any(_third_word(B0)[0] for B0 in old)


@pytest.mark.parametrize("D", [32767, 32768, 32769])
def test_far_edge_of_the_distance_window(D):
    B, = png_cases.restated("far_edge_%d" % D)[1]
    far = [t for t in _matches(B) if t[1] > 1]
    if D <= 32768:
        assert far == [(258, D)]
    else:
        assert far == [(3, 6)] and sum(1 for t in B.tokens if not isinstance(t, tuple)) == 9       # no far match: its three pixels are literals
    assert sum(1 for c in B.dist_hist if c) == (2 if D <= 32768 or far else 1)


def test_match_length_edges():
    _, idx, pal, S = png_cases.case("match_edges")
    raw = png_ref.raw_stream(idx, 256)
    stats = png_cases.restated("match_edges")[1]
    assert [B.length for B in stats] == [5000, 5000, 40]
    lengths = {t[0] for t in _matches(stats[0])}
    assert 257 in lengths and 258 in lengths                                 # symbol 284 with extra value 30, and symbol 285
    assert png_ref._length_symbol(257) == (284, 30, 5) and png_ref._length_symbol(258) == (285, 0, 0)
    for B in stats[1:]:
        assert B.tokens[-1][0] == 3                                          # a match of 3 that ends on the segment's last byte
    n, d = stats[0].tokens[-1]                                               # cut by L - m: the stream goes on alike past the segment
    assert n == 99 and d == 1 and raw[S - n - d:S + 50 - d] == raw[S - n:S + 50] and raw[S] != 0
    zero = png_cases.restated("all_zero")[1]
    assert [B.length for B in zero] == [4096, 4096, 811]
    for B in zero:                                                           # cut by L - m: the compare reads the zero padding
        assert B.tokens[0] == 0 and B.tokens[-1] == ((B.length - 1) % 258, 1) and set(B.tokens[1:-1]) == {(258, 1)}
        assert sum(1 for c in B.dist_hist if c) == 1                         # a block with exactly one used distance symbol


def test_run_length_edges():
    runs = {s: set() for s in (16, 17, 18)}
    for name in png_cases.names():
        for B in png_cases.restated(name)[1]:
            for s, e, _ in B.runs:
                if s >= 16:
                    runs[s].add(e + (11 if s == 18 else 3))
    assert {11, 138} <= runs[18] and {3, 10} <= runs[17] and {3, 6} <= runs[16], runs
    for name in ("run_edges_a", "run_edges_b", "run_edges_c"):
        B, = png_cases.restated(name)[1]
        assert not _matches(B)
    a = png_cases.restated("run_edges_a")[1][0].runs
    assert {(18, 0, 7), (18, 127, 7), (17, 0, 3), (17, 7, 3), (16, 0, 2), (16, 3, 2)} <= set(a)
    b = png_cases.restated("run_edges_b")[1][0].runs                         # 139 zeros: 138 and a plain zero
    i = b.index((18, 127, 7))
    assert b[i - 1][0] == 4 and b[i + 1] == (0, 0, 0) and b[i + 2][0] == 4
    c = png_cases.restated("run_edges_c")[1][0].runs                         # 148 zeros: 138 and 10
    i = c.index((18, 127, 7))
    assert c[i - 1][0] == 3 and c[i + 1] == (17, 7, 3) and c[i + 2][0] == 3


def test_header_extremes():
    """HLIT = 286, HDIST = 30 and HCLEN = 19 in one block; HLIT = 257 and HDIST = 1 with the smallest HCLEN there is beside them.
    HCLEN = 4 cannot occur: the code-length sequence always holds a length of 1 .. 15 (the end-of-block symbol's), and those stand
    at places 5 .. 19 of the order.  With HDIST = 1 the distance code's one length is 1, place 18 of the order: HCLEN >= 18."""
    B, = png_cases.restated("header_max")[1]
    assert (B.hlit, B.hdist, B.hclen) == (286, 30, 19) and B.lit_depth == 16 and max(B.lit_lens) == 15
    B, = png_cases.restated("run_edges_b")[1]
    assert (B.hlit, B.hdist, B.hclen) == (257, 1, 18)
    assert png_ref.CL_ORDER.index(1) == 17 and all(png_ref.CL_ORDER.index(l) >= 4 for l in range(1, 16))


def test_in_step_hash_groups():
    """Steps of 64 positions: one whose positions all share a hash, one with three groups or more, one in which two positions share
    a hash and not their three bytes (the candidate fails the byte test)."""
    steps = png_cases.restated("len_limit")[1][0].steps
    assert sum(1 for s in steps if s[0] == 64 and s[2] == 64) == 39
    assert sum(1 for s in steps if s[1] >= 3) == 769
    assert sum(s[3] for s in steps) == 0
    steps = png_cases.restated("dist_limit")[1][0].steps
    assert sum(s[3] for s in steps) == 94
    assert any(s[3] for s in png_cases.restated("pooled")[1][2].steps)       # and in noise


def test_pooled_segments():
    _, idx, pal, S = png_cases.case("pooled")
    stats = png_cases.restated("pooled")[1]
    assert S >= 4096 and len(stats) == 1101 and stats[-1].length == 2048 and all(B.length == S for B in stats[:-1])
    assert len({B.value for B in stats}) == 7                                # six blocks and the short one
    order = [B.value for B in stats[:-1]]
    assert sum(1 for x, y in zip(order, order[1:]) if x != y) > 800          # a chain mostly follows another block's


def test_max_bytes_is_exported_and_bounds_the_restatement(nq):
    L = nq.load_library()
    assert hasattr(L, "nq_png_max_bytes") and "nq_png_max_bytes" in nq.abi_symbols()
    rng = np.random.default_rng(11)
    for K in KS:
        for h, w in SHAPES:
            for S in segment_lengths(h, w, K):
                for kind in KINDS:
                    idx = content(kind, h, w, K, rng)
                    png = png_ref.encode(idx, 0xFF000000 | np.arange(K), S)
                    assert nq.png_max_bytes([w], [h], K, S) >= len(png), (K, h, w, S, kind)
                    assert nq.png_max_bytes([w], [h], None, S) >= len(png)
    assert nq.png_max_bytes([64, 99], [64, 17], [256, 3], 1) == nq.png_max_bytes([64], [64], 256, 1) + nq.png_max_bytes([99], [17], 3, 1)
    # pure arithmetic: the argument checks need no device
    for args in (([1], [1], 0, 0), ([1], [1], 257, 0), ([0], [1], 2, 0), ([65536], [1], 2, 0), ([1], [1], 2, -1), ([1], [1], 2, 65536),
                 ([], [], 2, 0), ([65535], [65535], 256, 0)):
        with pytest.raises(nq.NqError):
            nq.png_max_bytes(*args)


def test_png_wrappers_are_exported(nq):
    for name in ("encode_png", "encode_png_device", "write_png", "convert_to_png", "png_max_bytes"):
        assert callable(getattr(nq, name)) and name in nq.__all__, name
    L = nq.load_library()
    for name in ("nq_png_max_bytes", "nq_encode_png_device", "nq_encode_png"):
        assert name in nq.abi_symbols() and hasattr(L, name), name


def test_png_python_argument_checks(nq):
    with pytest.raises(ValueError):
        nq.encode_png([], [])
    with pytest.raises(ValueError):
        nq.encode_png([np.zeros(16, np.uint16)], [[0xFF000000]])
    with pytest.raises(TypeError):
        nq.encode_png([np.zeros((4, 4), np.float32)], [[0xFF000000]])
    with pytest.raises(ValueError):
        nq.convert_to_png(1, np.zeros((4, 4), np.int32), 257, True)


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_encode_png_has_no_cpu_fallback(nq):
    with pytest.raises(nq.NqError) as e:
        nq.encode_png(np.zeros((8, 8), np.uint16), [0xFF000000, 0xFFFFFFFF])
    assert e.value.status == -5
    with pytest.raises(nq.NqError) as e:
        nq.convert_to_png(0, np.full((8, 8), -1, np.int32), 16, False)
    assert e.value.status == -5
