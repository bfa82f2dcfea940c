"""The WebP encoder's definition (include/nquant_abi.h "WebP encoding") as restated in webp_ref.py, without a GPU: every case of
webp_cases.py composes back to palette[index] through webp_ref's own reader and through libwebp (Pillow), stays within the bound, and
holds the tokens the case was made for; the library's argument checks as far as they go without a device; the exports."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import conftest
import png_ref
import webp_cases
import webp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ["nq_webp_max_bytes", "nq_encode_webp_device", "nq_encode_webp"]


def _shape(frames):
    h, w = np.asarray(frames[0]).shape
    return w, h


# ---- the restatement against its own reader ----
@pytest.mark.parametrize("name", webp_cases.names())
def test_the_restatement_composes_back(name):
    _, frames, pal, kw = webp_cases.case(name)
    data, stats = webp_cases.restated(name)
    own = webp_ref.compose(data)
    assert len(own) == len(frames)
    for i, f in enumerate(frames):
        assert (own[i] == webp_ref.rgba_of(f, pal)).all(), (name, i)
    parsed = webp_ref.read(data)
    rects = webp_ref.rectangles(frames, kw.get("delta", True))
    assert [f["rect"] for f in parsed["frames"]] == rects
    assert [f["bands"] for f in parsed["frames"]] == stats                  # the reader counts the tokens the writer made
    assert all(f["palette"] == [int(c) for c in pal] for f in parsed["frames"])
    if len(frames) > 1:
        delays = kw.get("delays_cs") or [0] * len(frames)
        assert [f["duration_ms"] for f in parsed["frames"]] == [10 * d for d in delays] and parsed["loop"] == kw["loop"]
        assert all(x % 2 == 0 and y % 2 == 0 for x, y, _, _ in rects)


@pytest.mark.parametrize("name", webp_cases.names())
def test_the_restatement_stays_within_the_bound(nq, name):
    _, frames, _, kw = webp_cases.case(name)
    data, _ = webp_cases.restated(name)
    w, h = _shape(frames)
    bound = webp_ref.max_bytes(len(frames), w, h, kw.get("band_bits", 0))
    print(name, len(data), bound)
    assert len(data) <= bound
    assert nq.webp_max_bytes(len(frames), w, h, kw.get("band_bits", 0)) == bound


def test_the_bound_formula_over_shapes(nq):
    for n, w, h, p in ((1, 1, 1, 0), (3, 16384, 16384, 0), (65535, 300, 250, 0), (2, 8193, 5, 0), (1, 300, 250, 9), (1, 4096, 4096, 3),
                       (7, 8192, 9, 2), (1, 65, 2000, 9)):
        assert nq.webp_max_bytes(n, w, h, p) == webp_ref.max_bytes(n, w, h, p), (n, w, h, p)


def test_the_band_statistics_are_what_the_cases_were_made_for():
    st = lambda name: webp_cases.restated(name)[1]
    assert st("constant") == [[(1, 10)]]                                    # one literal, then 2559 pixels in copies of 258 and less
    assert st("noise") == [[(48 * 64, 0)]]                                  # no copy: the distance code is unused
    assert all(c > 0 for _, c in st("repeated_rows")[0]) and sum(l for l, _ in st("repeated_rows")[0]) < 2 * 150 + 8
    assert len(st("three_bands")[0]) == 3 and len(st("four_bands")[0]) == 4
    assert st("one_pixel") == [[(1, 0)]]
    for name in webp_cases.names():
        if name.startswith("anim") and name.endswith("delta"):
            assert st(name)[2] == [(1, 0)], name                           # the unchanged frame: a 1 x 1 rectangle
    # repeated rows: the copies reach back one packed row
    _, frames, pal, _ = webp_cases.case("repeated_rows")
    toks = png_ref.tokens_of(webp_ref.pack(frames[0], len(pal)).tobytes())
    assert any(isinstance(t, tuple) and t[1] == 150 for t in toks)
    # the constant map's longest copies, and its one-symbol distance code
    _, frames, pal, _ = webp_cases.case("constant")
    toks = png_ref.tokens_of(webp_ref.pack(frames[0], len(pal)).tobytes())
    assert max(t[0] for t in toks if isinstance(t, tuple)) == 258 and {t[1] for t in toks if isinstance(t, tuple)} == {1}


def test_the_fibonacci_map_needs_the_length_limit():
    _, frames, pal, _ = webp_cases.case("fibonacci")
    packed = webp_ref.pack(frames[0], len(pal))
    assert packed.shape[0] <= 1 << webp_ref.band_bits_of(packed.shape[1])     # one band
    f = [0] * webp_ref.GREEN_SYMBOLS
    for t in png_ref.tokens_of(packed.tobytes()):
        f[256 + webp_ref.prefix_of(t[0])[0] if isinstance(t, tuple) else t] += 1
    free, cut = png_ref.code_lengths(f, 40), png_ref.code_lengths(f, 15)
    print("deepest leaf %d, limited to %d" % (max(free), max(cut)))
    assert max(free) > 15 and max(cut) == 15
    assert sum(2.0 ** -l for l in cut if l) == 1.0


# ---- the limit cases reach their limits (DESIGN.md "WebP encoder", the limit cases): asserted from the restatement's statistics, so
# that an edit of a case cannot quietly stop reaching what it was made for ----
def _bands(name):
    return [b for image in webp_cases.restated(name)[1] for b in image]


def test_the_old_cases_reach_none_of_the_limits():
    """What the limit cases add: before them no item reached a third word of the emit window or went past 32 bits, no chain was
    full, no call held more chains than a grid or more than 256 segments in an image."""
    old = [c[0] for c in webp_cases.cases()]
    bands = [b for name in old for b in _bands(name)]
    assert max(b.item_bits for b in bands) == 28 and not any(b.third_word or b.wide_items for b in bands)
    assert max(b.length for b in bands) < webp_ref.MAX_CHAIN and max(b.distance for b in bands) < 1 << 14
    assert max(b.green_depth for b in bands) == 15 and max(b.dist_depth for b in bands) == 5
    assert max(sum(len(image) for image in webp_cases.restated(name)[1]) for name in old) <= 5


@pytest.mark.parametrize("name,shape,nbands", [("full_chain_K17", (5, 8192), 2), ("full_chain_K16", (9, 16384), 3)])
def test_a_full_chain(name, shape, nbands):
    _, frames, pal, kw = webp_cases.case(name)
    bands = _bands(name)
    assert frames[0].shape == shape and len(bands) == nbands
    assert [b.length for b in bands] == [webp_ref.MAX_CHAIN] * (nbands - 1) + [8192]      # the last band is one packed row
    assert all(b[0] > 0 and b[1] > 0 for b in bands[:-1])                  # literals and copies in every full band
    assert webp_ref.pack(frames[0], len(pal)).shape[1] == 8192             # the widest packed row there is


def test_the_far_copy():
    band, = _bands("far_copy")
    assert band.length == webp_ref.MAX_CHAIN and band.distance == 32765
    assert webp_ref.prefix_of(band.distance + 120) == (30, 32765 + 119 - (1 << 15), 14)     # the top prefix pair, 14 extra bits
    assert band.distance >= 32649 and band.distance >> 14 == 1              # (a token that kept 14 bits of it would lose one)


def test_the_wide_items():
    """The committed map's reach, exactly: 46 of the 51 bits an item can have -- 12 + 7 of the length, 14 + 13 of the
    distance."""
    band, = _bands("wide_items")
    assert band.length == webp_ref.MAX_CHAIN
    assert (band.item_bits, band.green_depth, band.dist_depth) == (46, 12, 14)
    assert band.wide_items == 3                                            # items over 32 bits
    assert band.third_word == 2 and band.third_word_set == 2               # both put a 1 into the third word they reach
    assert band.distance >= 32649 and band.copy == 258


@pytest.mark.parametrize("name", ["many_bands_K2", "many_bands_K256"])
def test_many_bands(name):
    _, frames, pal, kw = webp_cases.case(name)
    stats = webp_cases.restated(name)[1]
    nbands = len(stats[0])
    assert len(stats) == 1 and nbands == 1025
    assert nbands > 256 and len({y >> 8 for y in range(nbands)}) >= 5      # the entropy image's red channel takes five values
    assert 1 + 2 * nbands > 2048                                           # nine rounds of the scan
    assert nbands > 1024                                                   # more chains than a grid of 4 x 256 workgroups
    assert webp_ref.pack(frames[0], len(pal)).shape[1] == 8 and all(b.length == 32 for b in stats[0][:-1])
    assert sum(1 for b in stats[0] if b[1]) > 100                          # bands with copies among them


def test_many_frames():
    _, frames, pal, kw = webp_cases.case("many_frames")
    data, stats = webp_cases.restated("many_frames")
    assert len(frames) == 1100 and len({id(f) for f in frames}) == 6 and not kw["delta"]
    assert len(data) > 4194304                                             # the gather's grid cap: 16384 x 256 bytes in one pass
    assert sum(len(image) for image in stats) == 4400 and all(len(image) == 4 for image in stats)
    assert len(set(kw["delays_cs"])) > 2


def test_many_frames_delta():
    _, frames, pal, kw = webp_cases.case("many_frames_delta")
    stats = webp_cases.restated("many_frames_delta")[1]
    rects = webp_ref.rectangles(frames, True)
    heights = [1 << webp_ref.band_bits_of(webp_ref.pack(np.zeros((1, w), np.int64), len(pal)).shape[1]) for _, _, w, _ in rects]
    print(sorted(set(heights)), sorted({len(image) for image in stats}))
    assert len(frames) == 300 and len(set(heights)) >= 3                   # images of one call with different band heights
    assert {len(image) for image in stats} == {1, 2}                       # and band counts
    longest = [max(b.length for b in image) for image in stats]
    assert sorted(longest)[-1] > sorted(longest)[-2]                       # one image alone sets the call's largest chain


def test_the_memo_of_vp8l_returns_what_it_computes():
    """vp8l is memoised by content: the 1100 frames of many_frames cost six restatements."""
    _, frames, pal, kw = webp_cases.case("many_frames")
    data, _ = webp_cases.restated("many_frames")
    key = tuple(int(c) for c in pal)
    assert sum(1 for k in webp_ref._VP8L if k[3] == key) == 6
    # the memo returns what the restatement computes: one frame restated afresh
    assert webp_ref._vp8l(np.asarray(frames[1]), list(key), 4)[0] == webp_ref.vp8l(frames[1], list(key), 4)
    assert data.endswith(webp_ref.chunk(b"VP8L", webp_ref._vp8l(np.asarray(frames[1099]), list(key), 4)[0]))


def test_a_single_length_symbol_never_stands_alone():
    """A band's first token is a literal (no match reaches before the band), so a green code that holds a length symbol holds a literal
    too: a code with one used symbol has a symbol below 256 and fits the simple form."""
    for name in webp_cases.names():
        _, frames, pal, kw = webp_cases.case(name)
        for f, (x, y, w, h) in zip(frames, webp_ref.rectangles(frames, kw.get("delta", True))):
            packed = webp_ref.pack(np.asarray(f)[y:y + h, x:x + w], len(pal))
            rows = 1 << webp_ref.band_bits_of(packed.shape[1], kw.get("band_bits", 0))
            for b in range(0, h, rows):
                assert not isinstance(png_ref.tokens_of(packed[b:b + rows].tobytes())[0], tuple)


def test_bundling_and_prefix_codes():
    assert [webp_ref.per_of(K) for K in (1, 2, 3, 4, 5, 16, 17, 256)] == [8, 8, 4, 4, 2, 2, 1, 1]
    assert webp_ref.pack(np.array([[1, 0, 1, 1, 0, 0, 0, 1, 1]]), 2).tolist() == [[0b10001101, 1]]
    assert webp_ref.pack(np.array([[3, 1, 2]]), 4).tolist() == [[3 | 1 << 2 | 2 << 4]]
    assert webp_ref.pack(np.array([[9, 15, 4]]), 16).tolist() == [[9 | 15 << 4, 4]]
    for v in list(range(1, 600)) + [4096, 32768 + 120]:
        s, e, eb = webp_ref.prefix_of(v)
        back = s + 1 if s < 4 else ((2 + (s & 1)) << ((s - 2) >> 1)) + e + 1
        assert back == v and eb == (0 if s < 4 else (s - 2) >> 1) and e < (1 << eb)
    assert [webp_ref.band_bits_of(pw) for pw in (1, 64, 65, 300, 4096, 8192)] == [9, 9, 8, 6, 3, 2]
    with pytest.raises(ValueError):
        webp_ref.band_bits_of(8193)


# ---- libwebp: the decoder that judges the format ----
@pytest.mark.parametrize("name", webp_cases.names())
def test_libwebp_composes_the_same_frames(name):
    pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check("webp"):
        pytest.skip("Pillow without WebP")
    _, frames, pal, kw = webp_cases.case(name)
    data, _ = webp_cases.restated(name)
    im = Image.open(io.BytesIO(data))
    assert im.format == "WEBP" and getattr(im, "n_frames", 1) == len(frames)
    w, h = _shape(frames)
    assert im.size == (w, h)
    durations = []
    for i, f in enumerate(frames):
        im.seek(i)
        assert (np.asarray(im.convert("RGBA")) == webp_ref.rgba_of(f, pal)).all(), (name, i)
        durations.append(im.info.get("duration", 0))
    if len(frames) > 1:
        delays = kw.get("delays_cs") or [0] * len(frames)
        assert durations == [10 * d for d in delays] and im.info["loop"] == kw["loop"]


# ---- the library without a device ----
def test_the_calls_are_declared_and_exported(nq):
    L = nq.load_library()
    header = open(os.path.join(HERE, "..", "include", "nquant_abi.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in nq.abi_symbols() and ("int %s(" % s) in header, s
        assert "nq_handle" not in header.split("int %s(" % s)[1].split(")")[0]
    for name in ("webp_max_bytes", "encode_webp", "encode_webp_device", "write_webp", "convert_to_webp", "convert_frames_to_webp"):
        assert hasattr(nq, name) and name in nq.__all__, name


class _Call:
    """One valid call of both entry points on host memory (the device form only ever gets as far as the argument checks here, or to a
    device that is not there), with fields to spoil."""

    def __init__(self):
        self.device, self.n, self.w, self.h, self.K, self.loop, self.band_bits, self.delta = 0, 2, 6, 4, 3, 0, 0, 1
        self.maps = [np.zeros((4, 6), np.uint16) for _ in range(2)]
        self.pal = np.array([0xFF000000, 0xFFFFFFFF, 0x80808080], np.uint32)
        self.delays = np.array([1, 2], np.int32)
        self.ptrs = [m.ctypes.data for m in self.maps]
        self.table, self.p_pal, self.p_delays = True, self.pal.ctypes.data, self.delays.ctypes.data
        self.out = np.full(1 << 16, 0xAB, np.uint8)
        self.p_out, self.cap = self.out.ctypes.data, self.out.size
        self.size = C.c_int64(-7)
        self.p_size = C.byref(self.size)
        self.rects = np.full((2, 4), -9, np.int32)

    def run(self, L, symbol):
        src = (C.c_void_p * len(self.ptrs))(*self.ptrs) if self.table else None
        args = [self.device] + ([None] if symbol.endswith("_device") else [])
        return getattr(L, symbol)(*args, self.n, src, self.w, self.h, self.p_pal, self.K, self.p_delays, self.loop, self.band_bits, self.delta,
                                  self.p_out, self.cap, self.p_size, self.rects.ctypes.data)

    def untouched(self):
        return self.size.value == -7 and (self.out == 0xAB).all() and (self.rects == -9).all()


def _spoilers():
    def setter(**kw):
        def f(c):
            for k, v in kw.items():
                setattr(c, k, v)
        return f

    def delay(i, v):
        def f(c):
            c.delays[i] = v
        return f

    def pointer(i, v):
        def f(c):
            c.ptrs[i] = v if v is None else c.ptrs[i] + v
        return f

    return [("n = 0", setter(n=0)), ("n < 0", setter(n=-2)), ("n = 65536", setter(n=65536)), ("width 0", setter(w=0)),
            ("width 16385", setter(w=16385)), ("height 0", setter(h=0)), ("height 16385", setter(h=16385)), ("negative height", setter(h=-4)),
            ("K = 0", setter(K=0)), ("K = 257", setter(K=257)), ("delay -1", delay(1, -1)), ("delay 65536", delay(0, 65536)),
            ("loop -1", setter(loop=-1)), ("loop 65536", setter(loop=65536)), ("delta 2", setter(delta=2)), ("delta -1", setter(delta=-1)),
            ("band_bits 1", setter(band_bits=1)), ("band_bits 10", setter(band_bits=10)), ("band_bits -2", setter(band_bits=-2)),
            ("band_bits 9 at 100 packed pixels", setter(w=100, K=17, band_bits=9)),
            ("8193 packed pixels", setter(w=8193, K=17)), ("16384 packed pixels at K = 256", setter(w=16384, K=256)),
            ("16384 packed pixels at K = 17", setter(w=16384, K=17)),
            ("NULL table", setter(table=False)), ("NULL frame", pointer(1, None)), ("odd frame pointer", pointer(0, 1)),
            ("NULL palette", setter(p_pal=None)), ("NULL out_size", setter(p_size=None)), ("NULL out", setter(p_out=None)),
            ("cap < 0", setter(cap=-1)), ("negative device", setter(device=-1))]


@pytest.mark.parametrize("symbol", SYMBOLS[1:])
def test_invalid_arguments_are_refused_before_any_device(nq, symbol):
    L = nq.load_library()
    for what, spoil in _spoilers():
        c = _Call()
        spoil(c)
        assert c.run(L, symbol) == -1, what
        assert c.untouched(), what
        assert all((m == 0).all() for m in c.maps), what
        assert L.nq_last_error(None), what


def test_the_widest_frames_the_bundling_allows_pass_the_checks(nq):
    """8192 packed pixels is the limit: 16384 wide at K = 16, 8192 wide at K = 256.  Without a device the call gets past the checks
    to NQ_ERR_NO_DEVICE; with one, tests/test_gpu_webp.py runs valid calls."""
    if conftest.HAS_GPU:
        return
    L = nq.load_library()
    for w, K in ((16384, 16), (8192, 256)):
        c = _Call()
        c.w, c.h, c.K, c.n = w, 1, K, 1
        c.maps = [np.zeros((1, w), np.uint16)]
        c.ptrs = [c.maps[0].ctypes.data]
        c.pal = np.full(K, 0xFF000000, np.uint32)
        c.p_pal = c.pal.ctypes.data
        assert c.run(L, "nq_encode_webp") == -5 and c.untouched()


def test_the_widest_frame_one_palette_entry_too_many_is_refused_and_the_next_call_is_what_it_was(nq):
    """full_chain_K16 is 16384 wide at K = 16; at K = 17 nothing is bundled and the same width is 16384 packed pixels.  The refusal
    leaves no state behind: the same call at K = 16 gets as far as it did before (here: to the device that is not there;
    tests/test_gpu_webp.py encodes it)."""
    L = nq.load_library()
    _, frames, _, _ = webp_cases.case("full_chain_K16")

    def call(K):
        c = _Call()
        c.w, c.h, c.K, c.n = 16384, 9, K, 1
        c.maps = [np.ascontiguousarray(frames[0], np.uint16)]
        c.ptrs = [c.maps[0].ctypes.data]
        c.pal = np.full(K, 0xFF000000, np.uint32)
        c.p_pal = c.pal.ctypes.data
        return c.run(L, "nq_encode_webp"), c

    rc, c = call(17)
    assert rc == -1 and c.untouched() and b"packed width 16384" in L.nq_last_error(None)
    if not conftest.HAS_GPU:
        rc, c = call(16)
        assert rc == -5 and c.untouched()


def test_max_bytes_refuses_bad_shapes(nq):
    L = nq.load_library()
    out = C.c_int64(-7)
    for n, w, h, p in ((0, 4, 4, 0), (65536, 4, 4, 0), (1, 0, 4, 0), (1, 4, 16385, 0), (1, 4, 4, 1), (1, 4, 4, 10), (1, 65537, 4, 0),
                       (1, 16384, 4, 9)):
        assert L.nq_webp_max_bytes(n, w, h, p, C.byref(out)) == -1 and out.value == -7, (n, w, h, p)
    assert L.nq_webp_max_bytes(1, 4, 4, 0, None) == -1
    assert L.nq_webp_max_bytes(1, 16384, 4, 2, C.byref(out)) == 0 and out.value == webp_ref.max_bytes(1, 16384, 4, 2)


@pytest.mark.parametrize("symbol", SYMBOLS[1:])
def test_valid_arguments_need_a_device(nq, symbol):
    if conftest.HAS_GPU:
        return              # a device is present: tests/test_gpu_webp.py runs the valid calls (a device form must not see host memory)
    L = nq.load_library()
    c = _Call()
    assert c.run(L, symbol) == -5
    assert c.untouched() and b"no HIP device" in L.nq_last_error(None)
