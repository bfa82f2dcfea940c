"""CPU-side checks of the PNG encoder (include/nquant_abi.h "PNG encoding"): the restatement in png_ref.py writes files whose IDAT
Python's zlib inflates to the expected raw stream, whose chunk CRCs verify and which Pillow opens as the same palette image (so the
bytes the GPU tests compare against are right); nq_png_max_bytes bounds them; the Python wrappers exist; without a HIP device the host
form refuses to compute (no CPU fallback)."""
import io
import zlib

import numpy as np
import pytest

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
    """Symbol counts that grow like Fibonacci numbers: Huffman's tree is deeper than 15 (and the code-length code's deeper than 7),
    so the length limit of the construction is exercised."""
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
