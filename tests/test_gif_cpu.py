"""CPU-side checks of the GIF encoder (include/nquant_abi.h "GIF encoding"): the restatement in gif_ref.py is a GIF that Pillow reads
back exactly (so the bytes the GPU tests compare against are right), nq_gif_max_bytes bounds it, the Python wrappers exist, and
without a HIP device the host form refuses to compute (no CPU fallback)."""
import io

import numpy as np
import pytest

import gif_ref
from conftest import HAS_GPU

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402


def _content(kind, h, w, K, rng):
    if kind == "noise":
        return rng.integers(0, K, (h, w))
    if kind == "flat":
        return np.full((h, w), K - 1)
    return (np.arange(h * w).reshape(h, w) // 5) % K


CASES = [(K, shape, S, kind) for K in (2, 3, 5, 16, 256) for shape in ((1, 1), (1, 333), (37, 91)) for S in (1, 7, 0, 1 << 20)
         for kind in ("noise", "flat", "gradient")]


def test_restatement_round_trips_through_pillow():
    rng = np.random.default_rng(5)
    for K, (h, w), S, kind in CASES:
        idx = _content(kind, h, w, K, rng)
        pal = (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.int64)
        gif = gif_ref.encode(idx, pal, segment_pixels=S)
        im = Image.open(io.BytesIO(gif))
        im.load()
        assert im.mode == "P" and (np.array(im) == idx).all(), (K, h, w, S, kind)
        assert (gif_ref.parse(gif)[2][0]["index"] == idx).all()


def test_restatement_fills_the_table_many_times():
    """Noise at K = 256 in one chain of 65536 pixels resets the 4096-entry table many times; the last-code width bump is exercised
    by every segment length."""
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 256, (256, 256))
    pal = 0xFF000000 | np.arange(256)
    for S in (4096, 65536, 3000):
        gif = gif_ref.encode(idx, pal, segment_pixels=S)
        im = Image.open(io.BytesIO(gif))
        im.load()
        assert (np.array(im) == idx).all(), S


def test_restatement_animation_layout():
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 16, (40, 60)) for _ in range(3)]
    pal = 0xFF000000 | (np.arange(16) * 0x0F0F0F)
    gif = gif_ref.encode(frames, pal, delays_cs=[5, 7, 9], loop=0)
    im = Image.open(io.BytesIO(gif))
    assert im.n_frames == 3 and im.info["loop"] == 0
    for i, f in enumerate(frames):
        im.seek(i)
        assert im.info["duration"] == 50 + 20 * i
    screen, gct, parsed = gif_ref.parse(gif)
    assert screen["width"] == 60 and screen["height"] == 40 and len(gct) == 3 * 16
    assert [p["disposal"] for p in parsed] == [2, 2, 2]
    for p, f in zip(parsed, frames):
        assert (p["index"] == f).all()
    # one frame whose palette has an alpha-0 entry at 7
    pal = (0xFF000000 | np.arange(16) * 0x111111).astype(np.int64)
    pal[7] = 0x00123456
    gif = gif_ref.encode(frames[0], pal)
    im = Image.open(io.BytesIO(gif))
    im.load()
    assert im.info["transparency"] == 7 and (np.array(im) == frames[0]).all()


def test_max_bytes_is_exported_and_bounds_the_restatement(nq):
    L = nq.load_library()
    assert hasattr(L, "nq_gif_max_bytes") and "nq_gif_max_bytes" in nq.abi_symbols()
    rng = np.random.default_rng(11)
    for K, (h, w), S, kind in CASES:
        idx = _content(kind, h, w, K, rng)
        gif = gif_ref.encode(idx, 0xFF000000 | np.arange(K), segment_pixels=S)
        assert nq.gif_max_bytes([w], [h], K, S) >= len(gif), (K, h, w, S, kind)
    frames = [rng.integers(0, 256, (64, 64)), rng.integers(0, 256, (17, 99))]
    gif = gif_ref.encode(frames, 0xFF000000 | np.arange(256), delays_cs=[1, 2], segment_pixels=1)
    assert nq.gif_max_bytes([64, 99], [64, 17], 256, 1) >= len(gif)
    # pure arithmetic: the argument checks need no device
    for args in (([1], [1], 0, 0), ([1], [1], 257, 0), ([0], [1], 2, 0), ([65536], [1], 2, 0), ([1], [1], 2, -1), ([], [], 2, 0)):
        with pytest.raises(nq.NqError):
            nq.gif_max_bytes(*args)


def test_gif_wrappers_are_exported(nq):
    for name in ("encode_gif", "encode_gif_device", "write_gif", "convert_frames_to_gif", "gif_max_bytes"):
        assert callable(getattr(nq, name)), name
    L = nq.load_library()
    for name in ("nq_gif_max_bytes", "nq_encode_gif_device", "nq_encode_gif"):
        assert name in nq.abi_symbols() and hasattr(L, name), name


def test_gif_python_argument_checks(nq):
    with pytest.raises(ValueError):
        nq.encode_gif([], [0xFF000000])
    with pytest.raises(ValueError):
        nq.encode_gif([np.zeros(16, np.uint16)], [0xFF000000])
    with pytest.raises(TypeError):
        nq.encode_gif([np.zeros((4, 4), np.float32)], [0xFF000000])
    with pytest.raises(ValueError):
        nq.convert_frames_to_gif(1, [np.zeros((4, 4), np.int32)], 257, True)


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_encode_gif_has_no_cpu_fallback(nq):
    with pytest.raises(nq.NqError) as e:
        nq.encode_gif(np.zeros((8, 8), np.uint16), [0xFF000000, 0xFFFFFFFF])
    assert e.value.status == -5
    with pytest.raises(nq.NqError) as e:
        nq.convert_frames_to_gif(0, [np.full((8, 8), -1, np.int32)], 16, False)
    assert e.value.status == -5
