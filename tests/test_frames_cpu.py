"""CPU-side checks of the frames entry points (one palette for a sequence of frames): the Python wrappers and the C entry points
exist, and without a HIP device the host form refuses to compute (no CPU fallback)."""
import numpy as np
import pytest

from conftest import HAS_GPU


def test_frames_wrappers_are_exported(nq):
    for name in ("convert_frames", "convert_frames_device", "pnnquan_frames_device"):
        assert callable(getattr(nq, name)), name
    L = nq.load_library()
    for name in ("nq_pnnquan_frames_device", "nq_convert_frames_device", "nq_convert_frames"):
        assert name in nq.abi_symbols() and hasattr(L, name), name


def test_convert_frames_argument_checks(nq):
    with pytest.raises(ValueError):
        nq.convert_frames(1, [], 256, True)
    with pytest.raises(ValueError):
        nq.convert_frames(1, [np.zeros(16, np.int32)], 256, True)
    with pytest.raises(TypeError):
        nq.convert_frames(1, [np.zeros((4, 4), np.float32)], 256, True)


@pytest.mark.skipif(HAS_GPU, reason="checks the no-device error path")
def test_convert_frames_has_no_cpu_fallback(nq):
    frames = [np.full((8, 8), -1, np.int32), np.full((5, 7), -16777216, np.int32)]
    with pytest.raises(nq.NqError) as e:
        nq.convert_frames(1, frames, 256, True, seeds=[1, 2])
    assert e.value.status == -5
    with pytest.raises(nq.NqError) as e:
        nq.convert_frames(0, frames, 16, False)
    assert e.value.status == -5
