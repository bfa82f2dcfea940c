"""Shot detection: where a frame sequence needs a new palette (nq_frame_signatures / nq_shots_from_signatures / nq_detect_shots,
include/nquant_abi.h "shot detection").  A frame's signature is the four 256-bin histograms of its a, r, g, b channels (1024 counts,
computed on the GPU); the score of two signatures is the largest 1-D earth mover's distance of the four channels in per mille of the
full range; a shot ends when a frame scores above `cut` against the shot's FIRST frame and the shot is at least `min_shot` frames long.
The starts are what convert_shots_to_gif takes as shot_starts; convert_clip_to_gif (gif.py) does both.
cut=60 and min_shot=8 are interface choices (DESIGN.md 5b "Shot detection"): camera noise, moving objects and slow pans stay below
60; a hard cut between two scenes is far above it.
The signatures have no CPU fallback: without a HIP device those calls raise NqError with status -5 (NQ_ERR_NO_DEVICE).
shots_from_signatures is host arithmetic and needs no device."""
import ctypes as C

import numpy as np

from .gif import _Handle
from .host import NqError, _as_i32, load_library

SIG_WORDS = 1024


def _frames(frames):
    frames = [np.ascontiguousarray(_as_i32(f)) for f in frames]
    if len(frames) == 0:
        raise ValueError("no frames")
    if len({f.shape for f in frames}) != 1 or frames[0].ndim != 2:
        raise ValueError("shot detection: the frames must be 2-D arrays of one size, got %s" % sorted({f.shape for f in frames}))
    return frames


def _ptr_array(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[int(p) for p in ptrs])


def _signatures(L, handle, check, entry, ptrs, width, height):
    sig = np.zeros((max(len(ptrs), 1), 4, 256), np.uint32)
    check(getattr(L, entry)(handle, len(ptrs), _ptr_array(ptrs), int(width), int(height), sig.ctypes.data))
    return sig[:len(ptrs)]


def _detect(L, handle, check, entry, ptrs, width, height, cut, min_shot):
    """One nq_detect_shots* call.  Returns (starts as a list of ints, scores as n int32 values)."""
    n = len(ptrs)
    starts = np.zeros(max(n, 1), np.int32)
    scores = np.zeros(max(n, 1), np.int32)
    count = C.c_int32(0)
    check(getattr(L, entry)(handle, n, _ptr_array(ptrs), int(width), int(height), int(cut), int(min_shot), starts.ctypes.data, C.byref(count),
                            scores.ctypes.data))
    return starts[:count.value].tolist(), scores[:n]


def _detect_host(L, handle, check, frames, cut, min_shot):
    """nq_detect_shots of int32 frames of one size on an open handle."""
    height, width = frames[0].shape
    return _detect(L, handle, check, "nq_detect_shots", [f.ctypes.data for f in frames], width, height, cut, min_shot)


def frame_signatures(frames, device=0):
    """nq_frame_signatures on host arrays: `frames` are 2-D int32/uint32 ARGB_8888 arrays of one size.  Returns an (n, 4, 256) uint32
    array: [i, c, v] = pixels of frame i whose channel c (0..3: a, r, g, b) has the value v."""
    frames = _frames(frames)
    height, width = frames[0].shape
    hd = _Handle(device)
    try:
        return _signatures(hd._L, hd._h, hd._check, "nq_frame_signatures", [f.ctypes.data for f in frames], width, height)
    finally:
        hd.close()


def frame_signatures_device(q, d_argb_ptrs, width, height):
    """nq_frame_signatures_device on the handle of quantizer `q`: d_argb_ptrs[i] is the HIP device address of frame i (width x height
    ARGB pixels, 4-byte aligned; 16-byte aligned frames take the fast path; never written).  Returns the (n, 4, 256) uint32 array."""
    if len(d_argb_ptrs) == 0:
        raise ValueError("no frames")
    return _signatures(q._L, q._h, q._check, "nq_frame_signatures_device", list(d_argb_ptrs), width, height)


def shots_from_signatures(sig, npix, cut=60, min_shot=8):
    """nq_shots_from_signatures (no device needed): `sig` the (n, 4, 256) signatures of frames with npix pixels.  Returns
    (starts, scores): the frame numbers at which a shot begins (starts[0] = 0) and, per frame, the score in per mille against the
    first frame of the shot it was compared with (scores[0] = 0)."""
    sig = np.ascontiguousarray(sig, np.uint32)
    if sig.size == 0 or sig.size % SIG_WORDS:
        raise ValueError("signatures hold %d counts per frame, got an array of %d" % (SIG_WORDS, sig.size))
    n = sig.size // SIG_WORDS
    starts = np.zeros(n, np.int32)
    scores = np.zeros(n, np.int32)
    count = C.c_int32(0)
    rc = load_library().nq_shots_from_signatures(sig.ctypes.data, n, int(npix), int(cut), int(min_shot), starts.ctypes.data, C.byref(count),
                                                 scores.ctypes.data)
    if rc != 0:
        raise NqError(rc, "invalid arguments: cut must be 0..1000, min_shot at least 1, and every channel of every signature must sum "
                          "to npix (cut=%r, min_shot=%r, npix=%r)" % (cut, min_shot, npix))
    return starts[:count.value].tolist(), scores


def detect_shots(frames, cut=60, min_shot=8, device=0):
    """nq_detect_shots on host arrays (2-D int32/uint32 ARGB_8888 frames of one size): the signatures on the GPU, then the rule.
    Returns (starts, scores) as shots_from_signatures does."""
    frames = _frames(frames)
    hd = _Handle(device)
    try:
        return _detect_host(hd._L, hd._h, hd._check, frames, cut, min_shot)
    finally:
        hd.close()


def detect_shots_device(q, d_argb_ptrs, width, height, cut=60, min_shot=8):
    """nq_detect_shots_device on the handle of quantizer `q`; frames as for frame_signatures_device.  Returns (starts, scores)."""
    if len(d_argb_ptrs) == 0:
        raise ValueError("no frames")
    return _detect(q._L, q._h, q._check, "nq_detect_shots_device", list(d_argb_ptrs), width, height, cut, min_shot)
