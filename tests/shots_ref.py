"""Numpy restatement of shot detection (include/nquant_abi.h "shot detection"), independent of the library: signatures
with np.bincount, the score with np.cumsum, the rule as the loop it is.  What the CPU tests compare nq_shots_from_signatures with and
the GPU tests compare the signature kernel with, bit for bit.  sprite_cut_clip() and slide_show() are the two clips both use."""
import os

import numpy as np

import hold_ref
from nquant.android_amd import synth

SHIFTS = (24, 16, 8, 0)                             # a, r, g, b


def signature(frame):
    """(4, 256) uint32: [c, v] = pixels of the ARGB frame whose channel c has the value v."""
    p = np.asarray(frame).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    return np.stack([np.bincount((p >> s) & 255, minlength=256) for s in SHIFTS]).astype(np.uint32)


def signatures(frames):
    return np.stack([signature(f) for f in frames])


def score(a, b, npix):
    """Per mille: the largest 1-D earth mover's distance of the four channels over its largest possible value, rounded down."""
    d = np.asarray(a).astype(np.int64).reshape(4, 256) - np.asarray(b).astype(np.int64).reshape(4, 256)
    e = np.abs(np.cumsum(d, axis=1)[:, :255]).sum(axis=1)
    return int(1000 * int(e.max()) // (255 * int(npix)))


def shots(sig, npix, threshold_pm, min_shot):
    """(starts, scores) of the anchor rule over the signatures sig[0 .. n - 1]."""
    anchor, starts, scores = 0, [0], [0]
    for i in range(1, len(sig)):
        scores.append(score(sig[i], sig[anchor], npix))
        if scores[i] > threshold_pm and i - anchor >= min_shot:
            starts.append(i)
            anchor = i
    return starts, scores


def detect(frames, threshold_pm, min_shot):
    return shots(signatures(frames), np.asarray(frames[0]).size, threshold_pm, min_shot)


def rotate_channels(frame):
    """r <- g, g <- b, b <- r; alpha stays."""
    p = np.asarray(frame).view(np.uint32)
    r, g, b = (p >> 16) & 255, (p >> 8) & 255, p & 255
    return ((p & np.uint32(0xFF000000)) | (g << 16) | (b << 8) | r).astype(np.uint32).view(np.int32)


def sprite_cut_clip():
    """8 frames of 128 x 96: the noisy sprite sequence (hold_ref) and the same four frames with the channels rotated -- one cut, at 4."""
    frames, _ = hold_ref.noisy_sprite_sequence(96, 128, 4, 3)
    return frames + [rotate_channels(f) for f in frames]


def slide_show():
    """7 frames of 128 x 96: two gradients, two overlapping crops of the sample photo, a channel-rotated third, one crop twice."""
    rgb = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_495x438.npz"))["rgb"]
    photo = synth.tile_photo(rgb, 990, 876)
    crop = lambda y, x: np.ascontiguousarray(photo[y:y + 96, x:x + 128])      # (row, column) of the corner
    return [synth.gradient_noise(128, 96, 1), synth.gradient_noise(128, 96, 2), crop(0, 60), crop(10, 76), rotate_channels(crop(20, 92)),
            crop(300, 300), crop(300, 300)]
