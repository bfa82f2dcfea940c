"""Numpy restatement of the temporal hold (include/nquant_abi.h "temporal hold"), independent of the library: vectorised
over the pixels, a loop over the frames.  hold() is what the GPU tests compare against, bit for bit.  noisy_sprite_sequence() is the
footage-like input of the end-to-end tests: a still background with +-2 of noise per channel and frame, and a small sprite moving
over it."""
import numpy as np

from nquant.android_amd import synth


def distance(c, a):
    """Largest |difference| of the four 8-bit channels of two arrays of ARGB words."""
    c = np.asarray(c).astype(np.int64) & 0xFFFFFFFF
    a = np.asarray(a).astype(np.int64) & 0xFFFFFFFF
    d = np.zeros(c.shape, np.int64)
    for s in (24, 16, 8, 0):
        d = np.maximum(d, np.abs(((c >> s) & 255) - ((a >> s) & 255)))
    return d


def hold(frames, indices, threshold, outs=None):
    """frames: n ARGB arrays; indices: their n index maps; outs: their n ARGB outputs or None; all of one shape.  Returns
    (held index maps, held counts as n ints, held outputs or None); the inputs are not modified."""
    n = len(frames)
    idx = [np.array(a, copy=True) for a in indices]
    out = None if outs is None else [np.array(o, copy=True) for o in outs]
    held = [0] * n
    anchor = np.array(frames[0], copy=True)
    for i in range(1, n):
        c = np.asarray(frames[i])
        keep = distance(c, anchor) <= threshold
        idx[i][keep] = idx[i - 1][keep]
        if out is not None:
            out[i][keep] = out[i - 1][keep]
        held[i] = int(keep.sum())
        anchor = np.where(keep, anchor, c)
    return idx, held, out


SPRITE, STEP = 12, 5


def noisy_sprite_sequence(h, w, n, seed):
    """n opaque ARGB frames (int32, h x w): synth.gradient_noise with r, g, b clamped to 2..253, plus independent uniform integer noise in
    -2..+2 on r, g, b of every pixel of every frame, plus a SPRITE x SPRITE square of one saturated colour that moves STEP pixels per
    frame along x (and 2 along y) and whose every channel is at least 64 away from any background value under it.  Returns
    (frames, boxes) with boxes[i] = (x, y, w, h) of the sprite in frame i."""
    rng = np.random.default_rng(seed)
    base = synth.gradient_noise(w, h, seed).view(np.uint32).astype(np.int64)
    ch = [np.clip((base >> s) & 255, 2, 253) for s in (16, 8, 0)]
    boxes = [(7 + STEP * i, 9 + 2 * i, SPRITE, SPRITE) for i in range(n)]
    assert boxes[-1][0] + SPRITE <= w and boxes[-1][1] + SPRITE <= h, "the sprite leaves the frame"
    x0, y0, x1, y1 = boxes[0][0], boxes[0][1], boxes[-1][0] + SPRITE, boxes[-1][1] + SPRITE
    colour = []
    for c in ch:                                    # background + noise under the sprite's path lies in [lo - 2, hi + 2]
        lo, hi = int(c[y0:y1, x0:x1].min()), int(c[y0:y1, x0:x1].max())
        assert hi + 2 <= 255 - 64 or lo - 2 >= 64, "no saturated value is 64 away from this background"
        colour.append(255 if hi + 2 <= 255 - 64 else 0)
    frames = []
    for i in range(n):
        f = [c + rng.integers(-2, 3, (h, w)) for c in ch]
        x, y, sw, sh = boxes[i]
        for c, v in zip(f, colour):
            c[y:y + sh, x:x + sw] = v
        frames.append(((255 << 24) | (f[0] << 16) | (f[1] << 8) | f[2]).astype(np.uint32).view(np.int32))
    return frames, boxes


def union_mask(h, w, *boxes):
    m = np.zeros((h, w), bool)
    for x, y, bw, bh in boxes:
        m[y:y + bh, x:x + bw] = True
    return m
