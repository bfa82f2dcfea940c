"""What the delta-mode GIF tests of both suites share: the K values, a frame sequence that meets every case of the definition, and the
canvases Pillow shows for a file."""
import io

import numpy as np

KS = (2, 3, 4, 15, 16, 17, 128, 255, 256)


def sequence(h, w, K, rng):
    """Frames that meet every case of the definition: an identical frame, a frame that changes everywhere, one changed pixel in each
    corner, changes in the last row only and in the last column only, and a block in the middle."""
    f = [rng.integers(0, K, (h, w))]

    def step(edit):
        g = f[-1].copy()
        edit(g)
        f.append(g)

    def bump(g, ys, xs):
        g[ys, xs] = (g[ys, xs] + 1) % K

    step(lambda g: None)
    step(lambda g: bump(g, slice(None), slice(None)))
    step(lambda g: bump(g, 0, 0))
    step(lambda g: bump(g, 0, w - 1))
    step(lambda g: bump(g, h - 1, 0))
    step(lambda g: bump(g, h - 1, w - 1))
    step(lambda g: bump(g, h - 1, slice(None)))
    step(lambda g: bump(g, slice(None), w - 1))
    step(lambda g: bump(g, slice(h // 3, h // 3 + max(1, h // 4)), slice(w // 2, w // 2 + max(1, w // 5))))
    step(lambda g: (bump(g, h // 2, w // 4), bump(g, h // 4, w // 2)))
    return f


def palette_of(K, rng):
    return (0xFF000000 | rng.integers(0, 1 << 24, K)).astype(np.int64)


def pillow_canvases(gif):
    """The RGB canvas Pillow shows for every frame."""
    from PIL import Image
    im = Image.open(io.BytesIO(gif))
    out = []
    for i in range(im.n_frames):
        im.seek(i)
        out.append(np.array(im.convert("RGB")))
    return out


def rgb_of(frame, pal):
    c = np.asarray(pal).astype(np.int64)[np.asarray(frame)]
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8)
