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


# One grid stride of the difference and body kernels is 1024 workgroups x 256 threads x 8 pixels = 2 097 152 pixels.  1449 x 1450 is
# 2 101 050 pixels with an odd width, and its rows 1448 and 1449 lie wholly behind pixel 2 097 152 (1448 * 1449 = 2 098 152).
STRIDE_PIXELS = 1024 * 256 * 8
BIG_H, BIG_W = 1450, 1449


def past_one_grid_stride(K, rng):
    """Six 1449 x 1450 frames (uint16) whose changes sit on both sides of the first grid stride: 1 changes only the last pixel
    (x 1448, y 1449); 2 changes pixel (0, 0) and the last pixel, so its rectangle is the whole frame and its body exceeds one stride; 3
    changes a block inside the first 100 rows; 4 a block inside rows 1448 .. 1449 that reaches neither side edge; 5 equals 4.  Only
    frames 0 and 2 are full-size bodies.  Inside the two blocks some pixels keep their index."""
    h, w = BIG_H, BIG_W
    assert h * w > STRIDE_PIXELS and w % 2 == 1 and (h - 2) * w >= STRIDE_PIXELS
    f = [rng.integers(0, K, (h, w)).astype(np.uint16)]

    def step(edit):
        g = f[-1].copy()
        edit(g)
        f.append(g)

    def bump(g, y, x):
        g[y, x] = (g[y, x] + 1) % K

    def block(g, y0, y1, x0, x1):
        g[y0:y1, x0:x1] = rng.integers(0, K, (y1 - y0, x1 - x0))
        for y, x in ((y0, x0), (y1 - 1, x1 - 1)):              # the corners change for certain
            g[y, x] = (f[-1][y, x] + 1) % K

    step(lambda g: bump(g, h - 1, w - 1))
    step(lambda g: (bump(g, 0, 0), bump(g, h - 1, w - 1)))
    step(lambda g: block(g, 13, 71, 101, 340))
    step(lambda g: block(g, h - 2, h, 5, w - 9))
    step(lambda g: None)
    return f


BIG_RECTS = [(0, 0, BIG_W, BIG_H), (BIG_W - 1, BIG_H - 1, 1, 1), (0, 0, BIG_W, BIG_H), (101, 13, 239, 58), (5, BIG_H - 2, BIG_W - 14, 2),
             (0, 0, 1, 1)]

# gridDim.y of the same kernels is capped at 65 535, one frame pair each: with 65 540 frames the pairs 65 535 .. 65 538 (bodies of frames
# 65 536 .. 65 539) are the second step of blockIdx.y = 0 .. 3.
GRID_Y = 65535
MANY_FRAMES = 65540
ROWS = np.array([[0, 1, 2], [2, 1, 0], [1, 1, 1], [0, 0, 2], [2, 0, 1], [3, 1, 2], [0, 3, 3], [2, 1, 3]], np.uint16)   # 3 x 1 frames
ROWS_BELOW_3 = 5                                    # the first five hold no index 3


def many_rows(n, rng, K_of=None):
    """Which of ROWS frame i shows, for n frames in a seeded random order: most neighbours differ and some are equal.  K_of(i) < 4:
    frame i draws from the rows without an index 3."""
    pick = rng.integers(0, len(ROWS), n)
    if K_of is not None:
        low = rng.integers(0, ROWS_BELOW_3, n)
        pick = np.where(np.array([K_of(i) for i in range(n)]) < 4, low, pick)
    same = int((pick[1:] == pick[:-1]).sum())
    assert 0 < same < n // 4
    return pick


def device_pool(rows):
    """(torch buffer, its host copy, device pointers): the rows in ONE device buffer, every one at an odd uint16 offset that differs
    modulo 16 bytes from row to row, sentinels in between."""
    import torch
    offs, off = [], 1
    for i, r in enumerate(rows):
        offs.append(off)
        off += r.size + 2 * (i % 5) + 1
        off += 1 - off % 2
    host = np.full(off + 8, 0xFFFF, np.uint16)
    for r, o in zip(rows, offs):
        host[o:o + r.size] = np.asarray(r).reshape(-1)
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    ptrs = [buf.data_ptr() + 2 * o for o in offs]
    assert all(p % 4 == 2 for p in ptrs) and len({p % 16 for p in ptrs}) > 1
    return buf, host, ptrs


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
