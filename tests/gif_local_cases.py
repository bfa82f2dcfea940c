"""What the local-colour-table GIF tests of both suites share: gif_delta_cases.sequence paired with one palette per frame, the named edge
cases of the definition, and the RGB every frame shows."""
import numpy as np

from gif_delta_cases import palette_of, sequence

# every K of the definition's cases in one file (m runs from 2 to 8); the first two frames share a palette, so frame 1, which
# sequence() leaves identical, has an empty D; a 256 frame (no u) is followed by a 255 frame (u = 255)
MIXED_KS = (17, 17, 256, 255, 1, 2, 3, 4, 5, 16, 128)
SHORT_KS = (17, 17, 256, 255, 3, 128)              # the same idea for the large shapes


def near_palette(K, rng):
    """Opaque colours close to one another (some of them equal): a small `lossy` finds candidates."""
    return (0xFF000000 | (0x40 + rng.integers(0, 24, K)) << 16 | (0x80 + rng.integers(0, 24, K)) << 8 | (0x20 + rng.integers(0, 8, K))).astype(np.int64)


def mixed(h, w, rng, ks=MIXED_KS, near=False):
    """(frames, palettes): sequence()'s frames, frame i reduced modulo ks[i]; consecutive equal K share one palette, and every new palette
    takes the first half of its entries from the one before, so a pixel can keep its colour across a change of tables."""
    seq = sequence(h, w, 256, rng)
    assert len(ks) <= len(seq)
    make = near_palette if near else palette_of
    frames, palettes = [], []
    for i, K in enumerate(ks):
        frames.append(seq[i] % K)
        if i and K == ks[i - 1]:
            palettes.append(palettes[-1])
            continue
        pal = make(K, rng)
        if i:
            keep = min(K, ks[i - 1]) // 2
            pal[:keep] = palettes[-1][:keep]
        palettes.append(pal)
    return frames, palettes


def rgb_of(frame, pal):
    c = np.asarray(pal).astype(np.int64)[np.asarray(frame)]
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8)


def shown(frames, palettes):
    return [rgb_of(f, p) for f, p in zip(frames, palettes)]


def permuted(h, w, K, rng):
    """Frame 1's palette is a permutation of frame 0's (all colours distinct) and its indices are permuted to match: every index differs,
    no colour does."""
    pal = palette_of(K, rng)
    assert len(set((pal & 0xFFFFFF).tolist())) == K
    perm = np.roll(np.arange(K), 1)                  # entry perm[j] of the new palette is entry j of the old: no fixed point
    a = rng.integers(0, K, (h, w))
    pal2 = np.empty_like(pal)
    pal2[perm] = pal
    return [a, perm[a]], [pal, pal2]


def edge_cases(rng):
    """name -> (frames, palettes, expected rectangles or None) for the named cases of the definition."""
    out = {}
    f, p = permuted(19, 31, 17, rng)
    assert (f[0] != f[1]).all()
    out["permutation"] = (f, p, [(0, 0, 31, 19), (0, 0, 1, 1)])
    # two entries of one palette have equal RGB: a pixel that moves between them is unchanged
    pal = palette_of(9, rng)
    pal[4] = pal[2]
    a = rng.integers(0, 9, (19, 31))
    a[3, 5], a[7, 11] = 2, 0
    b = a.copy()
    b[3, 5] = 4
    b[7, 11] = 1
    out["equal rgb"] = ([a, b], [pal, pal], [(0, 0, 31, 19), (11, 7, 1, 1)])
    # two colours that differ in alpha only are unchanged
    pal2 = pal.copy()
    pal2[:] = (pal & 0xFFFFFF) | 0x80000000
    out["alpha only"] = ([a, a.copy()], [pal, pal2], [(0, 0, 31, 19), (0, 0, 1, 1)])
    # u exists on one side only
    for name, ks in (("256 after 255", (255, 256)), ("255 after 256", (256, 255))):
        pals = [palette_of(ks[0], rng), palette_of(ks[1], rng)]
        pals[1][:200] = pals[0][:200]
        c = rng.integers(0, 255, (19, 31))
        d = c.copy()
        d[2:9, 4:20] = ks[1] - 1
        out[name] = ([c, d], pals, None)
    return out
