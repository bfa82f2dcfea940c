"""The palette refinement of include/nquant_abi.h ("palette refinement") restated in numpy: a brute-force distance matrix, argmin
(first minimum = lowest index) and bincount.  Written from the definition; the reference project has no such step."""
import numpy as np

CHUNK = 1 << 15          # pixels per distance matrix


def _channels(v):
    v = np.asarray(v).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    return np.stack([(v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1)


def dist(p, c):
    """d[i][j] = da^2 + dr^2 + dg^2 + db^2 of pixel i and entry j ((n, 4) and (m, 4) channel arrays) as int64.  Expanded to
    |p|^2 + |c|^2 - 2 p.c so that the product is one float64 matrix multiplication: every term is an integer below 2^20, exact."""
    pf, cf = p.astype(np.float64), c.astype(np.float64)
    return ((pf * pf).sum(axis=1)[:, None] + (cf * cf).sum(axis=1)[None, :] - 2.0 * (pf @ cf.T)).astype(np.int64)


def assign(pixels, palette):
    """One assignment pass: (cnt[K], sums[K][3] of r, g, b, sse) of the flat pixel sequence under the palette, all int64."""
    pal = _channels(palette)
    K = pal.shape[0]
    live = np.flatnonzero(pal[:, 0] != 0)
    cnt = np.zeros(K, np.int64)
    sums = np.zeros((K, 3), np.int64)
    sse = 0
    px = _channels(pixels)
    px = px[px[:, 0] != 0]
    if live.size == 0:
        return cnt, sums, sse
    for s in range(0, px.shape[0], CHUNK):
        p = px[s:s + CHUNK]
        d = dist(p, pal[live])
        j = d.argmin(axis=1)
        k = live[j]
        sse += int(d[np.arange(p.shape[0]), j].sum())
        cnt += np.bincount(k, minlength=K)
        for c in range(3):
            sums[:, c] += np.bincount(k, weights=p[:, 1 + c], minlength=K).astype(np.int64)      # (at most 255 * CHUNK: exact in float64)
    return cnt, sums, sse


def update(palette, cnt, sums):
    """The update step: entries with cnt > 0 move to the rounded mean (half rounds up) of r, g, b; alpha never changes."""
    pal = (np.asarray(palette).reshape(-1).astype(np.int64) & 0xFFFFFFFF).copy()
    for k in np.flatnonzero(cnt > 0):
        c = [(2 * int(sums[k, i]) + int(cnt[k])) // (2 * int(cnt[k])) for i in range(3)]
        pal[k] = (pal[k] & 0xFF000000) | c[0] << 16 | c[1] << 8 | c[2]
    return pal.astype(np.uint32)


def _flat(f):
    f = np.asarray(f)
    return f.reshape(-1).view(np.uint32) if f.dtype == np.int32 else f.reshape(-1)


def refine(frames, palette, iterations):
    """(palette as uint32, sse as iterations + 1 int64 values, counts as K int64 values, passes) of the definition."""
    pixels = np.concatenate([_flat(f) for f in frames])
    return _passes(lambda pal: assign(pixels, pal), palette, iterations)


def refine_weighted(frames, weights, palette, iterations):
    """refine() of the sequence that holds frames[i] weights[i] times (in any order), at the cost of the distinct frames: cnt, sums and
    sse of an assignment pass are sums over the pixels, so a frame that occurs m times adds m times what it adds once."""
    assert len(frames) == len(weights) and all(int(m) >= 0 for m in weights)

    def one_pass(pal):
        cnt, sums, sse = np.zeros(pal.size, np.int64), np.zeros((pal.size, 3), np.int64), 0
        for f, m in zip(frames, weights):
            c, s, e = assign(_flat(f), pal)
            cnt += int(m) * c
            sums += int(m) * s
            sse += int(m) * int(e)
        return cnt, sums, sse

    return _passes(one_pass, palette, iterations)


def _passes(one_pass, palette, iterations):
    """The passes, the update between them and the early stop over one_pass(palette) -> (cnt, sums, sse)."""
    pal = (np.asarray(palette).reshape(-1).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    sse = np.zeros(iterations + 1, np.int64)
    passes = 0
    for j in range(iterations + 1):
        cnt, sums, sse[j] = one_pass(pal)
        passes = j + 1
        if j == iterations:
            break
        nxt = update(pal, cnt, sums)
        if (nxt == pal).all():
            sse[j + 1:] = sse[j]
            break
        pal = nxt
    return pal, sse, cnt, passes
