"""The gate protocol of tests/test_gpu_streams.py, and the inputs, poisons and references of its cases (tests/test_streams_cpu.py checks
those without a GPU).  A helper, not a test module and not a conftest.

What it makes visible: work of a `_device` entry point that is not ordered on the handle's stream -- a kernel, fill or copy on
another stream, a pointer table or palette read after the call has returned.  Every GPU test we had uploaded its inputs synchronously
and ran on the NULL stream between two device-wide waits, where any order gives the right answer.

The protocol, for one stream S the handle is set to:
  1. the true inputs and a POISON of the same shape, type and class are on the device, and the device is idle;
       ARGB frames      the true frame with its r, g, b bits inverted, alpha kept
       YUV planes       every byte inverted
       index maps       K - 1 - index
     poison is a valid input of the call: a wrong order gives a wrong answer, never an access out of range;
  2. the input buffers hold the poison, the outputs (and the guard words around them) a sentinel;
  3. on S: the gate (torch.cuda._sleep, a bounded spin), then one device-to-device copy per input that makes it true;
  4. the library call(s), with no host wait;
  5. on S, with no host wait: a copy of every output buffer, guards included, into a second buffer (the snapshot);
  6. for a call the header documents as asynchronous, on a handle warmed by one call of the same shape: S must still be busy --
     the call has returned while the gate ran.  This is also the guard against a gate that is too short: it fails, it does not pass
     vacuously;
  7. wait for S; the snapshot equals the reference of the TRUE inputs over the whole buffer, and the inputs equal the true inputs.
A call that read an input before S reached it saw the poison; a call that wrote an output after S's snapshot is missing from it.

Gate length.  Measured on an MI355X, once: issuing steps 3-5 of the slowest-issuing case, the six-image batch, with no gate takes
272 to 284 ms of host time (fills 0.06 ms, the call 272 to 284 ms -- it waits for its own results --, snapshots 0.2 ms).  The rule is
10 x that, at least 20 ms and at most 250 ms per gate, so the cap decides: GATE_MS = 250.  The spin is calibrated once per module
(a fixed cycle count timed between two events on S; 405 million cycles gave 169 ms).

Known limit: the machines run with four hardware queues, and a misplaced kernel that happens to share the gate's queue is serialised
behind it -- the case passes.  The protocol can miss a bug; it cannot fail falsely.

Buffers are laid out as _Stream / _Planes of tests/test_gpu_yuv.py lay them out (guard elements before, between and behind the
arrays); _Maps is _Stream for uint16 index maps."""
import numpy as np

from nquant.android_amd import synth

GATE_MS = 250.0
SENT_ARGB = -9
SENT_INDEX = 0xA5A5
TILE = (16, 16)
WIDE, NARROW = (48, 40, 0), (45, 37, 1)         # (width, height, shift): the 16-byte paths; the one-element paths (odd sides, one element off)
SHAPES = (WIDE, NARROW)
# (width, height, shift, K of the encoders' maps), 5 frames: the smallest shape whose encoder scratch has more than one entry per frame --
# 33 847 pixels are three LZW chains of 16 384, 182 * 187 = 34 034 raw bytes two deflate chains of 32 768 --, with 3 x 3 partly filled
# 64 x 64 orient tiles and an odd-sided 4:2:0 frame (tests/lifecycle_ops.py)
LARGE = (181, 187, 1, 256)
LARGE_FRAMES = 5


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and their poisons (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------------
def invert_rgb(a):
    return (np.ascontiguousarray(a).view(np.uint32) ^ np.uint32(0x00FFFFFF)).view(np.int32)


def invert_planes(frame):
    return tuple(np.ascontiguousarray(~p) for p in frame)


def flip_index(m, K):
    return (K - 1 - np.asarray(m).astype(np.int64)).astype(np.uint16)


def argb_frames(w, h, n, seed):
    """n frames of distinct random words, alpha 255 for most pixels and 1..254 for the rest (never 0: every pixel counts everywhere)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        rgb = rng.integers(0, 1 << 24, (h, w), dtype=np.int64)
        a = np.where(rng.random((h, w)) < 0.7, 255, rng.integers(1, 255, (h, w)))
        out.append(((a << 24) | rgb).astype(np.uint32).view(np.int32))
    return out


def yuv_frames(w, h, n, seed):
    import yuv_ref
    return [yuv_ref.random_planes(w, h, seed + i) for i in range(n)]


def index_maps(w, h, n, K, seed, still=False):
    """n random index maps; still=True: frames 1.. equal frame 0 outside a box of their own (what the delta encoders crop to)."""
    rng = np.random.default_rng(seed)
    maps = [rng.integers(0, K, (h, w)).astype(np.uint16) for _ in range(n)]
    if still:
        for i in range(1, n):
            m = maps[0].copy()
            y, x = 3 + 2 * i, 5 + 3 * i
            m[y:y + h // 2, x:x + w // 2] = maps[i][y:y + h // 2, x:x + w // 2]
            maps[i] = m
    return maps


def still_frames(w, h, n, seed):
    """Opaque footage for the temporal hold: one random picture with -2..+2 of noise per channel and frame (held at threshold 4), and
    an 8 x 8 block of new random colours at a place of its own in every frame (released)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(2, 254, (3, h, w))
    out = []
    for i in range(n):
        c = base + rng.integers(-2, 3, (3, h, w))
        y, x = (2 + 3 * i) % (h - 8), (4 + 5 * i) % (w - 8)
        c[:, y:y + 8, x:x + 8] = rng.integers(0, 256, (3, 8, 8))
        out.append(((255 << 24) | (c[0] << 16) | (c[1] << 8) | c[2]).astype(np.uint32).view(np.int32))
    return out


def palette(K, seed):
    rng = np.random.default_rng(seed)
    return (np.uint32(0xFF000000) | rng.integers(0, 1 << 24, K, dtype=np.int64).astype(np.uint32)).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the CPU oracle (quantizer cases)
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile(img):
    h, w = img.shape
    return (min(TILE[0], w), min(TILE[1], h))


def oracle_scalars(kind, img, K):
    """What the pre-scan leaves for the later stages: (hasSemiTransparency, transparentPixelIndex, transparentColor)."""
    import oracle_lib
    oq = oracle_lib.OracleQuantizer(kind, img)
    oq.prescan(K)
    p = oq.params
    oq.close()
    return (p.hasSemiTransparency, p.transparentPixelIndex, p.transparentColor)


def oracle_dither(kind, img, K, seed, pal, shared=None):
    """The oracle's tiled dither of img with `pal` (and, when given, another image's params): (index map uint16, ARGB int32)."""
    import oracle_lib
    oq = oracle_lib.OracleQuantizer(kind, img, seed=seed)
    oq.prescan(K)
    if shared is not None:
        oq.set_params(shared)
    oq.set_seed(seed)
    argb, idx = oq.dither(np.asarray(pal).view(np.int32), True, tile=_tile(img))
    oq.close()
    return idx.astype(np.uint16), argb


def oracle_convert(kind, img, K, seed):
    """convert(K, true), tiled: (palette, index map, ARGB, params)."""
    import oracle_lib
    oq = oracle_lib.OracleQuantizer(kind, img, seed=seed)
    oq.prescan(K)
    pal = oq.pnnquan(K)
    params = oq.params
    oq.set_seed(seed)
    argb, idx = oq.dither(pal, True, tile=_tile(img))
    oq.close()
    return pal, idx.astype(np.uint16), argb, params


def oracle_sequence(kind, frames, K):
    """(palette, params) of the concatenated sequence."""
    import oracle_lib
    oq = oracle_lib.OracleQuantizer(kind, np.concatenate([f.reshape(-1) for f in frames]).reshape(-1, 1))
    oq.prescan(K)
    pal = oq.pnnquan(K)
    params = oq.params
    oq.close()
    return pal, params


def oracle_frames(kind, frames, K, seeds, refine=0):
    """nq_convert_frames[_refined]: (palette as int32, index maps, ARGB outputs)."""
    import refine_ref
    pal, shared = oracle_sequence(kind, frames, K)
    if refine:
        pal = refine_ref.refine(frames, pal, refine)[0].view(np.int32)
    both = [oracle_dither(kind, f, K, s, pal, shared) for f, s in zip(frames, seeds)]
    return pal, [b[0] for b in both], [b[1] for b in both]


def quant_image(w, h, seed):
    """Opaque, with far more than 256 colours; so is its poison, and the pre-scan's scalars agree (test_streams_cpu.py)."""
    return synth.gradient_noise(w, h, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of part A: name -> Case.  inputs(poisoned) gives {group: arrays}; the group's name says what it is ("argb...", "yuv...",
# "index...": the classes of poison above); "io_..." groups are updated in place.  reference(inputs) gives {name: result}: "out_argb..."
# / "out_index..." are lists of per-pixel device outputs, "io_..." the in-place groups afterwards, everything else comes back on the host.
# ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, true, reference, asynchronous, K=None, shift=0, quant=None, **args):
        self.name, self.true, self.reference, self.asynchronous, self.K, self.shift, self.quant, self.args = \
            name, true, reference, asynchronous, K, shift, quant, args

    def inputs(self, poisoned):
        if not poisoned:
            return self.true
        out = {}
        for g, arrays in self.true.items():
            if "yuv" in g:
                out[g] = [invert_planes(f) for f in arrays]
            elif "index" in g:
                out[g] = [flip_index(m, self.K) for m in arrays]
            else:
                out[g] = [invert_rgb(a) for a in arrays]
        return out


_REF = {}


def want(case):
    """The reference of the case's true inputs, computed once."""
    if case.name not in _REF:
        _REF[case.name] = case.reference(case.true)
    return _REF[case.name]


def _frame_cases(shapes=SHAPES, n=3):
    """The frame and encoder cases at every shape of `shapes`: (width, height, shift) or (width, height, shift, K of the encoders' maps;
    default 256 at shift 0, else 16), n frames each."""
    import apng_ref
    import gif_delta_ref
    import gif_ref
    import hold_ref
    import ordered_ref
    import orient_ref
    import png_ref
    import refine_ref
    import resample_ref
    import shots_ref
    import yuv_ref
    cases = []
    for shape in shapes:
        w, h, shift = shape[:3]
        tag = "%dx%d" % (w, h)
        frames = argb_frames(w, h, n, 7000 + w)
        planes = yuv_frames(w, h, n, 7100 + w)
        footage = still_frames(w, h, n, 7200 + w)
        maps = index_maps(w, h, n, 256, 7300 + w)
        outs = argb_frames(w, h, n, 7400 + w)
        small = (13, 11) if w < 64 else (w // 3 + 1, h // 4 + 1)                           # (45 x 37: 13 x 11 of the crop 40 x 33 at (3, 2))
        size, crop = ((20, 16), None) if shift == 0 else (small, (3, 2, w - 5, h - 4))
        osize, ocrop = ((16, 20), None) if shift == 0 else (small[::-1], (2, 3, h - 4, w - 5))     # of the turned frame (codes 5..8)
        pal256, pal16 = palette(256, 7500 + w), palette(16, 7600 + w)
        turn = 6 if shift == 0 else 5

        def hold(i, counts):
            idx, held, out = hold_ref.hold(i["argb"], i["io_index"], 4, i["io_argb"])
            r = {"io_index": idx, "io_argb": out}
            if counts:
                r["held"] = np.asarray(held, np.int64)
            return r
        for counts in (True, False):
            cases.append(Case("hold%s-%s" % ("_counts" if counts else "", tag), {"argb": footage, "io_index": maps, "io_argb": outs},
                              lambda i, c=counts: hold(i, c), not counts, K=256, shift=shift, counts=counts, w=w, h=h))
        cases.append(Case("resample-" + tag, {"argb": frames},
                          lambda i, s=size, c=crop: {"out_argb": resample_ref.resample(i["argb"], s, c, resample_ref.LINEAR)},
                          True, shift=shift, size=size, crop=crop, w=w, h=h))
        cases.append(Case("yuv-" + tag, {"yuv": planes}, lambda i: {"out_argb": yuv_ref.convert(i["yuv"], yuv_ref.BT709)},
                          True, shift=shift, w=w, h=h))
        cases.append(Case("resample_yuv-" + tag, {"yuv": planes},
                          lambda i, s=size, c=crop: {"out_argb": yuv_ref.resample(i["yuv"], s, c, yuv_ref.BT709, yuv_ref.LINEAR)},
                          True, shift=shift, size=size, crop=crop, w=w, h=h))
        for code in (turn, 3):
            cases.append(Case("orient%d-%s" % (code, tag), {"argb": frames}, lambda i, c=code: {"out_argb": orient_ref.orient_all(i["argb"], c)},
                              True, shift=shift, code=code, w=w, h=h))
        cases.append(Case("yuv_oriented-" + tag, {"yuv": planes},
                          lambda i, c=turn: {"out_argb": orient_ref.yuv_oriented(i["yuv"], c, yuv_ref.BT709)}, True, shift=shift, code=turn, w=w, h=h))
        cases.append(Case("resample_oriented-" + tag, {"argb": frames},
                          lambda i, c=turn, s=osize, r=ocrop: {"out_argb": orient_ref.resample_oriented(i["argb"], c, s, r)},
                          True, shift=shift, code=turn, size=osize, crop=ocrop, w=w, h=h))
        cases.append(Case("resample_yuv_oriented-" + tag, {"yuv": planes},
                          lambda i, c=turn, s=osize, r=ocrop: {"out_argb": orient_ref.resample_yuv_oriented(i["yuv"], c, s, r, yuv_ref.BT709)},
                          True, shift=shift, code=turn, size=osize, crop=ocrop, w=w, h=h))

        def ordered(i, pal, stats):
            idx, out, st = ordered_ref.dither(i["argb"], pal, 24)
            r = {"out_index": idx, "out_argb": [o.view(np.int32) for o in out]}
            if stats:
                r["stats"] = st
            return r
        for stats in (True, False):
            cases.append(Case("ordered%s-%s" % ("_stats" if stats else "", tag), {"argb": frames},
                              lambda i, p=pal256, s=stats: ordered(i, p, s), not stats, shift=shift, palette=pal256, limit=24, stats=stats, w=w, h=h))

        def refine(i, pal):
            p, sse, counts, passes = refine_ref.refine(i["argb"], pal, 3)
            return {"palette": p, "sse": sse, "counts": counts, "passes": passes}
        cases.append(Case("refine-" + tag, {"argb": frames}, lambda i, p=pal16: refine(i, p), False, shift=shift, palette=pal16, w=w, h=h))
        cases.append(Case("signatures-" + tag, {"argb": frames}, lambda i: {"sig": shots_ref.signatures(i["argb"])}, False, shift=shift, w=w, h=h))

        def detect(i):
            starts, scores = shots_ref.detect(i["argb"], 0, 1)
            return {"starts": list(starts), "scores": np.asarray(scores, np.int32)}
        cases.append(Case("detect_shots-" + tag, {"argb": frames}, detect, False, shift=shift, w=w, h=h))

        K = shape[3] if len(shape) > 3 else 256 if shift == 0 else 16
        epal = pal256 if K == 256 else pal16
        emaps = index_maps(w, h, n, K, 7700 + w, still=True)
        delays = ([3, 0, 65535] * n)[:n]
        cases.append(Case("gif-" + tag, {"index": emaps}, lambda i, p=epal: {"file": gif_ref.encode(i["index"], p, delays_cs=delays, loop=0)},
                          False, K=K, shift=shift, palette=epal, delays=delays, w=w, h=h))
        cases.append(Case("gif_delta-" + tag, {"index": emaps},
                          lambda i, p=epal: {"file": gif_delta_ref.encode(i["index"], p, delays_cs=delays, loop=0),
                                             "rects": gif_delta_ref.rectangles(i["index"])},
                          False, K=K, shift=shift, palette=epal, delays=delays, w=w, h=h))
        cases.append(Case("png-" + tag, {"index": emaps}, lambda i, p=epal: {"files": [png_ref.encode(m, p) for m in i["index"]]},
                          False, K=K, shift=shift, palette=epal, w=w, h=h))
        cases.append(Case("apng-" + tag, {"index": emaps}, lambda i, p=epal: {"file": apng_ref.encode(i["index"], p, delays_cs=delays, loop=0)},
                          False, K=K, shift=shift, palette=epal, delays=delays, w=w, h=h))
    return cases


def _quant_cases():
    cases = []

    def convert(i, kind, K, seed):
        pal, idx, argb, _ = oracle_convert(kind, i["argb"][0], K, seed)
        return {"palette": pal, "out_index": [idx], "out_argb": [argb]}
    cases.append(Case("convert_device", {"argb": [quant_image(96, 80, 7801)]}, lambda i: convert(i, 1, 256, 51), False,
                      quant=(1, 256), kind=1, seed=51, w=96, h=80))
    cases.append(Case("pnnquan_dither_device", {"argb": [quant_image(64, 64, 7802)]}, lambda i: convert(i, 0, 16, 52), False,
                      quant=(0, 16), kind=0, seed=52, w=64, h=64))

    def frames(i, kind, K, seeds, refine):
        pal, idx, argb = oracle_frames(kind, i["argb"], K, seeds, refine)
        return {"palette": pal, "out_index": idx, "out_argb": argb}
    seeds = [61, 62, 63]
    cases.append(Case("convert_frames_device", {"argb": [quant_image(72, 64, 7810 + k) for k in range(3)]}, lambda i: frames(i, 1, 256, seeds, 0),
                      False, quant=(1, 256), kind=1, seeds=seeds, refine=None, w=72, h=64))
    cases.append(Case("convert_frames_refined_device", {"argb": [quant_image(64, 64, 7820 + k) for k in range(3)]},
                      lambda i: frames(i, 0, 16, seeds, 2), False, quant=(0, 16), kind=0, seeds=seeds, refine=2, w=64, h=64))

    def ordered(i, kind, K, limit):
        import ordered_ref
        pal, _ = oracle_sequence(kind, i["argb"], K)
        idx, out, _ = ordered_ref.dither(i["argb"], pal, limit)
        return {"palette": pal, "out_index": idx, "out_argb": [o.view(np.int32) for o in out]}
    cases.append(Case("convert_frames_ordered_device", {"argb": [quant_image(80, 64, 7830 + k) for k in range(3)]},
                      lambda i: ordered(i, 1, 256, 16), False, quant=(1, 256), kind=1, limit=16, w=80, h=64))
    return cases


_CASES = {}


def cases():
    """Every case of part A, by name (built once)."""
    if not _CASES:
        for c in _frame_cases() + _quant_cases():
            assert c.name not in _CASES
            _CASES[c.name] = c
    return _CASES


# part B: six images of mixed kinds, every one with a merge job
BATCH_K = 256
BATCH = [(1, 96, 80), (0, 64, 64), (1, 80, 72), (0, 70, 66), (1, 96, 64), (0, 72, 80)]     # (kind, width, height)
BATCH_SEEDS = [71, 72, 73, 74, 75, 76]


def batch_images():
    return [quant_image(w, h, 7900 + i) for i, (_, w, h) in enumerate(BATCH)]


def batch_want():
    """[(palette, index map, ARGB)] of the oracle per image, computed once."""
    if "batch" not in _REF:
        _REF["batch"] = [oracle_convert(kind, img, BATCH_K, seed)[:3] for (kind, _, _), img, seed in zip(BATCH, batch_images(), BATCH_SEEDS)]
    return _REF["batch"]


# part C: two asynchronous calls back to back on one handle -- n = 2, then n = 9 on other buffers (and, ordered, with another palette)
PAIR_KINDS = ("hold", "resample", "yuv", "orient", "ordered")
PAIR_W, PAIR_H = 48, 40


def pair_case(kind, n):
    """(true inputs, reference, arguments) of call `kind` over n frames of 48 x 40; computed once."""
    key = ("pair", kind, n)
    if key not in _REF:
        import hold_ref
        import ordered_ref
        import orient_ref
        import resample_ref
        import yuv_ref
        w, h, seed = PAIR_W, PAIR_H, 8000 + 10 * n
        args = {}
        if kind == "hold":
            ins = {"argb": still_frames(w, h, n, seed), "io_index": index_maps(w, h, n, 256, seed + 1), "io_argb": argb_frames(w, h, n, seed + 2)}
            idx, _, out = hold_ref.hold(ins["argb"], ins["io_index"], 4, ins["io_argb"])
            ref = {"io_index": idx, "io_argb": out}
        elif kind == "resample":
            ins = {"argb": argb_frames(w, h, n, seed + 3)}
            ref = {"out_argb": resample_ref.resample(ins["argb"], (20, 16), None, resample_ref.LINEAR)}
        elif kind == "yuv":
            ins = {"yuv": yuv_frames(w, h, n, seed + 4)}
            ref = {"out_argb": yuv_ref.convert(ins["yuv"], yuv_ref.BT709)}
        elif kind == "orient":
            ins = {"argb": argb_frames(w, h, n, seed + 5)}
            ref = {"out_argb": orient_ref.orient_all(ins["argb"], 6)}
        else:
            ins = {"argb": argb_frames(w, h, n, seed + 6)}
            args["palette"] = palette(256, seed + 7)
            idx, out, _ = ordered_ref.dither(ins["argb"], args["palette"], 24)
            ref = {"out_index": idx, "out_argb": [o.view(np.int32) for o in out]}
        _REF[key] = (ins, ref, args)
    return _REF[key]


def poisoned(inputs, K=256):
    """The poison of a dict of input groups (by the groups' names)."""
    return Case("", inputs, None, False, K=K).inputs(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the device side (needs torch and a GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
_CLASSES = []


def buffer_classes():
    """(_Stream, _Planes, _Maps)."""
    if not _CLASSES:
        import torch
        from test_gpu_yuv import GUARD, _Planes, _Stream

        class _Maps(_Stream):
            """_Stream for uint16 arrays (index maps)."""

            def __init__(self, arrays, shift, sentinel):
                px = arrays[0].size
                pitch = (px + 7) // 8 * 8 + GUARD
                self.offs = [GUARD + i * pitch + shift for i in range(len(arrays))]
                self.px = px
                self.host = np.full(GUARD + len(arrays) * pitch + 8, sentinel, np.uint16)
                self.fill(self.host, arrays)
                self.dev = torch.from_numpy(self.host.view(np.int16).copy()).cuda()
                assert self.dev.data_ptr() % 16 == 0
                self.ptrs = [self.dev.data_ptr() + 2 * o for o in self.offs]

            def read(self):
                return self.dev.cpu().numpy().view(np.uint16)
        _CLASSES.extend([_Stream, _Planes, _Maps])
    return _CLASSES


def _tensor(host):
    import torch
    return torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host)


def make_buffer(group, arrays, shift=0):
    """The device buffer of a group of arrays (by the group's name), guards included."""
    _Stream, _Planes, _Maps = buffer_classes()
    if "yuv" in group:
        return _Planes(arrays, "nv12", shift)
    if "index" in group:
        return _Maps(arrays, shift, SENT_INDEX)
    return _Stream(arrays, shift, SENT_ARGB)


def make_output(group, like, shift=0):
    """A sentinel-filled output buffer for arrays shaped like `like`."""
    _Stream, _Planes, _Maps = buffer_classes()
    if "index" in group:
        return _Maps([np.full(a.shape, SENT_INDEX, np.uint16) for a in like], shift, SENT_INDEX)
    return _Stream([np.full(a.shape, SENT_ARGB, np.int32) for a in like], shift, SENT_ARGB)


def calibrate(stream, ms=GATE_MS):
    """(cycles of torch.cuda._sleep that last `ms` on `stream`, the length in ms of one such gate as measured afterwards)."""
    import torch
    probe = 2000000
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)
        ev[0].record()
        torch.cuda._sleep(probe)
        ev[1].record()
    ev[1].synchronize()
    cycles = int(probe * ms / max(ev[0].elapsed_time(ev[1]), 1e-3))
    with torch.cuda.stream(stream):
        ev[2].record()
        torch.cuda._sleep(cycles)
        ev[3].record()
    ev[3].synchronize()
    return cycles, ev[2].elapsed_time(ev[3])


class Gate:
    """Steps 2 to 7 for the buffers registered with it.  stream: a torch stream (torch.cuda.default_stream() for the NULL stream)."""

    def __init__(self, stream, cycles):
        self.stream, self.cycles = stream, cycles
        self.ins, self.outs, self.decoys = [], [], []

    def input(self, group, true_arrays, poison_arrays, shift=0, in_place=False):
        """The working buffer of an input group: it holds the poison until S makes it true."""
        import torch
        work = make_buffer(group, poison_arrays, shift)
        true = make_buffer(group, true_arrays, shift)
        assert work.host.shape == true.host.shape
        work.true_host, work.true_dev = true.host, true.dev
        self.ins.append((work, in_place))
        if in_place:
            work.snap = torch.empty_like(work.dev)
            self.outs.append(work)
        return work

    def output(self, group, like, shift=0):
        import torch
        buf = make_output(group, like, shift)
        buf.snap = torch.empty_like(buf.dev)
        self.outs.append(buf)
        return buf

    def decoy(self, group, like):
        """A valid buffer nothing may write: what an overwritten pointer array points at."""
        buf = make_output(group, like)
        self.decoys.append(buf)
        return buf

    def prepare(self):
        """Step 2; the device is idle afterwards."""
        import torch
        for work, _ in self.ins:
            work.dev.copy_(_tensor(work.host))
        for buf in self.outs:
            if not hasattr(buf, "true_dev"):
                buf.dev.copy_(_tensor(buf.host))
        torch.cuda.synchronize()

    def start(self, gate=True):
        """Step 3.  gate=False: the same without the spin (warming calls, the issue-time measurement)."""
        import torch
        with torch.cuda.stream(self.stream):
            if gate:
                torch.cuda._sleep(self.cycles)
            for work, _ in self.ins:
                work.dev.copy_(work.true_dev, non_blocking=True)

    def arm(self, gate=True):
        self.prepare()
        self.start(gate)

    def finish(self, asynchronous, what="", wait=True):
        """Steps 5, 6 and (wait=True) the wait of step 7.  Returns whether S was still busy when the last snapshot had been enqueued."""
        import torch
        with torch.cuda.stream(self.stream):
            for buf in self.outs:
                buf.snap.copy_(buf.dev, non_blocking=True)
            busy = not self.stream.query()
        if asynchronous:
            assert busy, "%s: the stream was idle when the calls had returned -- they waited for the gate, or the gate is too short" % what
        if wait:
            self.stream.synchronize()
        return busy

    def snapshot(self, buf):
        return buf.snap.cpu().numpy().view(buf.host.dtype)

    def check(self, buf, arrays, what=""):
        """The snapshot of an output (or in-place) buffer equals `arrays` inside and the sentinel (in place: the guards) around them."""
        got = self.snapshot(buf)
        base = buf.true_host if hasattr(buf, "true_host") else buf.host
        expect = base.copy()
        buf.fill(expect, [np.ascontiguousarray(a).view(base.dtype) for a in arrays])
        bad = int((got != expect).sum())
        assert bad == 0, "%s: %d of %d elements of the snapshot differ from the reference (guards included)" % (what, bad, got.size)

    def check_inputs(self, what=""):
        """Step 7, second half: the inputs equal the true inputs, the decoys their sentinel."""
        for work, in_place in self.ins:
            if not in_place:
                assert (work.read() == work.true_host).all(), "%s: an input buffer does not hold the true input" % what
        for d in self.decoys:
            assert (d.read() == d.host).all(), "%s: a decoy buffer was written" % what
