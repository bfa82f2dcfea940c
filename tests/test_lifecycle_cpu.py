"""The op table and the schedules of tests/test_gpu_handle_lifecycle.py, without a GPU (tests/lifecycle_ops.py): every export that takes a
handle is driven by an op or is a getter or setter listed here by name, the schedules cover what they claim, and the LARGE references of the encoders are
files a decoder accepts."""
import os
import re
import zlib

import numpy as np

import lifecycle_ops as O
import stream_gate as G
from conftest import ROOT

# exports that take a handle and change nothing a later call reads but what they say: the lifetime calls, the error text, the
# diagnostics, and the setters that parts B and C of the GPU test call directly
GETTERS_AND_SETTERS = {
    "nq_create", "nq_destroy", "nq_last_error", "nq_get_params", "nq_set_params", "nq_set_stream", "nq_set_tile", "nq_set_option", "nq_set_band",
    "nq_get_stage_ms", "nq_get_merge_stats", "nq_get_team_stats", "nq_get_merge_variant", "nq_get_batch_phase_ms", "nq_get_dither_path",
    "nq_get_list_counts", "nq_selftest_ciede", "nq_selftest_fast",
}
# ops with no twin of the other form, each for its reason
DEVICE_ONLY = {
    "hold_device": "the host form always fetches the counts: hold_counts_host",
    "ordered_device": "the host form always fetches the statistics: ordered_stats_host",
    "batch_last_device": "the host batch runs with the handle first: batch_first_host",
    "pnnquan_frames_dither_device": "nq_pnnquan_frames has no host export",
    "split_first_device": "the split pipeline has device exports only",
    "split_last_device": "the split pipeline has device exports only",
}


def _handle_taking_exports():
    src = open(os.path.join(ROOT, "include", "nquant_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(m.group(1) for m in re.finditer(r"\b(nq_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", src, re.S) if "nq_handle" in m.group(2)))


def test_every_export_that_takes_a_handle_is_driven_or_listed(nq):
    exports = _handle_taking_exports()
    assert len(exports) >= 80 and set(exports) <= set(nq.abi_symbols())
    used = {s for op in O.OPS.values() for s in op.symbols}
    assert used <= set(exports), sorted(used - set(exports))
    assert not (used & GETTERS_AND_SETTERS)
    assert GETTERS_AND_SETTERS <= set(exports)
    missing = [e for e in exports if e not in used and e not in GETTERS_AND_SETTERS]
    assert not missing, "no op of tests/lifecycle_ops.py calls %s" % missing
    print("%d ops drive %d of %d handle-taking exports (%d getters and setters)" % (len(O.OPS), len(used), len(exports), len(GETTERS_AND_SETTERS)))
    # every _device op has its host form in the table, but for the short list above
    assert set(DEVICE_ONLY) <= set(O.OPS)
    for name in O.NAMES:
        if name.endswith("_device") and name not in DEVICE_ONLY:
            assert name[:-len("_device")] + "_host" in O.OPS, name


def test_centre_schedule_covers_every_ordered_pair_with_the_centre():
    for centre in (O.NAMES[0], "convert_tiled_dither_host", O.NAMES[-1]):
        steps = O.centre_schedule(centre)
        pairs = set(zip([s[0] for s in steps], [s[0] for s in steps[1:]]))
        for other in O.NAMES:
            if other != centre:
                assert (centre, other) in pairs and (other, centre) in pairs, (centre, other)
        # both orders of size: LARGE before small and small before LARGE, with the centre on either side
        sizes = set((a[0] == centre, a[1] == "LARGE", b[1] == "LARGE") for a, b in zip(steps, steps[1:]))
        assert {(True, True, False), (True, False, True), (False, True, True), (False, False, False)} <= sizes
        assert all(s[0] in O.OPS and s[1] in O.VARIANTS for s in steps)
    # every unordered pair of ops is adjacent in both orders somewhere in part A
    assert len(O.NAMES) == len(set(O.NAMES)) >= 60


def test_walks_are_reproducible_and_mixed():
    for seed in (11, 12, 13, 14):
        a, b = O.walk(seed), O.walk(seed)
        assert a == b and len(a) == 150
        assert a[:40] == O.walk(seed, 40)                          # (a prefix is the same walk: lifecycle_replay.py cuts it down)
        kinds = {s[0] for s in a}
        assert kinds == {"op", "option", "tile", "stream", "params"}, (seed, kinds)
        assert {s[2] for s in a if s[0] == "op"} == set(O.VARIANTS)
    assert O.walk(11) != O.walk(12)


def test_large_is_what_it_is_said_to_be():
    w, h, shift, K = G.LARGE
    assert (w * h + 16383) // 16384 == 3 and ((w + 1) * h + 32767) // 32768 == 2        # LZW chains, deflate chains per frame
    assert (w + 63) // 64 == 3 and (h + 63) // 64 == 3 and w % 64 and h % 64 and w % 2 and h % 2
    assert K == 256 and shift == 1 and G.LARGE_FRAMES == 5
    # the default of the shapes parameter is what it was
    assert sorted(c.name for c in G._frame_cases()) == sorted(n for n in G.cases() if "-" in n)


def test_large_encoder_references_decode():
    import png_ref
    cases = O.frame_cases()
    maps = cases[("png", "LARGE")].true["index"]
    pal = cases[("png", "LARGE")].args["palette"]
    files = G.want(cases[("png", "LARGE")])["files"]
    assert len(files) == 5
    for f, m in zip(files, maps):
        chunks = dict(png_ref.parse(f))                              # (every CRC verified)
        raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(m.shape[0], m.shape[1] + 1)
        assert (raw[:, 0] == 0).all() and (raw[:, 1:] == m).all()
        assert (np.asarray(png_ref.decode(f)[0]) == m).all()
    try:
        import io
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        rgb = np.stack([(pal.view(np.uint32) >> s) & 255 for s in (16, 8, 0)], -1).astype(np.uint8)
        for f, m in zip(files, maps):
            im = Image.open(io.BytesIO(f))
            assert im.size == (m.shape[1], m.shape[0])
            assert (np.asarray(im.convert("RGB")) == rgb[m]).all()
        for family in ("gif", "gif_delta", "apng"):
            im = Image.open(io.BytesIO(G.want(cases[(family, "LARGE")])["file"]))
            assert im.size == (181, 187) and getattr(im, "n_frames", 1) == 5, family
            im.seek(4)
            assert (np.asarray(im.convert("RGB")) == rgb[cases[(family, "LARGE")].true["index"][4]]).all(), family


def test_large_lossy_and_local_table_references_decode():
    """The LARGE references of the lossy and local-table GIF ops are files a decoder accepts: 5 frames of 181 x 187, every composed pixel
    within the lossy bound of the colour its index map asks for (gif_local_ref.compose; Pillow too if present)."""
    import gif_local_ref
    import gif_lossy_ref
    maps, K, pal, locals_, delays = O._gif_inputs("LARGE")
    files = {"lossy": (gif_lossy_ref.encode(maps, pal, delays_cs=delays, loop=0, lossy=O.LOSSY)[0], [pal] * 5, O.LOSSY, False),
             "delta_lossy": (gif_lossy_ref.encode_delta(maps, pal, delays_cs=delays, loop=0, lossy=O.LOSSY)[0], [pal] * 5, O.LOSSY, True),
             "local": (gif_local_ref.encode(maps, locals_, delays_cs=delays, loop=0, lossy=O.LOSSY)[0], locals_, O.LOSSY, False),
             "local_delta": (gif_local_ref.encode_delta(maps, locals_, delays_cs=delays, loop=0, lossy=0)[0], locals_, 0, True)}
    for name, (data, pals, lossy, delta) in files.items():
        canvases = gif_local_ref.compose(data)
        assert len(canvases) == 5 and canvases[0].shape == (187, 181, 3), name
        for i, (canvas, m, p) in enumerate(zip(canvases, maps, pals)):
            p = np.asarray(p).astype(np.int64) & 0xFFFFFF
            want = np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], -1)[m]
            # (a delta frame may keep a pixel of the frame before, itself within the bound of ITS colour: the bound holds where the frame paints)
            if not delta or i == 0:
                assert int(np.abs(canvas.astype(np.int64) - want).max()) <= lossy, (name, i)
        try:
            import io
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(data))
        assert im.size == (181, 187) and im.n_frames == 5, name

