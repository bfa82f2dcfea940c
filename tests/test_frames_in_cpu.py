"""The converters' shared opening (nquant.android_amd/_frames_in.py), without a GPU: what it refuses is refused from the arguments alone,
with the same exception for every converter, and before the converter's own checks."""
import re

import numpy as np
import pytest


def _trap_library(monkeypatch, nq):
    """From here on any use of the loaded library fails the test: the errors below are raised from the arguments alone."""
    class Trap:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    nq.load_library()
    monkeypatch.setattr(nq.host, "_LIB", Trap())


# (converter, its positional arguments after `frames`, whether it takes retime / delays_cs / seeds)
CONVERTERS = [("convert_frames_to_gif", (16, True), True), ("convert_shots_to_gif", ([0], 16, True), True), ("convert_clip_to_gif", (16, True), True),
              ("convert_frames_to_apng", (16, True), True), ("convert_frames_to_webp", (16, True), True),
              ("convert_frames_refined", (16, True, 2), False), ("convert_frames_ordered", (16, 32), False)]


@pytest.mark.parametrize("name,args,timed", CONVERTERS, ids=[c[0] for c in CONVERTERS])
def test_converters_refuse_their_frame_keywords_before_any_library_call(nq, monkeypatch, name, args, timed):
    """What the converters' shared opening refuses, per converter: the exception's type and text, and which of two errors wins."""
    _trap_library(monkeypatch, nq)
    fn = getattr(nq, name)
    frames = [np.zeros((4, 4), np.int32)] * 3
    t = [0, 10000, 20000, 30000]
    rt = dict(timestamps_us=t, fps=15)
    shots = name == "convert_shots_to_gif"
    no_retime = (TypeError, "unexpected keyword argument 'retime'")
    shots_retime = (ValueError, "retime changes the frames that shot_starts name")
    table = [(dict(yuv={}, yuv16={}), (TypeError, "yuv and yuv16 exclude each other")),
             (dict(yuv16=5), (TypeError, "yuv16 is None or a dict with the keys matrix / full_range / transfer / msb")),
             (dict(yuv16=dict(gamma=2)), (TypeError, "yuv16 is None or a dict with the keys")),
             (dict(retime=rt, delays_cs=[4, 4, 4]), (ValueError, "retime supplies delays_cs: pass one of the two")),
             (dict(retime=rt, seeds=[1, 2, 3]), (ValueError, "retime: seeds are given per frame")),
             (dict(retime=dict(fps=15)), (TypeError, "retime is None or a dict with the keys timestamps_us")),
             (dict(retime=15), (TypeError, "retime is None or a dict with the keys timestamps_us")),
             (dict(retime=dict(timestamps_us=t[:-1], fps=15)), (ValueError, "retime: 3 frames need 4 timestamps, got 3")),
             # two errors at once: the opening comes before the converter's own checks
             (dict(retime=rt, delays_cs=[4, 4, 4], nMaxColors=300), (ValueError, "retime supplies delays_cs: pass one of the two")),
             (dict(yuv={}, yuv16={}, nMaxColors=300), (TypeError, "yuv and yuv16 exclude each other")),
             (dict(yuv={}, yuv16={}, orient=9), (TypeError, "yuv and yuv16 exclude each other"))]
    for kw, want in table:
        kw = dict(kw)
        if "retime" in kw:
            if not timed:
                kw.pop("delays_cs", None), kw.pop("seeds", None)
                want = no_retime
            elif shots:
                want = shots_retime
        a = list(args)
        if "nMaxColors" in kw:
            a[1 if shots else 0] = kw.pop("nMaxColors")
        with pytest.raises(want[0], match=re.escape(want[1])):
            fn(1, frames, *a, **kw)
    if not timed:                                            # ... and before the check of refine
        with pytest.raises(TypeError, match="yuv and yuv16 exclude each other"):
            if name == "convert_frames_refined":
                fn(1, frames, 16, True, 65, yuv={}, yuv16={})
            else:
                fn(1, frames, 16, 32, refine=65, yuv={}, yuv16={})
