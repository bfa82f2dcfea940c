"""The JNI shim under a fake JNI runtime.  build() compiles tests/c/jni_fake/fake_jni.c together with the UNMODIFIED
nquant.android_amd/jni/nquant_jni.c (against tests/c/jni_fake/jni.h, our own declarations -- there is no JDK) into one shared object,
linked either to the real libnquant_hip.so (the GPU tests) or to tests/c/jni_fake/stub_abi.c, a scripted stand-in for the ABI (the CPU
tests; no GPU is opened).  Runtime wraps the object in ctypes: constructors for the Java-side objects, one Python method per
Java_com_android_nQuant_PnnQuantizer_* symbol, and after every native call the fake's counters in Runtime.last.  Not a real JVM: what
this holds is that the shim's own logic (marshalling, lengths, release modes, local references, exceptions) is right."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "c", "jni_fake")
SHIM = os.path.join(ROOT, "nquant.android_amd", "jni", "nquant_jni.c")
PREFIX = "Java_com_android_nQuant_PnnQuantizer_"
CFLAGS = ["-std=c11", "-O1", "-g", "-Wall", "-Werror", "-I", FAKE_DIR, "-I", os.path.join(ROOT, "include")]

_vp, _i32, _i64, _u8 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint8
# the native methods of PnnQuantizer.java: name -> (result, parameters after JNIEnv* and jclass); objects are void*
SIGS = {
    "nqCreate": (_i64, [_i32, _i32]),
    "nqDestroy": (None, [_i64]),
    "nqConvert": (_vp, [_i64, _vp, _i32, _i32, _i32, _u8, _i64, _i32, _vp, _vp]),
    "nqHasAlpha": (_u8, [_i64]),
    "nqConvertBatch": (_vp, [_vp, _vp, _vp, _vp, _i32, _u8, _vp, _i32, _vp]),
    "nqConvertFrames": (_vp, [_i64, _vp, _vp, _vp, _i32, _u8, _vp, _i32, _vp]),
    "nqGifMaxBytes": (_i64, [_vp, _vp]),
    "nqEncodeGif": (_i64, [_i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64]),
    "nqEncodeGifDelta": (_i64, [_i64, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i64]),
    "nqConvertFramesToGif": (_i64, [_i64, _vp, _vp, _vp, _i32, _u8, _vp, _i32, _vp, _i32, _u8, _vp, _i64]),
    "nqPngMaxBytes": (_i64, [_i32, _i32]),
    "nqEncodePng": (_i64, [_i64, _vp, _i32, _i32, _vp, _vp, _i64]),
    "nqConvertToPng": (_i64, [_i64, _vp, _i32, _i32, _i32, _u8, _i64, _i32, _vp, _i64]),
    "nqApngMaxBytes": (_i64, [_i32, _i32, _i32]),
    "nqEncodeApng": (_i64, [_i64, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i64]),
    "nqConvertFramesToApng": (_i64, [_i64, _vp, _i32, _i32, _i32, _u8, _vp, _i32, _vp, _i32, _vp, _i64]),
}
COUNTERS = ["violations", "outstanding", "live_locals", "peak_locals", "object_bytes", "aborted_writes", "alloc_calls", "pending",
            "jni_calls", "objects"]

# tests/c/jni_fake/stub_abi.c: function ids, and per function the recorded slots (the signature, then values read through the pointers)
STUB_FUNCTIONS = ["nq_create", "nq_destroy", "nq_get_params", "nq_convert", "nq_convert_batch", "nq_convert_frames", "nq_gif_max_bytes",
                  "nq_encode_gif", "nq_encode_gif_delta", "nq_png_max_bytes", "nq_encode_png", "nq_apng_max_bytes", "nq_encode_apng"]
_FRAMES_READ = ["src0", "srcl", "pal0", "pall", "delay0", "delayl", "index_first", "index_last"]
_ONE_SIZE = ["h", "n", "index", "width", "height", "palette", "K", "delays", "loop", "segment", "out", "cap", "out_size", "rects"] + _FRAMES_READ
STUB_SLOTS = {
    "nq_create": ["kind", "device", "out"],
    "nq_destroy": ["h"],
    "nq_get_params": ["h", "out"],
    "nq_convert": ["h", "argb", "width", "height", "nMaxColors", "dither", "seed", "mode", "out_argb", "out_index", "out_palette", "out_K",
                   "in_first", "in_last"],
    "nq_convert_batch": ["hs", "n", "argb", "widths", "heights", "nMaxColors", "dither", "seeds", "mode", "out_argb", "out_index",
                         "out_palettes", "stride", "out_K", "h0", "hl", "src0", "srcl", "dst0", "dstl", "w0", "wl", "h0_", "hl_", "seed0", "seedl"],
    "nq_convert_frames": ["h", "n", "argb", "widths", "heights", "nMaxColors", "dither", "seeds", "mode", "out_argb", "out_index",
                          "out_palette", "out_K", "src0", "srcl", "dst0", "dstl", "w0", "wl", "h0_", "hl_", "seed0", "seedl"],
    "nq_gif_max_bytes": ["n", "widths", "heights", "K", "segment", "out", "w0", "wl", "h0_", "hl_"],
    "nq_encode_gif": ["h", "n", "index", "widths", "heights", "palette", "K", "delays", "loop", "segment", "out", "cap", "out_size",
                      "w0", "wl", "h0_", "hl_"] + _FRAMES_READ,
    "nq_encode_gif_delta": _ONE_SIZE,
    "nq_encode_apng": _ONE_SIZE,
    "nq_png_max_bytes": ["n", "widths", "heights", "K", "segment", "out", "w0", "h0_"],
    "nq_encode_png": ["h", "n", "index", "widths", "heights", "palettes", "stride", "K", "segment", "out", "cap", "offsets", "w0", "h0_", "K0"]
                     + _FRAMES_READ,
    "nq_apng_max_bytes": ["n", "width", "height", "segment", "out"],
}
PENDING_SLOT = 31


def shim_path():
    """The shim under test; NQ_JNI_SHIM=<path> runs another copy of it (hand-made mutations of the shim, to see the tests fail)."""
    return os.environ.get("NQ_JNI_SHIM") or SHIM


def sources(stub):
    return [os.path.join(FAKE_DIR, "fake_jni.c"), shim_path()] + ([os.path.join(FAKE_DIR, "stub_abi.c")] if stub else [])


def build(out_dir, lib=None):
    """The shared object: fake runtime + shim + (lib: the real library at that path; None: the scripted stub).  Returns its path."""
    so = os.path.join(str(out_dir), "libnquant_jni_under_test.so")
    cmd = ["gcc"] + CFLAGS + ["-fPIC", "-shared", "-o", so] + sources(lib is None)
    if lib is not None:
        # flags and rpaths as tests/test_gpu_boundary.py::test_plain_c_caller_of_the_abi
        cmd += [lib, "-Wl,--allow-shlib-undefined"] + ["-Wl,-rpath," + r for r in (os.path.dirname(lib), "/opt/rocm/lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return so


def exported_natives(so):
    """The Java_com_android_nQuant_PnnQuantizer_* symbols the object exports, without the prefix."""
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1][len(PREFIX):] for line in out.splitlines() if line.split() and line.split()[-1].startswith(PREFIX))


class JavaException(Exception):
    def __init__(self, cls, message):
        super().__init__("%s: %s" % (cls, message))
        self.cls, self.message = cls, message


class Runtime:
    """One loaded object.  Objects made here are owned by the host side until reset()."""
    called = set()          # every native method any Runtime has called (the coverage tests read it)

    def __init__(self, so):
        self.so = so
        L = self.L = C.CDLL(so)
        for name in ("fj_env", "fj_new_int_array", "fj_new_long_array", "fj_new_short_array", "fj_new_object_array", "fj_new_direct_buffer",
                     "fj_new_heap_buffer", "fj_data", "fj_object_element"):
            getattr(L, name).restype = _vp
        L.fj_new_int_array.argtypes = L.fj_new_long_array.argtypes = L.fj_new_short_array.argtypes = [_vp, _i64]
        L.fj_new_object_array.argtypes = L.fj_new_heap_buffer.argtypes = [_i64]
        L.fj_new_direct_buffer.argtypes = [_vp, _i64]
        L.fj_set_object.argtypes = [_vp, _i64, _vp]
        L.fj_object_element.argtypes = [_vp, _i64]
        for name in ("fj_release", "fj_end_call", "fj_data", "fj_length", "fj_tag"):
            getattr(L, name).argtypes = [_vp]
        L.fj_length.restype = _i64
        L.fj_get.restype, L.fj_get.argtypes = _i64, [C.c_int]
        L.fj_fail_alloc.argtypes = [_i64]
        for name in ("fj_violation_log", "fj_exception_class", "fj_exception_message"):
            getattr(L, name).restype = C.c_char_p
        self.stub = hasattr(L, "st_reset")
        if self.stub:
            L.st_script.argtypes = [C.c_int, _i64, _i64, C.c_int]
            L.st_fail_call.argtypes = [C.c_int, C.c_int]
            L.st_set_error.argtypes = [C.c_char_p]
            L.st_call_arg.restype, L.st_call_arg.argtypes = _i64, [C.c_int, C.c_int]
        self._natives = {}
        for name, (res, params) in SIGS.items():
            fn = getattr(L, PREFIX + name)
            fn.restype, fn.argtypes = res, [_vp, _vp] + params
            self._natives[name] = fn
        self.env = L.fj_env()
        self._owned, self._keep = [], []
        self.last = {}

    # ---- the Java side's objects ----
    def _own(self, handle):
        self._owned.append(handle)
        return handle

    def ints(self, values):
        a = np.ascontiguousarray(np.asarray(values).astype(np.int64) & 0xFFFFFFFF, np.uint32).reshape(-1)
        return self._own(self.L.fj_new_int_array(a.ctypes.data, a.size))

    def longs(self, values):
        a = np.ascontiguousarray(values, np.int64).reshape(-1)
        return self._own(self.L.fj_new_long_array(a.ctypes.data, a.size))

    def shorts(self, values):
        a = np.ascontiguousarray(values).astype(np.uint16).reshape(-1)
        return self._own(self.L.fj_new_short_array(a.ctypes.data, a.size))

    def objects(self, handles):
        arr = self._own(self.L.fj_new_object_array(len(handles)))
        for i, h in enumerate(handles):
            self.L.fj_set_object(arr, i, h)
        return arr

    def direct(self, array, capacity=None):
        """A direct buffer over `array`'s memory (kept alive here); capacity in elements, default the array's size."""
        assert array.flags["C_CONTIGUOUS"]
        self._keep.append(array)
        return self._own(self.L.fj_new_direct_buffer(array.ctypes.data, array.size if capacity is None else capacity))

    def heap_buffer(self, capacity):
        return self._own(self.L.fj_new_heap_buffer(capacity))

    def read(self, handle, dtype):
        """The elements of a primitive array as they are now."""
        n = self.L.fj_length(handle)
        return np.frombuffer(C.string_at(self.L.fj_data(handle), n * np.dtype(dtype).itemsize), dtype).copy()

    def take_ints(self, handle):
        """A returned int[]: its elements; the host's hold on it ends."""
        a = self.read(handle, np.int32)
        self.L.fj_release(handle)
        return a

    def take_int_arrays(self, handle):
        """A returned int[][]."""
        out = [self.read(self.L.fj_object_element(handle, i), np.int32) for i in range(self.L.fj_length(handle))]
        self.L.fj_release(handle)
        return out

    def reset(self):
        """Between tests: nothing pending, nothing outstanding, every object made here released."""
        self.L.fj_exception_clear()
        self.L.fj_drop_outstanding()
        self.L.fj_fail_alloc(0)
        for h in reversed(self._owned):
            self.L.fj_release(h)
        self._owned, self._keep = [], []
        if self.stub:
            self.L.st_reset()
            self.L.st_script(5, 33, 4096, 0)
            self.L.st_set_error(b"scripted error")

    # ---- calls ----
    def counters(self):
        return {name: self.L.fj_get(i) for i, name in enumerate(COUNTERS)}

    def call(self, name, *args, fail_alloc=0):
        """The native method `name`; returns its result (an object result is host-owned: take_ints / take_int_arrays).  The exception it
        left stays pending (pending(), clear()); Runtime.last holds the counters of this call."""
        Runtime.called.add(name)
        self.L.fj_begin_call()
        self.L.fj_fail_alloc(fail_alloc)
        res = self._natives[name](self.env, None, *args)
        self.L.fj_end_call(res if SIGS[name][0] is _vp else None)
        self.last = self.counters()
        self.last["log"] = self.L.fj_violation_log().decode()
        return res

    def pending(self):
        """(class, message) of the pending exception, or None."""
        if not self.L.fj_get(COUNTERS.index("pending")):
            return None
        return self.L.fj_exception_class().decode(), self.L.fj_exception_message().decode()

    def clear(self):
        self.L.fj_exception_clear()

    def clean(self, max_locals=16):
        """What must hold after EVERY native call, failed or not; returns a description of what does not (empty: all is well)."""
        c, bad = self.last, []
        if c["violations"]:
            bad.append("violations: " + c["log"])
        if c["outstanding"]:
            bad.append("%d element pointer(s) not released" % c["outstanding"])
        if c["aborted_writes"]:
            bad.append("%d array(s) written through a pointer that was released with JNI_ABORT" % c["aborted_writes"])
        if c["peak_locals"] > max_locals:
            bad.append("peak of live local references %d > %d" % (c["peak_locals"], max_locals))
        if c["live_locals"]:
            bad.append("local references live after the call")
        return "; ".join(bad)

    # ---- the stub's record ----
    def stub_calls(self):
        """[(function name, {slot: value})] of the nq_* calls since the last reset() / st_reset."""
        out = []
        for i in range(min(self.L.st_ncalls(), 64)):
            fn = STUB_FUNCTIONS[self.L.st_call_fn(i)]
            rec = {slot: self.L.st_call_arg(i, j) for j, slot in enumerate(STUB_SLOTS[fn])}
            rec["pending"] = self.L.st_call_arg(i, PENDING_SLOT)
            out.append((fn, rec))
        return out
