"""The CPU oracle is the reference of tests/test_gpu_tiny_geometry.py, so it is pinned itself at those sizes: tests/c/oracle_tiny_main.c
walks the shape grid through nqo_convert, nqo_pnnquan and nqo_dither_tiled against buffers malloc'ed to the exact size, built plain and
with the address and undefined-behaviour sanitizers.  Both runs must end clean, throw nowhere and print the same checksum of every
output.  Stand-alone executables on the CPU: nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("oracle_tiny_san" if sanitize else "oracle_tiny"))
    cmd = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "oracle"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "oracle_tiny_main.c"), os.path.join(ROOT, "oracle", "nq_oracle.c"), "-lm"]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(tmp_path, sanitize):
    exe, r = _build(tmp_path, sanitize)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    m = re.search(r"oracle tiny: (\d+) converts, (\d+) tiled dithers, (\d+) throws, checksum ([0-9a-f]{16})", r.stdout)
    assert m, r.stdout[-1500:]
    # 2 kinds x 6 generators x 26 shapes x 5 K x 2 dither converts; K > 2 (3 of the 5) goes through 4 tiles as well
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (3120, 7488, 0)
    return m.group(4)


def test_oracle_on_the_tiny_grid_plain_and_under_asan_ubsan(tmp_path):
    plain, sanitized = _run(tmp_path, False), _run(tmp_path, True)
    assert plain == sanitized, "the sanitized build computes something else: %s / %s" % (plain, sanitized)
