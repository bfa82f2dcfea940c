"""Reruns a walk of tests/test_gpu_handle_lifecycle.py (part B) and prints the first step whose result differs:

    python tests/lifecycle_replay.py SEED [STEPS] [lab|rgb]

STEPS (default 150) cuts the walk down to its prefix; a walk is the same for the same seed, so the shortest failing prefix is found by
trying smaller values.  Needs a GPU.  A helper, not a test module."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv):
    if not 2 <= len(argv) <= 4:
        print(__doc__)
        return 2
    seed = int(argv[1])
    steps = int(argv[2]) if len(argv) > 2 else 150
    kind = {"lab": 1, "rgb": 0}[argv[3] if len(argv) > 3 else "lab"]
    import nquant.android_amd as nq
    from test_gpu_handle_lifecycle import run_walk
    last = [None]

    def report(i, step):
        last[0] = (i, step)
    try:
        run_walk(nq, kind, seed, steps, report=report)
    except AssertionError as e:
        print("first differing step: %d %r\n%s" % (last[0][0], last[0][1], e))
        return 1
    print("walk %d: %d steps, every result as expected" % (seed, steps))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
