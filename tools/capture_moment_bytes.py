#!/usr/bin/env python3
"""Writes tests/golden/moment_bytes.npz: what tests/test_gpu_moment_bytes.py's inputs give on the GPU, from a build that is NOT the one
under test -- the fixture pins the bytes of the deterministic sums and of the hypothesis draw across a change of the code, so it is
recorded from the commit before the change:

    git archive <parent> | tar -x -C DIR && make -C DIR/seggroup_amd/csrc
    python tools/capture_moment_bytes.py --package DIR [--out FILE]          # needs a GPU; a few seconds

The inputs are this tree's (the test module generates them); the package and its library are DIR's.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package", required=True, help="the built tree whose seggroup_amd is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "moment_bytes.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.package))
    import seggroup_amd
    import test_gpu_moment_bytes as T
    assert os.path.abspath(os.path.dirname(os.path.dirname(seggroup_amd.__file__))) == os.path.abspath(a.package), seggroup_amd.__file__
    out = {}
    for u in T.COUNTS:
        out.update(T.sums(u))
    out.update(T.label_sums())
    out.update(T.draws())
    np.savez(a.out, **out)
    print("wrote", a.out, "with", len(out), "arrays from", seggroup_amd.__file__)
    return 0


if __name__ == "__main__":
    sys.exit(main())
