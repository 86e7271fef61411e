#!/usr/bin/env python3
"""Writes tests/golden/tool_bytes.npz: what tests/test_gpu_tool_bytes.py's calls give on the GPU, from a build that is NOT the one under
test -- the fixture pins the outputs of the pose tools and of the batch commands across a change of the layers above the kernels, so it
is recorded from the commit before the change:

    git archive <parent> | tar -x -C DIR && make -C DIR/seggroup_amd/csrc
    python tools/capture_tool_bytes.py --package DIR [--out FILE]          # needs a GPU; under a minute

The inputs are this tree's (the test module builds them); the package and its library are DIR's.  Everything is recorded twice, and a key
whose two recordings differ is named and left out: it is not byte-stable in the recorded build itself.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package", required=True, help="the built tree whose seggroup_amd is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tool_bytes.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.package))
    import seggroup_amd
    import test_gpu_tool_bytes as T
    assert os.path.abspath(os.path.dirname(os.path.dirname(seggroup_amd.__file__))) == os.path.abspath(a.package), seggroup_amd.__file__
    takes = []
    for _ in range(2):
        out = {}
        for part in (T.icps, T.registration, T.planes_found, T.boxes_found):
            out.update(part())
        with tempfile.TemporaryDirectory() as tmp:
            out.update(T.commands(tmp))
        takes.append({k: np.asarray(v) for k, v in out.items()})
    unstable = sorted(k for k, v in takes[0].items() if v.dtype != takes[1][k].dtype or v.tobytes() != takes[1][k].tobytes())
    for k in unstable:
        print("NOT byte-stable between two runs of", seggroup_amd.__file__, ":", k)
    np.savez_compressed(a.out, **{k: v for k, v in takes[0].items() if k not in unstable})
    print("wrote", a.out, "with", len(takes[0]) - len(unstable), "arrays from", seggroup_amd.__file__)
    return 0


if __name__ == "__main__":
    sys.exit(main())
