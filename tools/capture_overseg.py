#!/usr/bin/env python3
"""Writes tests/golden/overseg_expected.json: per generated mesh of tests/overseg_ref.py the sha256 of seg_indices (little-endian
int32), the number of segments and the number of edges -- computed by the NumPy statement of the specification alone (the library is
not loaded).  The committed digests keep that reference and the library from drifting together: a change to either that moves a
result shows up against this file.

    python tools/capture_overseg.py            # rewrites the file (needs no GPU; the 150k lattice takes a few seconds)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overseg_ref as R  # noqa: E402


def main():
    out = {}
    for name, (xyz, faces) in R.case_meshes(include_large=True).items():
        _, edges, w = R.sorted_edges(xyz, faces)
        seg = R.merge(edges, w, xyz.shape[0])
        out[name] = {"V": int(xyz.shape[0]), "F": int(faces.shape[0]), "edges": int(edges.shape[0]), "segments": int(np.unique(seg).shape[0]),
                     "ties": int((np.diff(w) == 0).sum()) if w.shape[0] > 1 else 0, "negative_weights": int((w < 0).sum()),
                     "sha256": R.digest(seg)}
        print(name, out[name])
    xyz, faces = R.case_meshes()["room_j5e-4"]
    _, edges, w = R.sorted_edges(xyz, faces)
    out["room_j5e-4"]["sweep"] = {f"{k:g}/{m}": R.digest(R.merge(edges, w, xyz.shape[0], k, m)) for k, m in R.PARAM_SWEEP}
    path = os.path.join(ROOT, "tests", "golden", "overseg_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
