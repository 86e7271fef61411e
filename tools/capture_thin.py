#!/usr/bin/env python3
"""Writes tests/golden/thin_expected.json: per cloud of tests/thin_ref.py and voxel edge the number of occupied voxels and the sha256 of
`rep` and `thin_of_point` (int32, little endian), the large cloud at 0.05, and the quality figures of the thinned-and-lifted
segmentation -- computed by the NumPy statement of the specification alone (the library is not loaded).  The committed digests keep that
reference and the library from drifting together.

    python tools/capture_thin.py            # rewrites the file (needs no GPU; a few seconds)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pcseg_ref  # noqa: E402
import thin_ref as T  # noqa: E402


def entry(xyz, h):
    rep, top, _ = T.thin(xyz, h)
    cells, largest = T.stats(xyz, h, rep, top)
    return {"N": int(xyz.shape[0]), "M": int(rep.shape[0]), "rep": T.array_digest(rep), "thin_of_point": T.array_digest(top), "cells": cells,
            "largest_voxel": largest, "identity": bool(rep.shape[0] == xyz.shape[0])}


def quality(xyz, plane, h):
    seg, seg_thin, _, _ = T.segment_thinned(xyz, h)
    return {"purity": pcseg_ref.purity(seg, plane), "segments": int(np.unique(seg_thin).shape[0]), "sha256": T.array_digest(seg)}


def main():
    out = {"clouds": {}}
    for name, xyz in T.case_clouds().items():
        out["clouds"][name] = {"%g" % h: entry(xyz, h) for h in T.VOXELS}
        print(name, {h: e["M"] for h, e in out["clouds"][name].items()})
    big, bplane = T.big_cloud()
    out["big"] = dict(entry(big, 0.05), quality=quality(big, bplane, 0.05))
    xyz, plane = pcseg_ref.case_clouds(include_large=True)["room_20k"]
    out["room_20k_quality"] = quality(xyz, plane, 0.05)
    print("big", out["big"], "room_20k", out["room_20k_quality"])
    path = os.path.join(ROOT, "tests", "golden", "thin_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
