#!/usr/bin/env python3
"""Writes tests/golden/pcseg_expected.json: per generated cloud of tests/pcseg_ref.py the sha256 of every stage (kNN table, normals,
sorted edges, weights, seg_indices), the counts and, for the rooms, the quality figures -- computed by the NumPy statement of the
specification alone (the library is not loaded).  The committed digests keep that reference and the library from drifting together: a
change to either that moves a result shows up against this file.

    python tools/capture_pcseg.py            # rewrites the file (needs no GPU; the 20k room takes a few seconds)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pcseg_ref as R  # noqa: E402

SWEEP_CASE = "room_j5e-4"
VIEWPOINT = (0.4, 0.3, 3.0)


def main():
    out = {}
    clouds = R.case_clouds(include_large=True)
    for name, (xyz, plane) in clouds.items():
        r = R.sorted_edges(xyz, 10)
        seg = R.merge(r["edges"], r["w"], xyz.shape[0])
        w = r["w"]
        e = {"N": int(xyz.shape[0]), "edges": int(w.shape[0]), "segments": int(np.unique(seg).shape[0]),
             "ties": int((np.diff(w) == 0).sum()), "negative_weights": int((w < 0).sum()),
             "self_pairs": int((r["knn"][:, 1:] == np.arange(xyz.shape[0])[:, None]).sum())}
        e.update(R.stage_digests(r, seg))
        if name not in R.DEGENERATE:
            ang, share = R.eigh_check(xyz, r["knn"], r["normals"])
            e["max_angle_rad"], e["gap_share"] = ang, share
        if plane is not None:
            e["purity"] = R.purity(seg, plane)
        out[name] = e
        print(name, e)
    xyz, _ = clouds[SWEEP_CASE]
    r = R.sorted_edges(xyz, 10)
    out[SWEEP_CASE]["sweep"] = {f"{k:g}/{m}": R.digest(R.merge(r["edges"], r["w"], xyz.shape[0], k, m)) for k, m in R.PARAM_SWEEP}
    out[SWEEP_CASE]["k"] = {}
    for k in (5, 20):
        rk = R.sorted_edges(xyz, k)
        out[SWEEP_CASE]["k"][str(k)] = R.stage_digests(rk, R.merge(rk["edges"], rk["w"], xyz.shape[0]))
    rv = R.sorted_edges(xyz, 10, viewpoint=VIEWPOINT, table=r["knn"])
    out[SWEEP_CASE]["viewpoint"] = dict(R.stage_digests(rv, R.merge(rv["edges"], rv["w"], xyz.shape[0])), at=list(VIEWPOINT),
                                        flipped=int((rv["normals"] != r["normals"]).any(1).sum()))
    path = os.path.join(ROOT, "tests", "golden", "pcseg_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
