#!/usr/bin/env python3
"""Writes tests/golden/pcseg_radius_expected.json: per case of tests/pcseg_radius_ref.fixture_cases() the number of pairs T and the sha256
of every stage of the statement of DESIGN.md 8l -- off, idx, the normals, the lexicographic edges and weights, the sorted edges and weights
and the final ids -- computed by the NumPy statement alone; the library is never loaded.  Digests and counts only.

Every case's pair list is cross-checked against scipy.spatial.cKDTree in float64 under 8k's rule: a case in which any pair's float64
distance lies within 1e-6 (relative) of the radius is refused.  Without scipy the cross-check is skipped and the file says so.

    python tools/capture_pcseg_radius.py            # rewrites the file (needs no GPU; a few minutes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pcseg_radius_ref as Q  # noqa: E402

MARGIN = 1e-6


def kdtree_pairs(xyz, radius):
    """-> (pairs a < b in lexicographic order, the smallest |d/r - 1| over all pairs) from a float64 kd-tree"""
    from scipy.spatial import cKDTree
    pts = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    r = float(np.float32(radius))
    near = cKDTree(pts).query_pairs(r * (1.0 + 1e-5), output_type="ndarray")
    d = np.sqrt(((pts[near[:, 0]] - pts[near[:, 1]]) ** 2).sum(1)) if near.shape[0] else np.zeros(0)
    nearest = float(np.abs(d / r - 1.0).min()) if d.size else np.inf
    e = near[d <= r]
    e = np.stack([e.min(1), e.max(1)], 1) if e.shape[0] else np.zeros((0, 2), np.int64)
    return e[np.lexsort((e[:, 1], e[:, 0]))], nearest


def main():
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    cases = {}
    for name, (xyz, radius) in Q.fixture_cases().items():
        r = Q.sorted_edges(xyz, radius)
        seg = Q.P.merge(r["edges"], r["w"], xyz.shape[0], 0.01, 20)
        entry = dict(Q.stage_digests(r, seg), N=int(xyz.shape[0]), radius=radius, segments=int(np.unique(seg).shape[0]))
        if have_scipy:
            e, nearest = kdtree_pairs(xyz, radius)
            if nearest <= MARGIN:
                sys.exit("%s: a pair lies within %.3g (relative) of the radius %g; choose another radius" % (name, nearest, radius))
            if not np.array_equal(e, r["lex_edges"].astype(np.int64)):
                sys.exit("%s: the statement and the kd-tree disagree (%d pairs against %d)" % (name, r["lex_edges"].shape[0], e.shape[0]))
            entry["nearest_pair_to_radius"] = float("%.3g" % min(nearest, 1.0))
        cases[name] = entry
        print(name, radius, entry["T"], entry["segments"], flush=True)
    out = {"kdtree_cross_check": "scipy.spatial.cKDTree, float64" if have_scipy else "skipped: scipy is not importable", "cases": cases}
    path = os.path.join(ROOT, "tests", "golden", "pcseg_radius_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
