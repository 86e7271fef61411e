#!/usr/bin/env python3
"""Writes tests/golden/radius_expected.json: per (cloud, radius) of tests/radius_ref.fixture_cases() the number of components of the radius
graph, the ten largest sizes, the number of edges and the sha256 of `comp` and of `count` (int32, little endian) -- computed by the NumPy
statement of DESIGN.md 8k alone; the library is never loaded.

Every case is cross-checked against scipy.spatial.cKDTree in float64 (query_pairs + csgraph.connected_components): the counts, the
components and their number must be equal.  The float32 statement and a float64 kd-tree agree for a reason only when no pair sits on the
radius, so a case in which any pair's float64 distance lies within 1e-6 (relative) of the radius is refused: choose another radius.

    python tools/capture_radius.py            # rewrites the file (needs no GPU; about a minute)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import radius_ref as R  # noqa: E402

MARGIN = 1e-6


def main():
    out = {}
    for name, (xyz, radius) in R.fixture_cases().items():
        cnt, comp, _, c = R.solve(xyz, radius)
        k_cnt, k_comp, k_c, nearest = R.kdtree(xyz, radius)
        if nearest <= MARGIN:
            sys.exit("%s: a pair lies within %.3g (relative) of the radius %g; choose another radius" % (name, nearest, radius))
        if not (np.array_equal(cnt, k_cnt) and np.array_equal(comp, k_comp) and c == k_c):
            sys.exit("%s: the statement and the kd-tree disagree (C %d against %d)" % (name, c, k_c))
        out[name] = dict(R.entry(cnt, comp, c), radius=radius, nearest_pair_to_radius=float("%.3g" % min(nearest, 1.0)))
        print(name, radius, c, out[name]["sizes"][:4], out[name]["pairs"], "%.2g" % nearest)
    path = os.path.join(ROOT, "tests", "golden", "radius_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
