#!/usr/bin/env python3
"""Writes tests/golden/components_expected.json: per graph of tests/components_ref.py the number of components, the largest sizes and the
sha256 of `comp` (int32, little endian); the speck cloud's kNN graph at every cut and the thinned large cloud's at three voxel edges and at one --
computed by the NumPy statement of DESIGN.md 8j alone (the library is not loaded; the kNN tables are tests/pcseg_ref.py's).  The committed
digests keep that reference and the library from drifting together.

    python tools/capture_components.py            # rewrites the file (needs no GPU; under a minute)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import components_ref as R  # noqa: E402
import pcseg_ref  # noqa: E402
import thin_ref  # noqa: E402


def entry(comp, count):
    return {"V": int(comp.shape[0]), "C": int(count), "sizes": R.sizes_desc(comp)[:10], "sha256": R.digest(comp)}


def big_thinned():
    """the 5,403 points of 8i's test: thin_ref.big_cloud() thinned at 0.05"""
    xyz, _ = thin_ref.big_cloud()
    rep, _, _ = thin_ref.thin(xyz, 0.05)
    return xyz[rep]


def main():
    out = {"graphs": {}, "specks": {}}
    for name, case in R.case_graphs().items():
        comp, _, count = R.solve(case)
        out["graphs"][name] = entry(comp, count)
        print(name, count, out["graphs"][name]["sizes"][:4])
    xyz, _ = R.speck_cloud()
    table = pcseg_ref.knn_table(xyz, 10)
    for cut in R.CUTS:
        comp, _, count = R.from_knn(xyz, table, cut)
        out["specks"]["%g" % cut] = entry(comp, count)
        print("specks", cut, count, out["specks"]["%g" % cut]["sizes"])
    pts = big_thinned()
    table = pcseg_ref.knn_table(pts, 10)
    for key, cut in (("big_thinned", 3 * 0.05), ("big_thinned_tight", 0.05)):
        comp, _, count = R.from_knn(pts, table, cut)
        out[key] = entry(comp, count)
        print(key, out[key])
    path = os.path.join(ROOT, "tests", "golden", "components_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
