#!/usr/bin/env python3
"""Writes tests/golden/rekey_expected.json (build container only): the synthetic scan of tests/rekey_ref.py re-keyed onto each of its
segmentations by the NumPy statement of DESIGN.md 8e, the tree written from that result, and the UNMODIFIED label producers of the
reference's dataset/scannet/util.py -- generate_real_labels, generate_weak_labels for `manual` and `maxseg` -- run over it: they accept
the files, and what they write and return is the expectation the project's own producers and rekey_scan are held to.

    python tools/capture_rekey.py
"""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import capture_prepare as cp  # noqa: E402
import rekey_ref as R  # noqa: E402

NUM_POINTS = 2000
STYLES = ("manual", "maxseg")


def main():
    import torch
    util = cp._load_reference_util()
    scan, ann = R.source_scan()
    manual = R.clicks_with_points(scan, ann)
    ply = cp.fake_plydata(scan)
    out = {"scan": dict(R.SCAN, V=int(scan.xyz.shape[0]), src_segments=int(np.unique(scan.seg_indices).shape[0]),
                        groups=len(ann["aggregation"]["segGroups"]), clicks=len(R.clicks_of(manual)))}
    for which in R.SEGMENTATIONS:
        new_seg = R.new_segmentation(scan, which)
        res = R.rekey(scan.seg_indices, new_seg, ann["aggregation"], manual, scan.name)
        e = {"report": res["report"], "winner": R.digest(res["vote"]["winner"]), "vertex_winner": R.digest(res["vote"]["vertex_winner"])}
        with tempfile.TemporaryDirectory(prefix="sgrekey_") as td:
            scene_path = R.write_tree(td, scan, ann["tsv"], new_seg, res)
            cwd = os.getcwd()
            os.chdir(td)
            real_randperm = torch.randperm
            try:
                torch.randperm = lambda n, *a, **k: torch.from_numpy(scan.perm[:n].copy())
                util.generate_pointcloud_pth(scene_path, 5, NUM_POINTS, ply)
                torch.randperm = real_randperm
                util.generate_seg_labels_and_ds_set(scene_path)
                util.generate_real_labels(scene_path)
                raw = os.path.join("label", "real", "raw", scan.name)
                for k in ("ins", "sem"):
                    e[f"real.{k}"] = R.digest(np.loadtxt(os.path.join(raw, f"{scan.name}.{k}.txt"), dtype=np.int64))
                for style in STYLES:
                    ret = util.generate_weak_labels(scene_path, ply, label_style=style, manual_label_path=os.path.join(td, "manual_label"))
                    e[f"{style}.ret"] = [int(x) for x in ret]
                    for k in ("ins", "sem"):
                        e[f"{style}.{k}"] = R.digest(np.loadtxt(os.path.join("label", "seg", style, "raw", scan.name, f"{scan.name}.{k}.txt"), dtype=np.int64))
            finally:
                torch.randperm = real_randperm
                os.chdir(cwd)
        from seggroup_amd.synthetic import _CATEGORIES
        ins, sem = R.labels_of(res, ann["aggregation"], dict(_CATEGORIES))
        assert R.digest(ins) == e["real.ins"] and R.digest(sem) == e["real.sem"], "the reference reads something else out of the written tree"
        out[which] = e
        print(which, e["report"], e["manual.ret"], e["maxseg.ret"], flush=True)
    path = os.path.join(REPO, "tests", "golden", "rekey_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
