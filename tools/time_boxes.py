#!/usr/bin/env python3
"""Boxes of labelled points, measured stage by stage -> profiles/boxes_time.json.

    python tools/time_boxes.py [--repeats 5] [--out profiles/boxes_time.json]
    python tools/time_boxes.py --table profiles/boxes_time.json      # prints the markdown table of DESIGN.md 8t (no GPU needed)

One process, one GPU, one stream.  The cloud is make_room_scan(400, 375) (150,000 points on a 0.04 lattice with a jitter of 5e-4) under
three label vectors: 1,500 labels (the scan's own seg_indices name three parts only, so a label here is a run of 100 consecutive lattice
vertices: a strip of one lattice row), every point its own label, and one label for all.  The stages -- sg_label_index, sg_label_moments,
sg_label_yaw_boxes at A = 90 and A = 256, sg_label_frame_extents -- are timed by the library's own events on the stream
(hip.stage_timer("label")), the median (min .. max) of the repeats after a warm-up; label_boxes (yaw, 90) by the host's clock stands beside
them.  EXPECTED was written down before the first run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANGLES = (90, 256)
EXPECTED = ("the sweep is about 8 N A uncontracted double operations, 1.1e8 at 150,000 x 90 -- a fiftieth of the 5e9 that sg_plane_ransac's "
            "count does in 337 us (8s.6) -- so with 1,500 labels 10 to 30 us at A = 90 and 20 to 60 us at A = 256, launches and the two scans "
            "of the chunk table included; with one label 147 workgroups do not fill 256 CUs and a second kernel folds 147 partial rows, so "
            "about the same; with every point its own label 150,000 workgroups of one point each are all overhead, 100 to 300 us.  The "
            "index is three radix passes over 150,000 keys, the unique compaction and a dozen launches: 60 to 120 us, the largest device "
            "stage wherever the labels are not one per point.  Moments and frame extents stream 150,000 points once: 10 to 30 us each, more "
            "with one point per workgroup.  label_boxes by the host's clock: 1 to 3 ms -- four synchronising calls, half a dozen downloads "
            "and the uploads of the Python layer -- so the Python layer, not a kernel, dominates the call")
NOT_MEASURED = ["real scans", "clouds near the 2^24-point limit", "several streams in flight", "kind pca's host loop over the labels (sg_box_axes per label)",
                "the command (PLY read, .npz and PLY write)"]


def spread(rows):
    a = np.asarray(rows, np.float64)
    return dict(median=round(float(np.median(a)), 1), min=round(float(a.min()), 1), max=round(float(a.max()), 1))


def measure(repeats):
    import torch
    from seggroup_amd import boxes, hip, synthetic
    dev = "cuda:0"
    room = np.ascontiguousarray(synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz, dtype=np.float32)
    d_xyz = torch.from_numpy(room).to(dev)
    n = int(room.shape[0])
    vectors = {"1,500 labels": (np.arange(n) // 100).astype(np.int32), "every point its own": np.arange(n, dtype=np.int32),
               "one label": np.zeros(n, np.int32)}
    out = dict(points=n, clouds=[])
    for name, lab in vectors.items():
        d_lab = torch.from_numpy(lab).to(dev)
        state = {}

        def one_round(t=None):
            got = {}
            state["idx"] = idx = boxes.label_index(d_lab, device=dev)
            if t:
                got["index"] = t.read()[t.names.index("index")]
            boxes.label_moments(d_xyz, idx, device=dev)
            if t:
                got["moments"] = t.read()[t.names.index("moments")]
            for a in ANGLES:
                boxes.yaw_boxes(d_xyz, idx, a, device=dev)
                if t:
                    got["yaw, A = %d" % a] = t.read()[t.names.index("yaw")]
            boxes.frame_extents(d_xyz, idx, state["frames"], device=dev)
            if t:
                got["frame"] = t.read()[t.names.index("frame")]
            return got

        labels = int(np.unique(lab).size)
        state["frames"] = torch.eye(3, dtype=torch.float64, device=dev).repeat(labels, 1, 1)
        with hip.stage_timer("label") as timer:
            one_round()                                                       # the warm-up
            rows = [one_round(timer) for _ in range(repeats)]
        row = dict(name=name, labels=labels, stages_us={k: spread([r[k] for r in rows]) for k in rows[0]})
        boxes.label_boxes(d_xyz, d_lab, "yaw", 90, device=dev)
        torch.cuda.synchronize()
        wall = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            found = boxes.label_boxes(d_xyz, d_lab, "yaw", 90, device=dev)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        row.update(label_boxes_ms=dict(median=round(float(np.median(wall)), 2), min=round(min(wall), 2), max=round(max(wall), 2)),
                   boxes=int(found.values.shape[0]))
        out["clouds"].append(row)
        print(json.dumps(row), flush=True)
    return out


def table(doc):
    m = doc["measured"]
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    stages = list(m["clouds"][0]["stages_us"])
    lines = [f"| {m['points']:,} points | " + " | ".join(stages) + " | `label_boxes` (yaw, 90), host clock, ms |", "|---" * (len(stages) + 2) + "|"]
    for r in m["clouds"]:
        w = r["label_boxes_ms"]
        lines.append(f"| {r['name']} (L = {r['labels']:,}) | " + " | ".join(us(r["stages_us"][s]) for s in stages) +
                     f" | {w['median']:,} ({w['min']:,} .. {w['max']:,}) |")
    lines += ["", "µs between events: median (min .. max).", "", "Expected before the run: " + doc["expected"] + ".", "",
              "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream", expected=EXPECTED, not_measured=list(NOT_MEASURED),
               measured=measure(a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
