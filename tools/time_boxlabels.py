#!/usr/bin/env python3
"""Points in boxes, measured -> profiles/boxlabels_time.json.

    python tools/time_boxlabels.py [--repeats 5] [--out profiles/boxlabels_time.json]
    python tools/time_boxlabels.py --table profiles/boxlabels_time.json      # prints the markdown table of DESIGN.md 8v (no GPU needed)

One process, one GPU, one stream.  sg_points_in_boxes has no stage timer of its own, so every library call is bracketed by a pair of
torch.cuda.Event on the call's stream: a warm-up, then the median (min .. max) of the repeats.  Points are uniform in a 2 m cube a scene,
boxes those of tests/test_gpu_boxlabels.py (sizes 0.05 .. 0.5, even boxes with a yaw, odd boxes tilted).  Shapes: 150,000 points x 32
boxes, 150,000 x 1,024, 2^24 x 32, and 256 scenes of 150,000 x 32 in calls of at most 2^24 points (the sum over the calls).  Every shape is
timed without and with the per-box counts (d_held).  The expected ranges are written into the file BEFORE the first run; afterwards the
file says which of them missed.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE_POINTS = 150_000
MAX_POINTS = 1 << 24
# name, points a scene, boxes a scene, scenes, the expected range in us of the plain entry
SHAPES = (("150,000 x 32", SCENE_POINTS, 32, 1, (50.0, 110.0)), ("150,000 x 1,024", SCENE_POINTS, 1024, 1, (250.0, 450.0)),
          ("2^24 x 32", MAX_POINTS, 32, 1, (900.0, 1800.0)), ("256 scenes of 150,000 x 32", SCENE_POINTS, 32, 256, (2200.0, 4500.0)))
EXPECTED = ("a test of one point against one box is about 21 double operations (3 differences, 9 products, 6 sums, 3 comparisons of a "
            "magnitude) on 16 doubles the whole wave reads from LDS at one address; 8s.6 / 8t.6 saw 1.5e13 double operations a second, and 8u.6 a "
            "floor of 60 us for a call of one memset, three uploads, two check kernels and the flag's copy.  This call has ONE upload (the "
            "workgroup table, with the flag word in it), the preparation kernel, the test kernel and the flag's copy, so its floor should be "
            "40 to 70 us.  150,000 x 32 is 4.8e6 tests, 1e8 operations, 7 us at that rate: the floor and little else, 50 to 110 us.  "
            "150,000 x 1,024 is 1.5e8 tests, 3.2e9 operations, 215 us, over eight LDS tiles a workgroup: 250 to 450 us.  2^24 x 32 is 5.4e8 "
            "tests, 1.1e10 operations, 750 us, plus 200 MB read and 200 MB written (100 us at 4 TB/s, overlapped) and a table of 65,537 "
            "entries (1 MB from pageable memory, 100 to 200 us before the first launch): 0.9 to 1.8 ms.  256 scenes of 150,000 x 32 are three "
            "calls of 111, 111 and 34 scenes, 1.2e9 tests, 2.6e10 operations, 1.7 ms, plus three floors and tables: 2.2 to 4.5 ms in all.  "
            "The per-box counts add a ballot per box and wave and an LDS add where a box holds something: 5 to 20 % on top")
NOT_MEASURED = ["real scans (most points of a room are in no box or one: the same work, the test has no early exit)", "boxes near 2^20 a call",
                "several streams in flight", "the command's file work, its label_boxes calls (8t.6) and its vote (8e)"]


def boxes(seed, k, smax=0.5):
    rng = np.random.RandomState(seed)
    c = (rng.rand(k, 3) * 2.0).astype(np.float32).astype(np.float64)
    s = 0.05 + (smax - 0.05) * rng.rand(k, 3)
    R = np.zeros((k, 3, 3))
    for j in range(k):
        if j % 2 == 0:
            a = rng.rand() * 2.0 * np.pi
            R[j] = [[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
        else:
            R[j] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return np.ascontiguousarray(np.concatenate([c, s, R.reshape(k, 9)], 1))


def spread(rows, digits=1):
    a = np.asarray(rows, np.float64)
    return dict(median=round(float(np.median(a)), digits), min=round(float(a.min()), digits), max=round(float(a.max()), digits))


def measure(repeats):
    import torch
    from seggroup_amd import hip
    dev = torch.device("cuda:0")
    lib = hip.lib()
    stream = torch.cuda.Stream(device=dev)
    rows = []
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for name, n, k, scenes, _ in SHAPES:
            per_call = max(1, MAX_POINTS // n)
            parts = [min(per_call, scenes - at) for at in range(0, scenes, per_call)]
            most = max(parts)
            d_xyz = torch.rand((n * most, 3), dtype=torch.float32, device=dev) * 2.0          # every call of a shape reads the same scenes' points
            d_box = torch.from_numpy(boxes(1, k * most)).to(dev)
            out = torch.empty((3, n * most), dtype=torch.int32, device=dev)
            d_held = torch.empty(k * most, dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(lib.sg_points_in_boxes_ws_bytes(n * most, k * most, most)), 256), dtype=torch.uint8, device=dev)
            offs = {s: ((np.arange(s + 1) * n).astype(np.int32), (np.arange(s + 1) * k).astype(np.int32)) for s in set(parts)}

            def call(held):
                for s in parts:
                    off_p, off_b = offs[s]
                    hip.check(lib.sg_points_in_boxes(d_xyz.data_ptr(), 3, n * s, d_box.data_ptr(), k * s, off_p.ctypes.data, off_b.ctypes.data, s, 0.0,
                                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), d_held.data_ptr() if held else None,
                                                     ws.data_ptr(), ws.numel(), stream.cuda_stream))

            row = dict(name=name, points=n * scenes, boxes_a_scene=k, scenes=scenes, calls=len(parts), tests=n * k * scenes, us={})
            for label, held in (("plain", False), ("with_held", True)):
                call(held)                                                     # the warm-up
                times = []
                for _ in range(repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call(held)
                    e1.record(stream)
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                row["us"][label] = spread(times)
            count = out[0, :n * parts[-1]]
            row["shares"] = [round(float((count == 0).double().mean().item()), 3), round(float((count == 1).double().mean().item()), 3),
                             round(float((count > 1).double().mean().item()), 3)]
            row["tests_per_second"] = float("%.3g" % (row["tests"] / (row["us"]["plain"]["median"] * 1e-6)))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_xyz, d_box, out, d_held, ws
    return dict(shapes=rows)


def missed(measured):
    out = []
    for (name, _, _, _, (lo, hi)), row in zip(SHAPES, measured["shapes"]):
        m = row["us"]["plain"]["median"]
        if not lo <= m <= hi:
            out.append("%s: %.1f us, %s the expected %.0f to %.0f us" % (name, m, "below" if m < lo else "above", lo, hi))
        extra = row["us"]["with_held"]["median"] / m - 1.0
        if not 0.05 <= extra <= 0.20:
            out.append("%s: the per-box counts add %.0f %%, %s the expected 5 to 20 %%" % (name, 100.0 * extra, "below" if extra < 0.05 else "above"))
    return out


def table(doc):
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    lines = ["| shape | tests | calls | expected | three outputs | with `d_held` | tests a second |", "|---|---|---|---|---|---|---|"]
    for (_, _, _, _, (lo, hi)), r in zip(SHAPES, doc["measured"]["shapes"]):
        lines.append(f"| {r['name']} | {r['tests']:,} | {r['calls']} | {lo:,.0f} to {hi:,.0f} | {us(r['us']['plain'])} | {us(r['us']['with_held'])} | "
                     f"{r['tests_per_second']:.3g} |")
    lines += ["", "µs between events: median (min .. max).", "", "Expected before the run: " + doc["expected"] + ".", "",
              "Missed: " + ("; ".join(doc["missed"]) if doc["missed"] else "nothing") + ".", "", "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def write(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxlabels_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; torch.cuda.Event pairs around every library call",
               expected=EXPECTED, expected_us={name: list(r) for name, _, _, _, r in SHAPES}, not_measured=list(NOT_MEASURED), measured=None,
               missed=None)
    write(a.out, doc)                                                          # the expectations are on disk before the first run
    doc["measured"] = measure(a.repeats)
    doc["missed"] = missed(doc["measured"])
    write(a.out, doc)
    print(table(doc))


if __name__ == "__main__":
    main()
