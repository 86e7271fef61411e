#!/usr/bin/env python3
"""Box IoU and best partners, measured -> profiles/boxap_time.json.

    python tools/time_boxap.py [--repeats 5] [--out profiles/boxap_time.json]
    python tools/time_boxap.py --table profiles/boxap_time.json      # prints the markdown table of DESIGN.md 8u (no GPU needed)

One process, one GPU, one stream.  sg_box_iou and sg_box_best have no stage timer of their own, so every library call is bracketed by a
pair of torch.cuda.Event on the call's stream: a warm-up, then the median (min .. max) of the repeats.  The boxes are those of
tests/test_gpu_boxap.py: a 2 m cube a scene, sizes 0.05 .. 1.55, any yaw -- nearly every pair of a scene overlaps, the costly case.
Shapes: 64 x 64, 1,024 x 1,024 and 4,096 x 4,096 in one scene, and 1,024 scenes of 32 x 32.  The command's share: match_batch (one
sg_box_best over 256 scenes of 30 predictions x 30 ground-truth boxes in 18 classes) by the host's clock, beside the library call alone.
EXPECTED was written down before the first run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("64 x 64", 64, 64, 1), ("1,024 x 1,024", 1024, 1024, 1), ("4,096 x 4,096", 4096, 4096, 1), ("1,024 scenes of 32 x 32", 32, 32, 1024))
EXPECTED = ("a pair is about 200 double operations (16 products and sums for the corners, a distance per edge over four sides, a division and "
            "two products per crossing, the fan, the volumes) but about 2,500 instructions: every append is eight predicated moves of two "
            "doubles, 22 edge slots with up to two appends each -- the price of keeping the polygon out of scratch.  8s.6 saw 5e9 double "
            "operations in 337 us and 8t.6 the same rate for the sweep, 1.5e13 a second.  At that rate 4,096 x 4,096 (1.7e7 pairs, 4e10 "
            "instructions) is 2.8 ms: 1.5 to 4 ms for sg_box_iou, which also writes 134 MB; 1,024 x 1,024 a sixteenth, 100 to 250 us; 1,024 "
            "scenes of 32 x 32 are the same million pairs plus a ten-step bisection a thread: 100 to 300 us; 64 x 64 is sixteen workgroups "
            "under the call's floor -- a memset, three uploads, two check kernels, the flag's copy: 30 to 60 us, as the chunk table's floor "
            "in 8t.6 (about 40 us for nine operations).  sg_box_best: a wave a box of A.  64 x 64 the same floor, 30 to 60 us; 1,024 x 1,024 is "
            "1,024 waves, one a SIMD, of 16 turns with nothing to hide latency behind: 100 to 250 us; 4,096 x 4,096 four waves a SIMD of 64 "
            "turns: 1 to 3 ms, no faster than sg_box_iou although it writes nothing; 1,024 scenes of 32 x 32 are 32,768 waves with half "
            "their lanes idle: 150 to 400 us.  match_batch on 256 scenes of 30 x 30: the library call 40 to 80 us, the Python layer around it "
            "(concatenations, two uploads of classes, two downloads) 0.3 to 1 ms, so the host dominates")
NOT_MEASURED = ["real scans' boxes (most pairs of a room do not overlap: fewer crossings, fewer divisions)", "sets near 2^20 boxes a side",
                "several streams in flight", "the command's file work and its label_boxes calls (8t.6 has those)"]


def boxes(seed, k):
    rng = np.random.RandomState(seed)
    c = (rng.rand(k, 3) * 2.0).astype(np.float32).astype(np.float64)
    s = 0.05 + 1.5 * rng.rand(k, 3)
    yaw = rng.rand(k) * 2.0 * np.pi
    return np.ascontiguousarray(np.concatenate([c, s, np.cos(yaw)[:, None], np.sin(yaw)[:, None]], 1))


def spread(rows, digits=1):
    a = np.asarray(rows, np.float64)
    return dict(median=round(float(np.median(a)), digits), min=round(float(a.min()), digits), max=round(float(a.max()), digits))


def measure(repeats):
    import torch
    from seggroup_amd import boxap, hip
    dev = torch.device("cuda:0")
    lib = hip.lib()
    stream = torch.cuda.Stream(device=dev)
    out = dict(shapes=[])
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for name, ka, kb, scenes in SHAPES:
            a, b = boxes(1, ka * scenes), boxes(2, kb * scenes)
            off_a, off_b = (np.arange(scenes + 1) * ka).astype(np.int32), (np.arange(scenes + 1) * kb).astype(np.int32)
            d_a, d_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            pairs = ka * kb * scenes
            d_iou = torch.empty(pairs, dtype=torch.float64, device=dev)
            d_best = torch.empty(ka * scenes, dtype=torch.int32, device=dev)
            d_top = torch.empty(ka * scenes, dtype=torch.float64, device=dev)
            ws = torch.empty(max(int(lib.sg_box_iou_ws_bytes(ka * scenes, kb * scenes, scenes)), 256), dtype=torch.uint8, device=dev)
            calls = {
                "sg_box_iou": lambda: lib.sg_box_iou(d_a.data_ptr(), ka * scenes, d_b.data_ptr(), kb * scenes, off_a.ctypes.data, off_b.ctypes.data,
                                                     scenes, d_iou.data_ptr(), pairs, ws.data_ptr(), ws.numel(), stream.cuda_stream),
                "sg_box_best": lambda: lib.sg_box_best(d_a.data_ptr(), ka * scenes, d_b.data_ptr(), kb * scenes, None, None, off_a.ctypes.data,
                                                       off_b.ctypes.data, scenes, d_best.data_ptr(), d_top.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       stream.cuda_stream)}
            row = dict(name=name, pairs=pairs, us={})
            for entry, call in calls.items():
                hip.check(call())                                              # the warm-up
                times = []
                for _ in range(repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    hip.check(call())
                    e1.record(stream)
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                row["us"][entry] = spread(times)
            row["overlapping"] = round(float((d_top > 0).double().mean().item()), 3)
            out["shapes"].append(row)
            print(json.dumps(row), flush=True)
    # the command's share: one batch of 256 scenes
    rng = np.random.RandomState(3)
    batch = [boxap.SceneBoxes(boxes(10 + k, 30), rng.randint(0, 18, 30).astype(np.int32), boxes(500 + k, 30), rng.randint(0, 18, 30).astype(np.int32), None)
             for k in range(256)]
    boxap.match_batch(batch, dev)
    wall, table = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = boxap.match_batch(batch, dev)
        wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        boxap.evaluate(*got)
        table.append((time.perf_counter() - t0) * 1e3)
    a, b = np.concatenate([s.pred for s in batch]), np.concatenate([s.gt for s in batch])
    off = (np.arange(257) * 30).astype(np.int32)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        d_a, d_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        d_ca = torch.from_numpy(np.concatenate([s.pred_cls for s in batch])).to(dev)
        d_cb = torch.from_numpy(np.concatenate([s.gt_cls for s in batch])).to(dev)
        d_best = torch.empty(a.shape[0], dtype=torch.int32, device=dev)
        d_top = torch.empty(a.shape[0], dtype=torch.float64, device=dev)
        ws = torch.empty(max(int(lib.sg_box_best_ws_bytes(a.shape[0], b.shape[0], 256)), 256), dtype=torch.uint8, device=dev)
        times = []
        for k in range(repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            hip.check(lib.sg_box_best(d_a.data_ptr(), a.shape[0], d_b.data_ptr(), b.shape[0], d_ca.data_ptr(), d_cb.data_ptr(), off.ctypes.data,
                                      off.ctypes.data, 256, d_best.data_ptr(), d_top.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))
            e1.record(stream)
            e1.synchronize()
            if k:
                times.append(e0.elapsed_time(e1) * 1e3)
    out["command_batch"] = dict(scenes=256, predictions=int(a.shape[0]), ground_truth=int(b.shape[0]), sg_box_best_us=spread(times),
                                match_batch_ms=spread(wall, 3), evaluate_ms=spread(table, 3))
    print(json.dumps(out["command_batch"]), flush=True)
    return out


def table(doc):
    m = doc["measured"]
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    lines = ["| shape | pairs | `sg_box_iou` | `sg_box_best` |", "|---|---|---|---|"]
    for r in m["shapes"]:
        lines.append(f"| {r['name']} | {r['pairs']:,} | {us(r['us']['sg_box_iou'])} | {us(r['us']['sg_box_best'])} |")
    c = m["command_batch"]
    lines += ["", "µs between events: median (min .. max).", "",
              f"The command's batch ({c['scenes']} scenes, {c['predictions']:,} predictions, {c['ground_truth']:,} ground-truth boxes, classes): "
              f"`sg_box_best` {us(c['sg_box_best_us'])} µs; `match_batch` {c['match_batch_ms']['median']} ms and `evaluate` {c['evaluate_ms']['median']} ms "
              "by the host's clock.", "", "Expected before the run: " + doc["expected"] + ".", "", "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxap_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; torch.cuda.Event pairs around every library call",
               expected=EXPECTED, not_measured=list(NOT_MEASURED), measured=measure(a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
