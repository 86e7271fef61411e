#!/usr/bin/env python3
"""Non-maximum suppression of boxes, measured -> profiles/boxnms_time.json.

    python tools/time_boxnms.py [--repeats 5] [--out profiles/boxnms_time.json]
    python tools/time_boxnms.py --table profiles/boxnms_time.json      # prints the markdown table of DESIGN.md 8w (no GPU needed)

One process, one GPU, one stream.  sg_box_nms has no stage timer of its own, so every library call is bracketed by a pair of
torch.cuda.Event on the call's stream (8u.6's method): a warm-up, then the median (min .. max) of the repeats.  Boxes are the proposals
of tests/boxnms_ref.py (ceil(n/8) objects in a 2 m cube, each repeated 8 times with jitter; scores round(rand, 2)), class-agnostic, at
an IoU of 0.25.  Shapes: one scene of 256, 1,024, 4,096 and 16,384 boxes, 1,024 scenes of 512 (a detector's raw output) and 256 scenes
of 30 (the command's batch).  Events on the caller's stream cannot separate the four kernels of one call; the second column of times
runs the same shape at an IoU of 0.999, where nothing is suppressed: the mask kernel does the same work, every row is kept, and the
scan ORs every row -- its worst case -- so the difference bounds what the scan's row passes cost.  The expected ranges are written into
the file BEFORE the first run -- of the first build of the kernels, whose medians the file keeps beside them --; afterwards the file says
which of them missed.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IOU = 0.25
# name, boxes a scene, scenes, the expected range in us at IoU 0.25
SHAPES = (("256", 256, 1, (90.0, 200.0)), ("1,024", 1024, 1, (130.0, 350.0)), ("4,096", 4096, 1, (500.0, 1200.0)),
          ("16,384", 16384, 1, (4000.0, 11000.0)), ("1,024 scenes of 512", 512, 1024, (3000.0, 8000.0)), ("256 scenes of 30", 30, 256, (70.0, 160.0)))
EXPECTED = ("8u.6 measured 49 to 53 ps a pair for the pair function at full occupancy and 8v.6 a floor of about 47 us for a call of one "
            "upload, two kernels and the flag's copy; this call has one upload and four kernels.  The mask kernel evaluates at most n(n+1)/2 "
            "pairs a scene (those whose z intervals overlap; of proposals in a 2 m cube about half do), one wave a 64 x 64 tile: a wave "
            "walks its 64 columns one after the other, about 2,000 cycles of double arithmetic each, so a tile takes about 50 us however few "
            "tiles there are, and the pair rate only shows once the tiles fill the device (3 waves a SIMD, about 3,000 tiles).  The rank kernel "
            "costs n^2 comparisons out of LDS, a few us.  THE SCAN IS THE UNKNOWN: one wave a scene, per block of 64 ranks one strided load "
            "of the diagonal words (1 to 2 us), 64 register steps of two read-lanes and a handful of integer operations (about 1,500 cycles, "
            "under 1 us), then the kept rows of the block (a quarter of the ranks of these proposals, so about 15) ORed into the later words "
            "in groups of eight independent loads (1 to 2 us a group and word slot): 3 to 8 us a block, so 15 us at 256 boxes, 60 us at "
            "1,024, 250 us at 4,096 and 1 to 3 ms at 16,384 (256 blocks, up to four word slots a lane).  256 boxes: floor + a tile's 50 us + "
            "scan: 90 to 200 us.  1,024: 5.2e5 pairs, 136 tiles: 130 to 350 us.  4,096: 8.4e6 pairs, 430 us at the pair rate if all were "
            "evaluated, 2,080 tiles, scan 250 us: 0.5 to 1.2 ms.  16,384: 1.3e8 pairs, 3 to 7 ms, scan 1 to 3 ms: 4 to 11 ms.  1,024 scenes "
            "of 512: the same 1.3e8 pairs in 36,864 tiles, the scans side by side (8 blocks each): 3 to 8 ms.  256 scenes of 30: one tile "
            "of 30 columns a scene, all at once: 70 to 160 us")
# The ranges above were written for the first build of the kernels (the issue's shape: a lane a row and one wave a tile in the mask kernel).  Its
# medians at IoU 0.25, kept so that the file shows what the ranges were first held against; DESIGN.md 8w.6 says what changed after them.
FIRST_BUILD_US = {"256": 453.9, "1,024": 585.1, "4,096": 1333.3, "16,384": 8839.3, "1,024 scenes of 512": 5796.6, "256 scenes of 30": 193.1}
NOT_MEASURED = ["the kernels one by one (events on the caller's stream cannot separate them and the entry has no stage timer by its contract; "
                "a kernel trace would)", "real detector output (fewer, larger clusters than 8 proposals an object)", "more than one wave a long scene in the scan",
                "classes (a class test before the pair function: less work, never more)", "several streams in flight", "the command's file work"]


def proposals(seed, k):
    """tests/boxnms_ref.py's generator: ceil(k/8) objects, 8 jittered copies each, every sixteenth box a copy of its neighbour, shuffled"""
    rng = np.random.RandomState(seed)
    m = (k + 7) // 8
    c, s, yaw = rng.rand(m, 3) * 2.0, 0.2 + 0.6 * rng.rand(m, 3), rng.rand(m) * 2.0 * np.pi
    c, s, yaw = np.repeat(c, 8, 0), np.repeat(s, 8, 0), np.repeat(yaw, 8)
    c = (c + (rng.rand(8 * m, 3) * 2.0 - 1.0) * 0.3 * s).astype(np.float32).astype(np.float64)
    s = s * (0.8 + 0.4 * rng.rand(8 * m, 3))
    yaw = yaw + (rng.rand(8 * m) * 2.0 - 1.0) * 0.15
    rows = np.concatenate([c, s, np.cos(yaw)[:, None], np.sin(yaw)[:, None]], 1)
    rows[15::16] = rows[14::16][:rows[15::16].shape[0]]
    rows = rows[:k][rng.permutation(k)]
    return np.ascontiguousarray(rows), np.round(rng.rand(k), 2)


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
        for name, n, scenes, _ in SHAPES:
            parts = [proposals(1 + s % 16, n) for s in range(min(scenes, 16))]           # sixteen distinct scenes, repeated
            box = np.concatenate([parts[s % 16][0] for s in range(scenes)])
            score = np.concatenate([parts[s % 16][1] for s in range(scenes)])
            k = n * scenes
            off = (np.arange(scenes + 1) * n).astype(np.int32)
            words = scenes * n * ((n + 63) // 64)
            d_box, d_score = torch.from_numpy(box).to(dev), torch.from_numpy(score).to(dev)
            out = torch.empty((3, k), dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(lib.sg_box_nms_ws_bytes(k, scenes, words)), 256), dtype=torch.uint8, device=dev)

            def call(iou):
                hip.check(lib.sg_box_nms(d_box.data_ptr(), d_score.data_ptr(), None, k, off.ctypes.data, scenes, iou, out[0].data_ptr(), out[1].data_ptr(),
                                         out[2].data_ptr(), words, ws.data_ptr(), ws.numel(), stream.cuda_stream))

            row = dict(name=name, boxes=k, scenes=scenes, pairs=scenes * n * (n + 1) // 2, words=words, us={}, kept={})
            for label, iou in (("iou_0.25", IOU), ("iou_0.999", 0.999)):
                call(iou)                                                      # the warm-up
                times = []
                for _ in range(repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call(iou)
                    e1.record(stream)
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                row["us"][label] = spread(times)
                row["kept"][label] = int(out[1].sum().item())
            row["ps_a_pair"] = round(row["us"]["iou_0.25"]["median"] * 1e6 / row["pairs"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_box, d_score, out, ws
    return dict(shapes=rows)


def missed(measured):
    out = []
    for (name, _, _, (lo, hi)), row in zip(SHAPES, measured["shapes"]):
        m = row["us"]["iou_0.25"]["median"]
        if not lo <= m <= hi:
            out.append("%s: %.1f us, %s the expected %.0f to %.0f us" % (name, m, "below" if m < lo else "above", lo, hi))
    return out


def table(doc):
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    lines = ["| shape | boxes | pairs n(n+1)/2 | expected | IoU 0.25 | kept | IoU 0.999 (all kept) | ps a pair |", "|---|---|---|---|---|---|---|---|"]
    for (_, _, _, (lo, hi)), r in zip(SHAPES, doc["measured"]["shapes"]):
        lines.append(f"| {r['name']} | {r['boxes']:,} | {r['pairs']:,} | {lo:,.0f} to {hi:,.0f} | {us(r['us']['iou_0.25'])} | {r['kept']['iou_0.25']:,} | "
                     f"{us(r['us']['iou_0.999'])} | {r['ps_a_pair']:,.1f} |")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxnms_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; torch.cuda.Event pairs around every library call",
               expected=EXPECTED, expected_us={name: list(r) for name, _, _, r in SHAPES}, first_build_us=dict(FIRST_BUILD_US), not_measured=list(NOT_MEASURED),
               measured=None, missed=None)
    write(a.out, doc)                                                          # the expectations are on disk before the first run
    doc["measured"] = measure(a.repeats)
    doc["missed"] = missed(doc["measured"])
    write(a.out, doc)
    print(table(doc))


if __name__ == "__main__":
    main()
