#!/usr/bin/env python3
"""Plane extraction, measured stage by stage -> profiles/planes_time.json.

    python tools/time_planes.py [--repeats 5] [--dist 0.01] [--min-points 1000] [--out profiles/planes_time.json]
    python tools/time_planes.py --table profiles/planes_time.json      # prints the markdown table of DESIGN.md 8s (no GPU needed)

One process, one GPU, one stream.  The cloud is make_room_scan(400, 375) (150,000 points on a 0.04 lattice with a jitter of 5e-4), every
point free.  At H = 1,024 / 4,096 / 16,384 the stages of sg_plane_ransac (compact, generate, count), of sg_plane_moments and of
sg_plane_assign on the winning plane are timed by the library's own events on the stream (hip.stage_timer("plane")), the median (min .. max)
of the repeats after a warm-up; the count also with the kept hypotheses NOT compacted.  The whole of detect_planes by the host's clock and
the planes it finds stand beside them.  EXPECTED was written down before the first run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HYPOTHESES = (1 << 10, 1 << 12, 1 << 14)
EXPECTED = ("the count is H x M point-plane tests of about eight double operations (three multiplies, three adds, the absolute value's compare, "
            "the counter) and nothing contracts, so at H = 4,096 and M = 150,000 it is 5e9 operations: 125 us if every fp64 lane of the device "
            "were busy, and with the LDS reads, the widening of a tile and 16 waves a CU in flight 200 to 400 us, in proportion to H above "
            "that and 60 to 100 us at 1,024, where the segments over the free list have to fill the device; the issue's own guess was tens "
            "of microseconds.  Compaction (five small launches over 150,000 points) 20 to 40 us, generation under 10 us, the moments and the "
            "labelling 10 to 20 us each, launch and copy included; not compacting the kept hypotheses costs the rejected share, about a "
            "tenth.  detect_planes by the host's clock: a few milliseconds a round -- five synchronising calls, a clone and the uploads of "
            "the Python layer -- so the Python layer, not a kernel, dominates")
NOT_MEASURED = ["real scans", "normals in the inlier test (the tile is twice as large: 3 workgroups a CU instead of 6)", "several streams in flight",
                "clouds near the 2^24-point limit", "a cloud most of whose points are already labelled", "the command (PLY read and write)"]


def spread(rows):
    a = np.asarray(rows, np.float64)
    return [dict(median=round(float(np.median(a[:, i])), 1), min=round(float(a[:, i].min()), 1), max=round(float(a[:, i].max()), 1))
            for i in range(a.shape[1])]


def measure(dist, min_points, repeats):
    import torch
    from seggroup_amd import hip, planes, synthetic
    dev = "cuda:0"
    lib = hip.lib()
    room = np.ascontiguousarray(synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz, dtype=np.float32)
    d_xyz = torch.from_numpy(room).to(dev)
    n = int(room.shape[0])
    origin = 0.5 * (room.min(0).astype(np.float64) + room.max(0).astype(np.float64))
    out = dict(points=n, dist=dist, min_points=min_points, min_edge=10.0 * dist, stages=None, rounds=[], whole_call=[])
    free = torch.full((n,), -1, dtype=torch.int32, device=dev)
    for h in HYPOTHESES:
        row = dict(hypotheses=h)
        state = {}

        def one_round():
            state["count"], state["plane"], _, state["best"] = planes.plane_ransac(d_xyz, dist, h, 0, free, device=dev)
            pl = state["plane"][state["best"]].cpu().numpy()
            planes.plane_moments(d_xyz, pl, dist, origin, free, device=dev)
            state["labelled"] = planes.plane_assign(d_xyz, free.clone(), pl, dist, 0, device=dev)[1]

        for compact in (1, 0):
            try:
                hip.check(lib.sg_plane_set_tuning(compact))
                with hip.stage_timer("plane") as t:
                    one_round()                                           # the warm-up
                    rows = []
                    for _ in range(repeats):
                        one_round()
                        rows.append(t.read())
            finally:
                hip.check(lib.sg_plane_set_tuning(1))
            out["stages"] = t.names
            row["stages_us" if compact else "stages_us_not_compacted"] = dict(zip(t.names, spread(rows)))
            state["bytes_%d" % compact] = state["count"].cpu().numpy().tobytes()
        assert state["bytes_1"] == state["bytes_0"]
        kept = int((state["count"] >= 0).sum())
        row.update(kept=kept, kept_fraction=round(kept / float(h), 4), best_count=int(state["count"].max()), labelled=int(state["labelled"]))
        out["rounds"].append(row)
        print(json.dumps(row), flush=True)
    for h in HYPOTHESES:
        planes.detect_planes(d_xyz, dist, min_points=min_points, hypotheses=h, device=dev)
        torch.cuda.synchronize()
        wall = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            found = planes.detect_planes(d_xyz, dist, min_points=min_points, hypotheses=h, device=dev)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out["whole_call"].append(dict(hypotheses=h, wall_ms=dict(median=round(float(np.median(wall)), 2), min=round(min(wall), 2), max=round(max(wall), 2)),
                                      planes=int(found.planes.shape[0]), points=found.points.tolist(), unlabelled=int((found.labels < 0).sum()),
                                      rms=[round(float(r), 6) for r in found.rms]))
        print(json.dumps(out["whole_call"][-1]), flush=True)
    return out


def table(doc):
    m = doc["measured"]
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    lines = [f"| {m['points']:,} points, dist {m['dist']:g}, min_edge {m['min_edge']:g} | µs between events: median (min .. max) |", "|---|---|"]
    for r in m["rounds"]:
        s, s0 = r["stages_us"], r["stages_us_not_compacted"]
        lines.append(f"| H = {r['hypotheses']:,}: compact; generate; count; count without compacting the kept; kept (share) | {us(s['compact'])}; "
                     f"{us(s['generate'])}; {us(s['count'])}; {us(s0['count'])}; {r['kept']:,} ({100 * r['kept_fraction']:.1f} %) |")
        lines.append(f"| H = {r['hypotheses']:,}: moments; assign ({r['labelled']:,} points labelled) | {us(s['moments'])}; {us(s['assign'])} |")
    for w in m["whole_call"]:
        lines.append(f"| `detect_planes`, H = {w['hypotheses']:,}: host clock, ms; planes found (points) | {w['wall_ms']['median']:,} ({w['wall_ms']['min']:,} .. "
                     f"{w['wall_ms']['max']:,}); {w['planes']} ({', '.join(str(p) for p in w['points'])}; {w['unlabelled']:,} unlabelled) |")
    lines += ["", "Expected before the run: " + doc["expected"] + ".", "", "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dist", type=float, default=0.01)
    ap.add_argument("--min-points", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream", expected=EXPECTED, not_measured=list(NOT_MEASURED),
               measured=measure(a.dist, a.min_points, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
