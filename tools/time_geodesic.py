#!/usr/bin/env python3
"""Geodesic distances over a graph, measured -> profiles/geodesic_time.json.

    python tools/time_geodesic.py [--repeats 5] [--out profiles/geodesic_time.json]
    python tools/time_geodesic.py --table profiles/geodesic_time.json     # prints the markdown table of DESIGN.md 8x (no GPU needed)

One process, one GPU, one stream.  sg_graph_geodesic has no stage timer, so every library call is bracketed by a pair of
torch.cuda.Event on the call's stream (8u.6's method): a warm-up, then the median (min .. max) of the repeats.  Shapes: triangulated
jittered sheets (tests/geodesic_ref.py's generator: float32 coordinates, the three sides of every face as rows, so every inner edge is
there twice) of 150,000 and 1,000,000 vertices with 30 and 300 random seeds, by length, and the 150,000 sheet in a shuffled vertex
order -- the case tiles do not help.  Recorded per shape: us, the two launch counts, the arcs and the tight arcs.

The yardstick for "the inner sweeps pay" is the same build with ONE sweep a launch and ONE launch a host wait, reached through
SG_GEODESIC_SCHEDULE=1,1 (S inner sweeps at most, R launches a host wait), which the library reads once: those rows come from a child
process of this tool (--rows-only) and sit beside the others as `plain`; --schedules S,R ... measures further ones the same way
(`schedules` in the file).  The expected ranges are written into the file BEFORE the first run; afterwards the file says which missed.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name, grid, seeds, shuffled, the expected range in us
SHAPES = (("150,000 / 30 seeds", (387, 388), 30, False, (3000.0, 15000.0)), ("150,000 / 300 seeds", (387, 388), 300, False, (1500.0, 6000.0)),
          ("1,000,000 / 30 seeds", (1000, 1000), 30, False, (40000.0, 130000.0)), ("1,000,000 / 300 seeds", (1000, 1000), 300, False, (15000.0, 50000.0)),
          ("150,000 shuffled / 30 seeds", (387, 388), 30, True, (5000.0, 25000.0)))
EXPECTED = ("nothing was measured before this file.  A sheet of V vertices has 6 V rows (three sides a face, two faces a cell), so 12 V arcs; a "
            "launch of the relaxation reads per arc its target (4 bytes), its weight (8) and the neighbour's value (8, a gather), about 240 bytes "
            "a vertex: 36 MB at 150,000 vertices, 15 to 30 us at the rate gathers reach, 240 MB and 100 to 150 us at a million.  Beside it a "
            "kernel boundary (about 1.5 us) and, once in eight launches, a host wait (30 to 50 us).  So the call is bound by the NUMBER OF "
            "LAUNCHES, which is the hop depth of the seeds' cells -- with 30 seeds on 150,000 vertices a cell has a radius of about 40 hops "
            "and the worst vertex is 80 to 100 from its seed, with 300 seeds a third of that, on a million vertices 2.6 times that -- times "
            "up to 1.5 for lengths (a longer walk of more hops replaces a shorter one), divided by what the inner sweeps and fresh reads of "
            "other tiles buy (unknown: a tile of 256 consecutive vertices is a piece of one grid line, so the sweeps carry a value ALONG the "
            "line only).  The owner phase walks the tight arcs to the same depth.  150,000 / 30: 100 to 350 launches in all at 25 to 40 us, "
            "and 0.3 ms for the sort and the rows: 3 to 15 ms; / 300: 1.5 to 6 ms.  1,000,000 / 30: 300 to 900 launches at 110 to 150 us: 40 to "
            "130 ms; / 300: 15 to 50 ms.  Shuffled: no neighbour is in the tile, every read is a scattered 8-byte gather (40 to 60 us a launch) "
            "and the inner sweeps buy nothing: 5 to 25 ms.  The plain schedule (one sweep a launch, a host wait a launch) pays a wait of 20 to "
            "30 us a launch and needs every hop as a launch of its own: 1.5 to 3 times the time is the guess")
NOT_MEASURED = ["the kernels one by one (events on the caller's stream cannot separate them and the entry has no stage timer by its contract)",
                "a real room mesh (its vertex order is local but not a grid's)", "hops and explicit weights (the same kernels, less to read)",
                "other values of the inner-sweep cap, the batch, the tile and the long-row threshold than the build's and the plain schedule",
                "several streams in flight", "the command's file work"]


def sheet(grid, seeds, shuffled, seed=1):
    import geodesic_ref as R
    xyz, faces = R.grid_mesh(grid[0], grid[1], seed)
    V = xyz.shape[0]
    rng = np.random.RandomState(seed + 7)
    if shuffled:
        perm = rng.permutation(V)                                            # old vertex v becomes perm[v]
        moved = np.empty_like(xyz)
        moved[perm] = xyz
        xyz, faces = moved, perm[faces].astype(np.int32)
    s = np.full(V, -1, np.int32)
    s[rng.choice(V, seeds, replace=False)] = 1
    return xyz, R.face_sides(faces), s


def spread(rows, digits=1):
    a = np.asarray(rows, np.float64)
    return dict(median=round(float(np.median(a)), digits), min=round(float(a.min()), digits), max=round(float(a.max()), digits))


def measure(repeats):
    import ctypes as C

    import torch
    from seggroup_amd import hip
    dev = torch.device("cuda:0")
    lib = hip.lib()
    stream = torch.cuda.Stream(device=dev)
    rows = []
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for name, grid, seeds, shuffled, _ in SHAPES:
            xyz, edges, s = sheet(grid, seeds, shuffled)
            V, E = int(xyz.shape[0]), int(edges.shape[0])
            d_xyz, d_e, d_s = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz, edges, s))      # row-major: the library reads rows
            d_dist, d_owner = torch.empty(V, dtype=torch.float64, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(lib.sg_graph_geodesic_ws_bytes(V, E)), 256), dtype=torch.uint8, device=dev)

            def call():
                hip.check(lib.sg_graph_geodesic(d_e.data_ptr(), E, V, d_xyz.data_ptr(), 3, None, d_s.data_ptr(), float("inf"), d_dist.data_ptr(),
                                                d_owner.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))

            call()                                                             # the warm-up
            times, launches = [], []
            h = (C.c_int64 * 5)()
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
                hip.check(lib.sg_graph_geodesic_stats(h, 5))
                launches.append((int(h[1]), int(h[2])))
            row = dict(name=name, vertices=V, rows=E, arcs=int(h[0]), tight_arcs=int(h[3]), reached=int(h[4]), us=spread(times),
                       distance_launches=sorted(set(l[0] for l in launches)), owner_launches=sorted(set(l[1] for l in launches)),
                       largest_distance=float(d_dist[torch.isfinite(d_dist)].max().item()), owner_sum=int(d_owner.long().sum().item()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_xyz, d_e, d_s, d_dist, d_owner, ws
    return rows


def schedule_rows(schedule, repeats):
    """the same shapes under SG_GEODESIC_SCHEDULE=<schedule>, in a child process: the library reads the switch once"""
    env = dict(os.environ, SG_GEODESIC_SCHEDULE=schedule)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-only", "--repeats", str(repeats)], capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError("the child of schedule %s failed:\n" % schedule + (r.stdout + r.stderr)[-3000:])
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def missed(measured):
    out = []
    for (name, _, _, _, (lo, hi)), row in zip(SHAPES, measured["shapes"]):
        m = row["us"]["median"]
        if not lo <= m <= hi:
            out.append("%s: %.1f us, %s the expected %.0f to %.0f us" % (name, m, "below" if m < lo else "above", lo, hi))
    return out


def table(doc):
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    ln = lambda v: "/".join(str(x) for x in v)                                  # noqa: E731
    lines = ["| shape | vertices | arcs | tight arcs | expected µs | µs | launches (distance, owner) | plain µs | plain launches | plain / build |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for (_, _, _, _, (lo, hi)), r, q in zip(SHAPES, doc["measured"]["shapes"], doc["measured"]["plain"]):
        lines.append(f"| {r['name']} | {r['vertices']:,} | {r['arcs']:,} | {r['tight_arcs']:,} | {lo:,.0f} to {hi:,.0f} | {us(r['us'])} | "
                     f"{ln(r['distance_launches'])}, {ln(r['owner_launches'])} | {us(q['us'])} | {ln(q['distance_launches'])}, {ln(q['owner_launches'])} | "
                     f"{q['us']['median'] / r['us']['median']:.2f} |")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    ap.add_argument("--schedules", nargs="*", default=[], metavar="S,R", help="further schedules to measure beside the build's and the plain one")
    ap.add_argument("--rows-only", action="store_true", help="(the tool's own child) measure and print the rows, write no file")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    if a.rows_only:
        measure(a.repeats)
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; torch.cuda.Event pairs around every library call; the plain "
               "schedule (SG_GEODESIC_SCHEDULE=1,1: one sweep a launch, one launch a host wait) and any further one in child processes",
               expected=EXPECTED, expected_us={name: list(r) for name, _, _, _, r in SHAPES}, not_measured=list(NOT_MEASURED), measured=None, missed=None)
    write(a.out, doc)                                                          # the expectations are on disk before the first run
    shapes = measure(a.repeats)
    others = {sch: schedule_rows(sch, a.repeats) for sch in ["1,1"] + [x for x in a.schedules if x != "1,1"]}
    for sch, rows in others.items():
        for r, q in zip(shapes, rows):
            if (r["largest_distance"], r["owner_sum"], r["tight_arcs"]) != (q["largest_distance"], q["owner_sum"], q["tight_arcs"]):
                raise RuntimeError("schedule %s disagrees with the build's on %s" % (sch, r["name"]))
    doc["measured"] = dict(shapes=shapes, plain=others.pop("1,1"), schedules=others)
    doc["missed"] = missed(doc["measured"])
    write(a.out, doc)
    print(table(doc))


if __name__ == "__main__":
    main()
