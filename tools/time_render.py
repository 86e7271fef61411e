#!/usr/bin/env python3
"""sg_render measured -> profiles/render_time.json.

    python tools/time_render.py [--repeats 15] [--out profiles/render_time.json]
    python tools/time_render.py --table profiles/render_time.json     # prints the markdown table of DESIGN.md 8y (no GPU needed)

One process, one GPU, one stream.  sg_render has no stage timer, so every library call is bracketed by a pair of torch.cuda.Event on the
call's stream: two warm-up calls, then the median (min .. max) of the repeats.  Shapes: a ScanNet-sized synthetic mesh (tests/render_ref.py's
folded sheet at 548 x 274: 150,152 vertices, 298,662 faces, two layers deep over a third of it), its vertices alone as 3 x 3 splats, and
the same sheet COARSE (64 x 32: 2,048 vertices, 3,906 faces of hundreds of pixels each -- the meshes of `boxes --ply`, of planes, of CAD
models: the only shape here on which the small-primitive threshold decides anything), at 640 x 480 and 1296 x 968 (ScanNet's depth and
colour frames), 1 and 8 orbit views a call.  The meshes are drawn under the small-primitive thresholds 4, 8, 16 and 32
(sg_render_set_tuning), ALTERNATING inside every repeat so that drift of the machine falls on all alike; the images of all of them
must be the same bytes, or the tool fails.  The expected ranges are written into the file BEFORE the first run.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((640, 480), (1296, 968))
VIEWS = (1, 8)
THRESHOLDS = (4, 8, 16, 32)
GRID = (548, 274)
COARSE = (64, 32)
# (primitives, W, views) -> the expected range in us
EXPECTED_US = {("mesh", 640, 1): (60.0, 400.0), ("mesh", 640, 8): (150.0, 1500.0), ("mesh", 1296, 1): (80.0, 600.0), ("mesh", 1296, 8): (300.0, 3000.0),
               ("coarse mesh", 640, 1): (50.0, 300.0), ("coarse mesh", 640, 8): (80.0, 1000.0), ("coarse mesh", 1296, 1): (60.0, 500.0),
               ("coarse mesh", 1296, 8): (200.0, 2500.0),
               ("splats", 640, 1): (50.0, 300.0), ("splats", 640, 8): (100.0, 1000.0), ("splats", 1296, 1): (60.0, 400.0), ("splats", 1296, 8): (250.0, 2500.0)}
EXPECTED = ("nothing was measured before this file.  A call is two clears, one small upload, four launches (three for splats), one 64-byte "
            "copy back and one host wait: 40 to 60 us before any work.  Per view the mesh costs 150,000 projections (16 bytes written each), "
            "300,000 primitive threads that gather three 16-byte records and rasterise a few pixels (at 640 x 480 a face of this mesh covers "
            "about one pixel, at 1296 x 968 about four), and a pixel pass that reads 8 bytes and writes 12: 4 MB at 640 x 480, 15 MB at "
            "1296 x 968, 120 MB for eight views of the latter -- tens of microseconds at the rate HBM streams, so the call is bound by "
            "launches and the host wait at one view and by the primitive threads' gathers and 64-bit atomics at eight.  With faces of one to "
            "four pixels hardly any primitive exceeds even the 8 x 8 threshold, so 8, 16 and 32 should time alike on this mesh; "
            "the queue matters for meshes with few large faces, which ScanNet's are not.  The coarse sheet is such a mesh: a face's box is about 10 x 15 "
            "pixels at 640 x 480 and 20 x 30 at 1296 x 968, so at threshold 8 every face goes to the queue and a workgroup of 256 threads, at "
            "32 nearly every face is walked by ONE thread through up to 1,024 pixels with two double divisions each, the other lanes of its "
            "wave waiting: 8 should win there, by a factor that grows with the image, and the pixel pass, the same for every threshold, bounds the "
            "difference from below.  Threshold 4 should be level with 8 on the coarse sheet (all its faces are queued at 8 already) and behind "
            "on the fine mesh at 1296 x 968, where boxes of 5 x 5 pixels begin to go to the queue and take a workgroup of 256 threads each")
NOT_MEASURED = ["the kernels one by one (events on the caller's stream cannot separate them and the entry has no stage timer)",
                "a real room mesh (deeper in layers, its faces less even in size)", "faces larger than the coarse sheet's (walls of a floor plan across the whole image)",
                "point sizes other than 3", "several streams in flight", "the command's file work, the PNG encoding and sg_render_colour"]


def spread(rows, digits=1):
    a = np.asarray(rows, np.float64)
    return dict(median=round(float(np.median(a)), digits), min=round(float(a.min()), digits), max=round(float(a.max()), digits))


def measure(repeats):
    import torch
    import render_ref as R
    from seggroup_amd import hip
    from seggroup_amd import render as M
    dev = torch.device("cuda:0")
    lib = hip.lib()
    stream = torch.cuda.Stream(device=dev)
    xyz, faces, _ = R.folded_sheet(*GRID)
    coarse_xyz, coarse_faces, _ = R.folded_sheet(*COARSE)
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    rows = []
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        fine = (torch.from_numpy(xyz).to(dev), torch.from_numpy(faces).to(dev))
        coarse = (torch.from_numpy(coarse_xyz).to(dev), torch.from_numpy(coarse_faces).to(dev))
        d_hits = torch.empty(xyz.shape[0], dtype=torch.int32, device=dev)
        for W, H in SIZES:
            for B in VIEWS:
                cams = M.camera_rows(M.orbit_views(lo, hi, (W, H), B, 35.0))
                d_prim, d_vert = (torch.empty((B, H, W), dtype=torch.int32, device=dev) for _ in range(2))
                d_depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
                for prims, d_xyz, d_f, settings in (("mesh", fine[0], fine[1], THRESHOLDS), ("coarse mesh", coarse[0], coarse[1], THRESHOLDS),
                                                    ("splats", fine[0], None, (0,))):
                    V, nf = int(d_xyz.shape[0]), 0 if d_f is None else int(d_f.shape[0])
                    ws = torch.empty(max(int(lib.sg_render_ws_bytes(V, nf, B, W, H)), 256), dtype=torch.uint8, device=dev)

                    def call(small):
                        hip.check(lib.sg_render_set_tuning(small))
                        hip.check(lib.sg_render(d_xyz.data_ptr(), 3, V, hip.ptr(d_f), nf, 3, B, cams.ctypes.data, 0, 0.05, W, H, d_prim.data_ptr(),
                                                d_depth.data_ptr(), d_vert.data_ptr(), d_hits.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))

                    times = {s: [] for s in settings}
                    digest, stats = {}, {}
                    h = (C.c_int64 * 6)()
                    try:
                        for s in settings:
                            call(s), call(s)                                   # the warm-up
                            digest[s] = hashlib.sha1(b"".join(t.cpu().numpy().tobytes() for t in (d_prim, d_depth, d_vert, d_hits[:V]))).hexdigest()
                            hip.check(lib.sg_render_stats(h, 6))
                            stats[s] = dict(zip(M.STAT_NAMES, (int(x) for x in h)))
                        for _ in range(repeats):
                            for s in settings:                                  # alternating: drift falls on every setting alike
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record(stream)
                                call(s)
                                e1.record(stream)
                                e1.synchronize()
                                times[s].append(e0.elapsed_time(e1) * 1e3)
                    finally:
                        hip.check(lib.sg_render_set_tuning(0))
                    if len(set(digest.values())) != 1:
                        raise RuntimeError("the thresholds disagree on %s %d x %d x %d: %r" % (prims, W, H, B, digest))
                    for s in settings:
                        row = dict(primitives=prims, vertices=V, faces=nf, width=W, height=H, views=B, threshold=s or None, us=spread(times[s]),
                                   digest=digest[s][:16], **stats[s])
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                    del ws
                del d_prim, d_vert, d_depth
    return rows


def missed(rows):
    out = []
    for r in rows:
        lo, hi = EXPECTED_US[r["primitives"], r["width"], r["views"]]
        m = r["us"]["median"]
        if not lo <= m <= hi:
            out.append("%s %d x %d x %d, threshold %s: %.1f us, %s the expected %.0f to %.0f us" % (
                r["primitives"], r["width"], r["height"], r["views"], r["threshold"], m, "below" if m < lo else "above", lo, hi))
    return out


def table(doc):
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    lines = ["| primitives | image | views | threshold | expected µs | µs | kept | large | covered pixels |", "|---|---|---|---|---|---|---|---|---|"]
    for r in doc["measured"]:
        lo, hi = EXPECTED_US[r["primitives"], r["width"], r["views"]]
        lines.append(f"| {r['primitives']} | {r['width']} x {r['height']} | {r['views']} | {r['threshold'] or '-'} | {lo:,.0f} to {hi:,.0f} | {us(r['us'])} | "
                     f"{r['kept']:,} | {r['large']:,} | {r['covered']:,} |")
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
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; torch.cuda.Event pairs around every library call; the "
               "thresholds alternate inside every repeat", expected=EXPECTED, expected_us={"%s %d x%d" % k: list(v) for k, v in EXPECTED_US.items()},
               not_measured=list(NOT_MEASURED), measured=None, missed=None)
    write(a.out, doc)                                                          # the expectations are on disk before the first run
    doc["measured"] = measure(a.repeats)
    doc["missed"] = missed(doc["measured"])
    write(a.out, doc)
    print(table(doc))


if __name__ == "__main__":
    main()
