#!/usr/bin/env python3
"""sg_lift and sg_lift_vote measured -> profiles/lift_time.json.

    python tools/time_lift.py [--repeats 15] [--out profiles/lift_time.json]
    python tools/time_lift.py --table profiles/lift_time.json     # prints the markdown table of DESIGN.md 8z (no GPU needed)

One process, one GPU, one stream.  Neither entry has a stage timer, so every library call is bracketed by a pair of torch.cuda.Event on the
call's stream: two warm-up calls, then the median (min .. max) of the repeats, sg_lift and sg_lift_vote separately.  The scan is a
ScanNet-sized synthetic mesh (tests/render_ref.py's folded sheet at 548 x 274: 150,152 vertices), the images 640 x 480 (ScanNet's depth
frames), 1, 8 and 64 orbit views a call, 41 classes (NYU40 and none) and 400 (instances).  The label images are the scan's own, rendered:
every vertex carries a random class, a pixel the class of the vertex it sees; the depth images are sg_render's.  Beside the plain call
(the depth images given) stands the self-occluding path, sg_render followed by sg_lift, and beside both the same work in NumPy: the
restatement tests/lift_ref.py (accumulate, then vote), wall time on the host, the only comparison there is -- the tree had no way from
images to vertices before.  Nothing gates on a time.  The expected ranges are written into the file BEFORE the first run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = (640, 480)
VIEWS = (1, 8, 64)
CLASSES = (41, 400)
GRID = (548, 274)
TOL = 0.02
# views -> the expected range of sg_lift in us
EXPECTED_US = {1: (30.0, 200.0), 8: (40.0, 400.0), 64: (150.0, 2500.0)}
EXPECTED = ("nothing was measured before this file.  sg_lift is one clear of 64 bytes, one small upload, ONE launch, one 64-byte copy back and one "
            "host wait: 30 to 50 us before any work.  A (view, vertex) pair reads 12 bytes of coordinates (coalesced), does about 20 double "
            "operations with two divisions, gathers 4 bytes of depth and 4 of label from a pixel that its neighbours in the wave mostly do not "
            "share, and adds to two scattered words: 150,152 pairs a view, so 9.6 million at 64 views -- at a few hundred bytes of transactions "
            "a pair a few GB, a millisecond or so at the rate scattered 64-byte accesses go, and the double divisions (a quarter-rate pipe, "
            "some 40 cycles each) amount to less.  So the pair kernel should be bound by its gathers and scattered atomics, not by the "
            "arithmetic: a SUPPOSITION, which these figures can support (time per pair, against what the arithmetic alone would cost) and not "
            "prove.  The vote reads V * C counts once, coalesced: 25 MB at 41 classes, 240 MB at 400 -- 10 to 20 us and 60 to 120 us.  The "
            "NumPy restatement should take around a second for eight views")
NOT_MEASURED = ["real ScanNet frames (a sensor's depth, holes and noise: more NODEPTH and OCCLUDED pairs, which end early)", "classes in the thousands",
                "several streams in flight", "the command's file work (PNG decoding, the .npz, the label files)", "hardware counters of the pair kernel"]


def spread(rows, digits=1):
    a = np.asarray(rows, np.float64)
    return dict(median=round(float(np.median(a)), digits), min=round(float(a.min()), digits), max=round(float(a.max()), digits))


def measure(repeats, numpy_views):
    import torch
    import lift_ref as L
    import render_ref as R
    from seggroup_amd import hip
    from seggroup_amd import lift as M
    from seggroup_amd import render
    dev = torch.device("cuda:0")
    lib = hip.lib()
    stream = torch.cuda.Stream(device=dev)
    xyz, faces, _ = R.folded_sheet(*GRID)
    V, F = int(xyz.shape[0]), int(faces.shape[0])
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    W, H = SIZE
    rng = np.random.RandomState(0)
    rows = []

    def timed(fn):
        fn(), fn()                                                               # the warm-up
        out = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return spread(out)

    with torch.cuda.device(dev), torch.cuda.stream(stream):
        d_xyz, d_faces = torch.from_numpy(xyz).to(dev), torch.from_numpy(faces).to(dev)
        for B in VIEWS:
            cams = render.camera_rows(render.orbit_views(lo, hi, SIZE, B, 35.0))
            d_prim, d_vert = (torch.empty((B, H, W), dtype=torch.int32, device=dev) for _ in range(2))
            d_depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
            rws = torch.empty(max(int(lib.sg_render_ws_bytes(V, F, B, W, H)), 256), dtype=torch.uint8, device=dev)
            lws = M.workspace(lib.sg_lift_ws_bytes(V, B), dev)

            def draw():
                hip.check(lib.sg_render(d_xyz.data_ptr(), 3, V, d_faces.data_ptr(), F, 3, B, cams.ctypes.data, 0, 0.05, W, H, d_prim.data_ptr(),
                                        d_depth.data_ptr(), d_vert.data_ptr(), None, rws.data_ptr(), rws.numel(), stream.cuda_stream))

            draw()
            for K in CLASSES:
                own = torch.from_numpy(rng.randint(0, K, V).astype(np.int32)).to(dev)
                d_label = torch.where(d_vert >= 0, own[d_vert.clamp(min=0).long()], torch.full_like(d_vert, -1)).contiguous()
                d_counts = torch.zeros((V, K), dtype=torch.int32, device=dev)
                d_seen = torch.zeros(V, dtype=torch.int32, device=dev)
                out = [torch.empty(V, dtype=torch.int32, device=dev) for _ in range(4)]

                def lift():
                    hip.check_arg(lib.sg_lift(d_xyz.data_ptr(), 3, V, B, cams.ctypes.data, 0, 0.05, W, H, d_label.data_ptr(), d_depth.data_ptr(), TOL, K,
                                              d_counts.data_ptr(), d_seen.data_ptr(), lws.data_ptr(), lws.numel(), stream.cuda_stream))

                def vote():
                    hip.check(lib.sg_lift_vote(d_counts.data_ptr(), V, K, *(t.data_ptr() for t in out), stream.cuda_stream))

                row = dict(vertices=V, width=W, height=H, views=B, classes=K, lift_us=timed(lift), vote_us=timed(vote),
                           render_and_lift_us=timed(lambda: (draw(), lift())))
                row.update(M.call_stats())
                row["ns_per_pair"] = round(row["lift_us"]["median"] * 1e3 / (B * V), 3)
                if B in numpy_views:
                    labels, depth = d_label.cpu().numpy(), d_depth.cpu().numpy()
                    t0 = time.perf_counter()
                    counts, seen, stats, _ = L.accumulate(xyz, cams, labels, depth, TOL, K, False, 0.05)
                    t1 = time.perf_counter()
                    ref = L.vote(counts)
                    t2 = time.perf_counter()
                    row["numpy_accumulate_ms"], row["numpy_vote_ms"] = round((t1 - t0) * 1e3, 1), round((t2 - t1) * 1e3, 1)
                    d_counts.zero_(), d_seen.zero_()
                    lift(), vote()
                    stream.synchronize()
                    same = np.array_equal(d_counts.cpu().numpy(), counts) and np.array_equal(d_seen.cpu().numpy(), seen) and M.call_stats() == stats and \
                        all(np.array_equal(t.cpu().numpy(), r) for t, r in zip(out, ref))
                    if not same:
                        raise RuntimeError("the library and the restatement disagree at %d views, %d classes" % (B, K))
                    row["equal_to_numpy"] = True
                rows.append(row)
                print(json.dumps(row), flush=True)
                del d_counts, d_label
            del d_prim, d_vert, d_depth, rws
    return rows


def missed(rows):
    out = []
    for r in rows:
        lo, hi = EXPECTED_US[r["views"]]
        m = r["lift_us"]["median"]
        if not lo <= m <= hi:
            out.append("%d views, %d classes: sg_lift %.1f us, %s the expected %.0f to %.0f us" % (r["views"], r["classes"], m, "below" if m < lo else "above", lo, hi))
    return out


def table(doc):
    us = lambda d: f"{d['median']:,.1f} ({d['min']:,.1f} .. {d['max']:,.1f})"     # noqa: E731
    lines = ["| views | classes | expected µs | sg_lift µs | ns a pair | sg_lift_vote µs | sg_render + sg_lift µs | NumPy accumulate ms | NumPy vote ms | labelled pairs |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["measured"]:
        lo, hi = EXPECTED_US[r["views"]]
        lines.append(f"| {r['views']} | {r['classes']} | {lo:,.0f} to {hi:,.0f} | {us(r['lift_us'])} | {r['ns_per_pair']} | {us(r['vote_us'])} | "
                     f"{us(r['render_and_lift_us'])} | {r.get('numpy_accumulate_ms', '-')} | {r.get('numpy_vote_ms', '-')} | {r['labelled']:,} |")
    lines += ["", "µs between events: median (min .. max); the NumPy columns are wall time on the host, once.", "", "Expected before the run: " + doc["expected"] + ".", "",
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
    ap.add_argument("--numpy-views", type=int, nargs="*", default=list(VIEWS), help="the view counts at which the NumPy restatement is timed and compared")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; torch.cuda.Event pairs around every library call; the NumPy "
               "restatement once per shape, wall time", expected=EXPECTED, expected_us={str(k): list(v) for k, v in EXPECTED_US.items()},
               not_measured=list(NOT_MEASURED), measured=None, missed=None)
    write(a.out, doc)                                                          # the expectations are on disk before the first run
    doc["measured"] = measure(a.repeats, set(a.numpy_views))
    doc["missed"] = missed(doc["measured"])
    write(a.out, doc)
    print(table(doc))


if __name__ == "__main__":
    main()
