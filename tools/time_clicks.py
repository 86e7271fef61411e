#!/usr/bin/env python3
"""Simulated clicks, measured -> profiles/clicks_time.json.

    python tools/time_clicks.py [--sizes 400x375:10,400x400:2] [--iters 20] [--label-iters 3] [--out profiles/clicks_time.json]

Per synthetic scan (a W x H lattice of make_raw_scan in CELL x CELL segments with synthetic annotations: 150,000 vertices / 1,520
segments, and 160,000 vertices / 40,000 segments, where the dense [S,S] matrix is 12.8 GB of mostly untouched pages) every stage of
sg_segment_graph on the scan's adj.pth by HIP events (sg_segment_graph_set_timing; three warm-up calls, the median of `iters` calls),
the host fold sg_click_clusters, and the wall time of `labels.generate_weak_labels(label_style="maxseg")` with seg_graph="dense" -- the
code of the parent commit, unchanged -- and seg_graph="scan", in this one process (the median of `label-iters` calls each).  Both must
click the same segments.  The figures are recorded, not gated: nothing depends on them.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def available_bytes():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def time_graph(adj, seg, S, iters):
    import torch
    from seggroup_amd import hip, seggraph
    lib = hip.lib()
    d_adj, d_seg = adj.cuda().contiguous(), torch.from_numpy(seg.astype(np.int32)).cuda()
    e, v = int(d_adj.shape[0]), int(d_seg.shape[0])
    d_pairs = torch.empty((e, 2), dtype=torch.int32, device="cuda")
    d_cross = torch.empty(e, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sg_segment_graph_ws_bytes(e, S), dtype=torch.uint8, device="cuda")
    n_p = C.c_longlong(0)

    def call():
        hip.check(lib.sg_segment_graph(d_adj.data_ptr(), e, d_seg.data_ptr(), v, S, d_pairs.data_ptr(), d_cross.data_ptr(), C.byref(n_p),
                                       ws.data_ptr(), ws.numel(), None))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    rows, wall = [], []
    with hip.stage_timer("segment_graph") as timer:
        for _ in range(iters):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            rows.append(timer.read())
    us = np.median(np.asarray(rows), 0)
    pairs, cross = d_pairs[:n_p.value].cpu().numpy(), d_cross[:n_p.value].cpu().numpy()
    return pairs, dict(E=e, crossing_rows=int(cross.sum()), pairs=int(n_p.value), key_bits=2 * max(S - 1, 0).bit_length(),
                       stages_us={n: round(float(u), 1) for n, u in zip(timer.names, us)}, event_sum_us=round(float(us.sum()), 1),
                       host_wall_us=round(float(np.median(wall)) * 1e6, 1))


def measure(w, h, cell, iters, label_iters, td):
    import torch
    import capture_labels as cl
    from seggroup_amd import labels, prepare, seggraph, synthetic
    name = "scene%04d_00" % cell
    scan = synthetic.make_raw_scan(w, h, 11, name=name, cell=cell, dup_frac=0.0, degenerate_faces=0)
    ann = synthetic.make_annotations(scan, 3, blocks_per_row=-(-w // cell))
    scene_path = cl.write_inputs(td, scan, ann)
    prepare.write_ply(os.path.join(scene_path, name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
    v = scan.xyz.shape[0]
    prepare.prepare_scene(scene_path, 0, v, root=td, perm=scan.perm)
    labels.generate_real_labels(scene_path, root=td)
    raw = os.path.join(td, "label", "real", "raw", name)
    seg = np.array(labels.load_labels(os.path.join(raw, name + ".seg.txt")))
    ins = np.array(labels.load_labels(os.path.join(raw, name + ".ins.txt")))
    S = int(seg.max()) + 1
    adj = torch.load(os.path.join(td, "adj", "mesh", "raw", name, name + ".adj.pth"))
    pairs, graph = time_graph(adj, seg, S, iters)
    _, seg_ins, _ = labels.segment_table(seg, ins, on_device=False)
    fold = []
    for _ in range(max(label_iters, 3)):
        t0 = time.perf_counter()
        off, _, _ = seggraph.click_clusters(pairs, seg_ins, S)
        fold.append(time.perf_counter() - t0)
    out = dict(lattice=f"{w}x{h}", cell=cell, V=int(v), segments=S, instances=int(np.unique(ins[ins > 0]).shape[0]), clusters=int(off.shape[0] - 1),
               dense_matrix_bytes=8 * S * S, sg_segment_graph=graph, sg_click_clusters_host_us=round(float(np.median(fold)) * 1e6, 1))
    rets = {}
    for which in ("scan", "dense"):
        wall = []
        if which == "dense" and available_bytes() < 2 * 8 * S * S:
            out["generate_weak_labels_dense_wall_ms"] = None
            out["dense_note"] = "not measured: the matrix does not fit this host's free memory"
            continue
        try:
            for _ in range(label_iters):
                t0 = time.perf_counter()
                rets[which] = labels.generate_weak_labels(scene_path, None, label_style="maxseg", root=td, seg_graph=which)
                wall.append(time.perf_counter() - t0)
            out[f"generate_weak_labels_{which}_wall_ms"] = round(float(np.median(wall)) * 1e3, 1)
        except MemoryError:
            out[f"generate_weak_labels_{which}_wall_ms"] = None
            out[f"{which}_note"] = "the matrix did not fit this host"
    if len(rets) == 2:
        assert rets["scan"] == rets["dense"], (rets["scan"], rets["dense"])
    out["returned"] = list(rets["scan"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="400x375:10,400x400:2", help="WxH:CELL lattices of make_raw_scan: 1,520 and 40,000 segments")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--label-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clicks_time.json"))
    a = ap.parse_args()
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, label_iters=a.label_iters, warm_up_calls=3, label_style="maxseg", scans=[])
    for size in a.sizes.split(","):
        wh, cell = size.split(":")
        w, h = (int(x) for x in wh.split("x"))
        with tempfile.TemporaryDirectory(prefix="sgclicks_") as td:
            doc["scans"].append(measure(w, h, int(cell), a.iters, a.label_iters, td))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                               # after every scan: a run cut short leaves what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["scans"][-1]), flush=True)


if __name__ == "__main__":
    main()
