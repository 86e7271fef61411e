#!/usr/bin/env python3
"""Point-cloud over-segmentation, measured -> profiles/pcseg_time.json, and the DESIGN table generated from that file.

    python tools/time_pcseg.py [--sizes 400x375,800x625] [--knn 10] [--iters 3] [--out profiles/pcseg_time.json]
    python tools/time_pcseg.py --table profiles/pcseg_time.json        # prints the markdown table of DESIGN.md 8f (no GPU needed)

Per cloud size, all taken in one run: every device stage of sg_pcseg_edges by HIP events (sg_pcseg_set_timing) with its share of the
call -- the brute-force kNN is N^2 pair scores and is expected to dominate -- the host chain (sg_overseg_merge) in ms, the whole call
(segment_pointcloud: upload, device stages, copy back, chain), and the mesh path's row of profiles/overseg_time.json at the same number
of vertices for comparison.  The clouds are the vertices of tools/time_overseg.py's lattices, without their faces.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(w, h, k, iters):
    import torch
    from seggroup_amd import hip, oversegment, synthetic
    lib = hip.lib()
    scan = synthetic.make_room_scan(w, h, 11, jitter=5e-4, name="scene0000_00")
    N = scan.xyz.shape[0]
    d_xyz = torch.from_numpy(scan.xyz).cuda()
    nrm = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    edges = torch.empty((N * k, 2), dtype=torch.int32, device="cuda")
    wts = torch.empty(N * k, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.sg_pcseg_ws_bytes(N, k), dtype=torch.uint8, device="cuda")
    n_e = C.c_int(0)

    def device_call():
        hip.check(lib.sg_pcseg_edges(d_xyz.data_ptr(), N, k, None, None, nrm.data_ptr(), edges.data_ptr(), wts.data_ptr(), C.byref(n_e), ws.data_ptr(),
                                     ws.numel(), None))
    device_call()
    torch.cuda.synchronize()
    rows, wall = [], []
    with hip.stage_timer("pcseg") as timer:
        for _ in range(iters):
            t0 = time.perf_counter()
            device_call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            rows.append(timer.read())
    names = timer.names
    E = n_e.value
    us = np.median(np.asarray(rows), 0)
    total = float(us.sum())
    stages = {nm: dict(us=round(float(u), 1), share=round(float(u) / total, 4)) for nm, u in zip(names, us)}
    stages["knn"]["pair_scores"] = N * N
    stages["knn"]["pair_scores_per_s"] = round(N * N / (float(us[names.index("knn")]) * 1e-6), 0)
    h_e, h_w = edges[:E].cpu().numpy(), wts[:E].cpu().numpy()
    chain = []
    for _ in range(3):
        t0 = time.perf_counter()
        seg = oversegment.merge_edges(h_e, h_w, N)
        chain.append(time.perf_counter() - t0)
    whole = []
    for _ in range(max(iters // 2, 2)):
        t0 = time.perf_counter()
        seg2 = oversegment.segment_pointcloud(scan.xyz, k, device="cuda:0")
        whole.append(time.perf_counter() - t0)
    assert np.array_equal(seg, seg2)
    med = lambda x: round(float(np.median(x)) * 1e3, 3)                          # noqa: E731
    return dict(lattice=f"{w}x{h}", N=N, k=k, E=E, segments=int(np.unique(seg).shape[0]), negative_weights=int((h_w < 0).sum()), stages=stages,
                device_call_event_sum_ms=round(total / 1e3, 3), device_call_wall_ms=med(wall), host_chain_ms=med(chain),
                segment_pointcloud_whole_call_ms=med(whole))


def mesh_row(V):
    """the mesh path's measurements at the same number of vertices (profiles/overseg_time.json), or the reason there are none"""
    p = os.path.join(ROOT, "profiles", "overseg_time.json")
    if not os.path.exists(p):
        return "not measured: profiles/overseg_time.json is missing"
    for m in json.load(open(p))["meshes"]:
        if m["V"] == V:
            return {key: m[key] for key in ("V", "F", "E", "segments", "device_call_event_sum_ms", "device_call_wall_ms", "host_chain_ms",
                                            "segment_mesh_whole_call_ms")}
    return "not measured: no mesh of %d vertices in profiles/overseg_time.json" % V


def table(doc):
    cs = doc["clouds"]
    lines = ["| what | " + " | ".join(f"{m['N']:,} points, k = {m['k']}: {m['E']:,} edges" for m in cs) + " |", "|---|" + "---|" * len(cs)]
    for nm in cs[0]["stages"]:
        lines.append(f"| `{nm}` (events): µs, share of the call | " + " | ".join(f"{m['stages'][nm]['us']:,.0f}, {100 * m['stages'][nm]['share']:.2f} %" for m in cs) + " |")
    lines.append("| kNN: pair scores, 10^9 per second | " + " | ".join(f"{m['stages']['knn']['pair_scores']:.3g}, {m['stages']['knn']['pair_scores_per_s'] / 1e9:,.0f}" for m in cs) + " |")
    for key, label in (("device_call_event_sum_ms", "all device stages, sum of the events, ms"), ("device_call_wall_ms", "`sg_pcseg_edges`, host wall time, ms"),
                       ("host_chain_ms", "host chain `sg_overseg_merge`, ms"), ("segment_pointcloud_whole_call_ms", "whole call `segment_pointcloud`, ms")):
        lines.append(f"| {label} | " + " | ".join(f"{m[key]:,.3f}" for m in cs) + " |")
    for key, label in (("E", "mesh path at the same V: edges"), ("device_call_event_sum_ms", "mesh path: all device stages, ms"), ("host_chain_ms", "mesh path: host chain, ms"),
                       ("segment_mesh_whole_call_ms", "mesh path: whole call `segment_mesh`, ms")):
        lines.append(f"| {label} | " + " | ".join(f"{m['mesh_path'][key]:,}" if isinstance(m["mesh_path"], dict) else m["mesh_path"] for m in cs) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="400x375,800x625", help="lattices of make_room_scan: 150,000 and 500,000 points")
    ap.add_argument("--knn", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcseg_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, runs="one process, one GPU, medians over the timed iterations", clouds=[])
    for w, h in (tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")):
        m = measure(w, h, a.knn, a.iters)
        m["mesh_path"] = mesh_row(m["N"])
        doc["clouds"].append(m)
        print(json.dumps(m), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
