#!/usr/bin/env python3
"""Mesh over-segmentation, measured -> profiles/overseg_time.json, and the DESIGN table generated from that file.

    python tools/time_overseg.py [--sizes 400x375,800x625] [--iters 10] [--out profiles/overseg_time.json] [--no-rocprof]
    python tools/time_overseg.py --table profiles/overseg_time.json        # prints the markdown table of DESIGN.md 8d (no GPU needed)

Per mesh size, all taken in one run: every device stage of sg_overseg_edges by HIP events (sg_overseg_set_timing) with its algorithmic
bytes and GB/s; the kernels of one `rocprofv3 --kernel-trace --stats` run of a child process; the host chain (sg_overseg_merge) in ms;
the whole call (segment_mesh: upload, device stages, copy back, chain) beside the rest of prepare_scene for the same scan.  What could
not be measured is recorded as "not measured" with the reason.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stage_bytes(V, F, E):
    """algorithmic bytes per stage (reads + writes of the arrays a stage touches once; gathers counted at their element size)"""
    n = 3 * F
    passes_v = -(-max(int(V).bit_length(), 1) // 11)
    return {
        "check": 12 * V + 12 * F,
        "face_normals": 12 * F + 36 * F + 12 * F + 8 * n,                      # faces, three gathered corners, normals, (vertex, face) pairs
        "incidence_sort": passes_v * 20 * n,                                   # per pass: keys for the histogram, keys + values in and out
        "vertex_normals": 8 * n + 12 * n + 12 * V,                             # sorted pairs, gathered face normals, normals
        "edges": 12 * F + 8 * n + 4 * 24 * n + 12 * n + 16 * E,                # sg_mesh_adjacency: keys, four 64-bit passes, unique, unpack
        "weights": 16 * E + 48 * E + 12 * E,                                   # edge list, normals + coordinates of both ends, w / key / index
        "weight_sort": 3 * 20 * E,
        "gather": 4 * E + 16 * E + 4 * E + 12 * E,
    }


def measure(w, h, iters):
    import torch
    from seggroup_amd import hip, oversegment, prepare, synthetic
    lib = hip.lib()
    scan = synthetic.make_room_scan(w, h, 11, jitter=5e-4, name="scene0000_00")
    V, F = scan.xyz.shape[0], scan.faces.shape[0]
    d_xyz, d_f = torch.from_numpy(scan.xyz).cuda(), torch.from_numpy(scan.faces).cuda()
    nrm = torch.empty((V, 3), dtype=torch.float32, device="cuda")
    edges = torch.empty((3 * F, 2), dtype=torch.int32, device="cuda")
    wts = torch.empty(3 * F, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.sg_overseg_ws_bytes(V, F), dtype=torch.uint8, device="cuda")
    n_e = C.c_int(0)

    def device_call():
        hip.check(lib.sg_overseg_edges(d_xyz.data_ptr(), V, d_f.data_ptr(), F, None, nrm.data_ptr(), edges.data_ptr(), wts.data_ptr(), C.byref(n_e),
                                       ws.data_ptr(), ws.numel(), None))
    for _ in range(3):
        device_call()
    torch.cuda.synchronize()
    rows, wall = [], []
    with hip.stage_timer("overseg") as timer:
        for _ in range(iters):
            t0 = time.perf_counter()
            device_call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            rows.append(timer.read())
    names = timer.names
    E = n_e.value
    us = np.median(np.asarray(rows), 0)
    nbytes = stage_bytes(V, F, E)
    stages = {nm: dict(us=round(float(u), 1), bytes=int(nbytes[nm]), gb_per_s=round(nbytes[nm] / max(float(u), 1e-3) / 1e3, 1)) for nm, u in zip(names, us)}
    h_e, h_w = edges[:E].cpu().numpy(), wts[:E].cpu().numpy()
    chain = []
    for _ in range(max(iters // 2, 3)):
        t0 = time.perf_counter()
        seg = oversegment.merge_edges(h_e, h_w, V)
        chain.append(time.perf_counter() - t0)
    whole = []
    for _ in range(max(iters // 2, 3)):
        t0 = time.perf_counter()
        seg2 = oversegment.segment_mesh(scan.xyz, scan.faces, device="cuda:0")
        whole.append(time.perf_counter() - t0)
    assert np.array_equal(seg, seg2)
    # the rest of prepare_scene for the same scan (segs.json present): point cloud + unmapper, segment lists, mesh adjacency, with their files
    tmp = tempfile.mkdtemp(prefix="overseg_time_")
    try:
        sp = os.path.join(tmp, "scans", scan.name)
        os.makedirs(sp)
        prepare.write_ply(os.path.join(sp, scan.name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
        t0 = time.perf_counter()
        oversegment.oversegment_scan(sp, device="cuda:0")
        t_file = time.perf_counter() - t0
        rest = []
        for it in range(3):
            root = os.path.join(tmp, "root%d" % it)
            t0 = time.perf_counter()
            prepare.prepare_scene(sp, 0, 150000, root=root, perm=scan.perm, device="cuda:0")
            rest.append(time.perf_counter() - t0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    med = lambda x: round(float(np.median(x)) * 1e3, 3)                          # noqa: E731
    return dict(lattice=f"{w}x{h}", V=V, F=F, E=E, segments=int(np.unique(seg).shape[0]), stages=stages,
                device_call_event_sum_ms=round(float(us.sum()) / 1e3, 3), device_call_wall_ms=med(wall), host_chain_ms=med(chain),
                segment_mesh_whole_call_ms=med(whole), oversegment_scan_with_ply_read_and_json_write_ms=round(t_file * 1e3, 1),
                rest_of_prepare_scene_ms=med(rest), rest_of_prepare_scene_first_ms=round(rest[0] * 1e3, 1))


def only_device(w, h, iters):
    from seggroup_amd import oversegment, synthetic
    scan = synthetic.make_room_scan(w, h, 11, jitter=5e-4)
    for _ in range(iters):
        oversegment.device_edges(scan.xyz, scan.faces, device="cuda:0")


def rocprof_kernels(size, iters):
    """one child process under rocprofv3 --kernel-trace --stats -> {kernel: (calls, average us)} of the over-segmenter's launches"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return "not measured: rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="overseg_prof_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--only-device", "--sizes", size,
                            "--iters", str(iters)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        if r.returncode != 0:
            return "not measured: rocprofv3 run failed: " + (r.stdout + r.stderr)[-300:]
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return "not measured: no kernel_stats.csv in the profiler's output"
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "").replace("(anonymous namespace)::", "").strip()
            name = name[5:] if name.startswith("void ") else name
            short = name.split("(")[0].split("<")[0].split("::")[-1].strip()
            if short.startswith(("k_os_", "k_rs_", "k_face_edges", "k_unpack_edges", "k_head_flags", "k_scan_", "k_compact_heads")):
                e = out.setdefault(short, dict(calls=0, total_us=0.0))
                e["calls"] += int(row["Calls"])
                e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for e in out.values():
            e["avg_us"] = round(e["total_us"] / max(e["calls"], 1), 2)
            e["total_us"] = round(e["total_us"], 1)
        return dict(runs_of_the_device_call=iters, kernels=out)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def table(doc):
    lines = ["| what | " + " | ".join(f"{m['V']:,} vertices / {m['F']:,} faces / {m['E']:,} edges" for m in doc["meshes"]) + " |",
             "|---|" + "---|" * len(doc["meshes"])]
    for nm in doc["meshes"][0]["stages"]:
        lines.append(f"| `{nm}` (events): µs, GB/s | " + " | ".join(f"{m['stages'][nm]['us']:g}, {m['stages'][nm]['gb_per_s']:g}" for m in doc["meshes"]) + " |")
    for key, label in (("device_call_event_sum_ms", "all device stages, sum of the events, ms"), ("device_call_wall_ms", "`sg_overseg_edges`, host wall time, ms"),
                       ("host_chain_ms", "host chain `sg_overseg_merge`, ms"), ("segment_mesh_whole_call_ms", "whole call `segment_mesh` (upload, stages, copy back, chain), ms"),
                       ("rest_of_prepare_scene_ms", "rest of `prepare_scene` for the same scan (150,000 points, files included), ms")):
        lines.append(f"| {label} | " + " | ".join(f"{m[key]:g}" for m in doc["meshes"]) + " |")
    for m in doc["meshes"]:
        rp = m.get("rocprofv3")
        if isinstance(rp, dict):
            ks = ", ".join(f"`{k}` {v['avg_us']:g} x {v['calls'] // rp['runs_of_the_device_call']}" for k, v in sorted(rp["kernels"].items()) if k.startswith("k_os_"))
            lines.append(f"| `rocprofv3 --kernel-trace --stats`, {m['lattice']}: average µs x launches per call | " + ks + " |" + " |" * (len(doc["meshes"]) - 1))
        elif rp:
            lines.append(f"| `rocprofv3`, {m['lattice']} | {rp} |" + " |" * (len(doc["meshes"]) - 1))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="400x375,800x625", help="lattices of make_room_scan: 150,000 and 500,000 vertices")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overseg_time.json"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--only-device", action="store_true", help="only the device call (the child of the profiler run)")
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")]
    if a.only_device:
        for w, h in sizes:
            only_device(w, h, a.iters)
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, band_tb_per_s_of_memory_bound_launches="3-5 (DESIGN.md section 4)", meshes=[])
    for w, h in sizes:
        m = measure(w, h, a.iters)
        m["rocprofv3"] = "not measured: --no-rocprof" if a.no_rocprof else rocprof_kernels(f"{w}x{h}", 5)
        doc["meshes"].append(m)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    print(table(doc))


if __name__ == "__main__":
    main()
