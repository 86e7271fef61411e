#!/usr/bin/env python3
"""Voxel thinning, measured -> profiles/thin_time.json, and the DESIGN table generated from that file.

    python tools/time_thin.py [--sides 1150,2300] [--iters 3] [--out profiles/thin_time.json]
    python tools/time_thin.py --table profiles/thin_time.json        # prints the markdown table of DESIGN.md 8g (no GPU needed)

Per cloud, all taken in one run: every device stage of sg_cloud_thin by HIP events (sg_cloud_thin_set_timing), the call by wall clock,
and the NumPy statement of the specification (tests/thin_ref.py) on the same host for the same input -- the reference here: the parent of
this change refuses these inputs -- with the ratio.  The outputs of the two are compared while at it.  The clouds: tests/thin_ref.py's
1,058,050 points at h = 0.05, and pcseg_ref.make_room_cloud lattices of `side` points a side (1150: about 4 M points, 2300: about 16 M)
at the edge that leaves about 500 k voxels.  The per-voxel argmin is the 64-bit atomicMin: `argmin_by_sort_estimate_us` is what the
alternative of 8g -- three more 11-bit radix passes, over the 32 bits of d2 -- would cost at the measured time of a pass.  Last,
segment_pointcloud(voxel = 0.05) on the large cloud against the un-thinned call on its first 1,000,000 points.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(label, xyz, voxel, iters):
    import torch
    import thin_ref as T
    from seggroup_amd import hip
    lib = hip.lib()
    n = xyz.shape[0]
    d_xyz = torch.from_numpy(xyz).cuda()
    rep = torch.empty(n, dtype=torch.int32, device="cuda")
    top = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sg_cloud_thin_ws_bytes(n), dtype=torch.uint8, device="cuda")
    m = C.c_int(0)

    def device_call():
        hip.check(lib.sg_cloud_thin(d_xyz.data_ptr(), 3, n, float(voxel), rep.data_ptr(), top.data_ptr(), C.byref(m), None, ws.data_ptr(),
                                    ws.numel(), None))
    device_call()
    torch.cuda.synchronize()
    rows, wall = [], []
    with hip.stage_timer("cloud_thin") as timer:
        for _ in range(iters):
            t0 = time.perf_counter()
            device_call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            rows.append(timer.read())
    names = timer.names
    us =np.median(np.asarray(rows), 0)
    total = float(us.sum())
    stages = {nm: dict(us=round(float(u), 1), share=round(float(u) / total, 4)) for nm, u in zip(names, us)}
    t0 = time.perf_counter()
    want_rep, want_top, _ = T.thin(xyz, voxel)
    ref_s = time.perf_counter() - t0
    cells, largest = T.stats(xyz, voxel, want_rep, want_top)
    key_bits = sum(max(int(c) - 1, 0).bit_length() for c in cells)
    passes = -(-key_bits // 11)
    equal = bool(m.value == want_rep.shape[0] and np.array_equal(rep[:m.value].cpu().numpy(), want_rep) and np.array_equal(top.cpu().numpy(), want_top))
    wall_ms = float(np.median(wall)) * 1e3
    out = dict(cloud=label, N=n, voxel=float(np.float32(voxel)), M=int(m.value), cells=cells, largest_voxel=largest, key_bits=key_bits,
               radix_passes=passes, stages=stages, device_call_event_sum_ms=round(total / 1e3, 3), device_call_wall_ms=round(wall_ms, 3),
               points_per_s=round(n / (wall_ms * 1e-3), 0), numpy_statement_ms=round(ref_s * 1e3, 1), numpy_over_device=round(ref_s * 1e3 / wall_ms, 1),
               equal_to_the_statement=equal, workspace_bytes=int(ws.numel()))
    if passes:
        out["argmin_by_sort_estimate_us"] = round(3 * float(us[names.index("sort")]) / passes, 1)
    return out


def measure_segmenter(iters):
    import thin_ref as T
    from seggroup_amd import oversegment
    big, _ = T.big_cloud()
    oversegment.segment_pointcloud(big, voxel=0.05, device="cuda:0")
    thinned, plain = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        oversegment.segment_pointcloud(big, voxel=0.05, device="cuda:0")
        thinned.append(time.perf_counter() - t0)
    first = np.ascontiguousarray(big[:1000000])
    for _ in range(2):
        t0 = time.perf_counter()
        oversegment.segment_pointcloud(first, device="cuda:0")
        plain.append(time.perf_counter() - t0)
    a, b = float(np.median(thinned)) * 1e3, float(min(plain)) * 1e3
    return dict(thinned_points=int(big.shape[0]), thinned_voxel=0.05, thinned_whole_call_ms=round(a, 3), unthinned_points=int(first.shape[0]),
                unthinned_whole_call_ms=round(b, 3), unthinned_over_thinned=round(b / a, 1))


def table(doc):
    cs = doc["clouds"]
    lines = ["| what | " + " | ".join(f"{m['N']:,} points, h = {m['voxel']:.4g}: {m['M']:,} voxels" for m in cs) + " |", "|---|" + "---|" * len(cs)]
    lines.append("| cells per axis; key bits, radix passes; largest voxel | " + " | ".join(
        f"{' x '.join(str(c) for c in m['cells'])}; {m['key_bits']}, {m['radix_passes']}; {m['largest_voxel']:,}" for m in cs) + " |")
    for nm in cs[0]["stages"]:
        lines.append(f"| `{nm}` (events): µs, share of the call | " + " | ".join(f"{m['stages'][nm]['us']:,.0f}, {100 * m['stages'][nm]['share']:.1f} %" for m in cs) + " |")
    lines.append("| argmin by three more sort passes instead, estimate, µs | " + " | ".join(f"{m.get('argmin_by_sort_estimate_us', 0):,.0f}" for m in cs) + " |")
    for key, label in (("device_call_event_sum_ms", "all device stages, sum of the events, ms"), ("device_call_wall_ms", "`sg_cloud_thin`, host wall time, ms"),
                       ("numpy_statement_ms", "the NumPy statement on the same host, ms"), ("numpy_over_device", "NumPy / device"),
                       ("equal_to_the_statement", "outputs equal to the statement's")):
        lines.append(f"| {label} | " + " | ".join(f"{m[key]:,}" if not isinstance(m[key], bool) else ("yes" if m[key] else "NO") for m in cs) + " |")
    s = doc.get("segmenter")
    if s:
        lines += ["", f"`segment_pointcloud(voxel = {s['thinned_voxel']})` on {s['thinned_points']:,} points: {s['thinned_whole_call_ms']:,.1f} ms; "
                      f"un-thinned on the first {s['unthinned_points']:,}: {s['unthinned_whole_call_ms']:,.1f} ms ({s['unthinned_over_thinned']:,} x)."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="1150,2300", help="make_room_cloud lattices: about 4 M and about 16 M points")
    ap.add_argument("--voxels-left", type=float, default=500e3, help="the lattices are thinned at the edge that leaves about this many voxels")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-segmenter", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import pcseg_ref
    import thin_ref as T
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, runs="one process, one GPU, medians over the timed iterations", clouds=[])
    big, _ = T.big_cloud()
    jobs = [("room_20k x 50", big, 0.05)]
    del big
    spacing = 0.0025
    for side in (int(s) for s in a.sides.split(",") if s):
        jobs.append((side, None, None))
    for label, xyz, h in jobs:
        if xyz is None:
            xyz, _ = pcseg_ref.make_room_cloud(label, spacing, 2.5e-5, seed=9)
            h = spacing * math.sqrt(xyz.shape[0] / a.voxels_left)
            label = "make_room_cloud(%d, %g, 2.5e-5, seed=9)" % (label, spacing)
        m = measure(label, xyz, h, a.iters)
        doc["clouds"].append(m)
        print(json.dumps(m), flush=True)
        del xyz
    if not a.no_segmenter:
        doc["segmenter"] = measure_segmenter(a.iters)
        print(json.dumps(doc["segmenter"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
