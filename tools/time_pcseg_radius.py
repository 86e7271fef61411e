#!/usr/bin/env python3
"""The point-cloud over-segmenter over the radius graph, measured -> profiles/pcseg_radius_time.json, and the DESIGN table
generated from that file.

    python tools/time_pcseg_radius.py [--repeats 5] [--out profiles/pcseg_radius_time.json] [--max-pairs 400000000]
    python tools/time_pcseg_radius.py --table profiles/pcseg_radius_time.json      # prints the markdown table of DESIGN.md 8l (no GPU needed)

One process, one GPU, one stream.  Per (cloud, radius): T from the query form; sg_pcseg_edges_radius between two events on the stream after
a warm-up, the median (min .. max) of the repeats; its thirteen stages by the library's own events (sg_pcseg_radius_set_timing), the median
of three further repeats; the mean and the largest row; the host chain (sg_overseg_merge on the downloaded edges) and the whole call
(segment_pointcloud(radius=): query, workspace, device stages, download, chain) on the host's clock, once each.  The normals stage is put
beside the records it gathers -- 2 (T + N) packed 16-byte records, each load waiting for the index before it -- as records per second.
Beside each cloud what the parent commit offers on it: segment_pointcloud(index="grid", k=10), its time and its segment count.  That is
ANOTHER GRAPH, and the table says so.
Clouds: the 150,000-point room cloud of tools/time_pcseg.py (a 0.04 lattice with a jitter of 5e-4) at 0.048 and at 0.1, and
tests/thin_ref.big_cloud() (1,058,050 points: a 0.025 lattice, every site 50 times within 0.004) at 0.0075 and at 0.03.  A case whose T
is above --max-pairs is not run, and the file says so with T and the workspace it would need.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOT_MEASURED = ["several streams in flight", "clouds near 2^24 points", "real scans", "forced cells with R > 1 on the large clouds",
                "rows far above a few hundred entries (the rows stage is quadratic in a row's length)",
                "hardware counters of k_pc_normals_csr (the gather-bound reading rests on its time against the records it loads)",
                "a radix sort of (i, j) keys in place of the rank sort of the rows (not built)"]
CLOUDS = (("150,000-point room", "room", 0.048), ("150,000-point room", "room", 0.1), ("1,058,050 points", "big", 0.0075),
          ("1,058,050 points", "big", 0.03))


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3), repeats=repeats)


def parent_route(d_x, repeats):
    """what the parent commit offers on the same cloud: the kNN-10 graph on the grid index -- another graph"""
    from seggroup_amd import oversegment
    t, seg = [], None
    for _ in range(max(repeats, 1)):
        t0 = time.perf_counter()
        seg = oversegment.segment_pointcloud(d_x, 10, device="cuda:0", index="grid")
        t.append((time.perf_counter() - t0) * 1e3)
    sizes = np.unique(seg, return_counts=True)[1]
    return dict(whole_call_ms=round(float(np.median(t)), 1), segments=int(sizes.shape[0]), largest_segment=int(sizes.max()), runs=len(t))


def measure(label, xyz, radius, repeats, max_pairs):
    import torch
    from seggroup_amd import components, hip, oversegment
    lib = hip.lib()
    n = xyz.shape[0]
    d_x = torch.from_numpy(xyz).cuda()
    out = dict(cloud=label, N=int(n), radius=radius)
    t_pairs = components.radius_pairs(d_x, n, radius, 0.0, "cuda:0", None)[0]
    need = int(lib.sg_pcseg_ws_bytes_radius(n, t_pairs))
    out.update(T=int(t_pairs), E=int(t_pairs // 2), workspace_bytes=need, parent_knn10_grid=parent_route(d_x, min(repeats, 3)))
    if t_pairs > max_pairs:
        out.update(run=False, why="T = %d: above --max-pairs %d (a workspace of %.1f GB and %.1f GB of edges on the host)" %
                   (t_pairs, max_pairs, need / 1e9, t_pairs // 2 * 12 / 1e9))
        return out
    e = max(t_pairs // 2, 1)
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    idx = torch.empty(max(t_pairs, 1), dtype=torch.int32, device="cuda")
    nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    edges = torch.empty((e, 2), dtype=torch.int32, device="cuda")
    w = torch.empty(e, dtype=torch.float32, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    n_e, total = C.c_int(0), C.c_int64(0)

    def call():
        hip.check(lib.sg_pcseg_edges_radius(d_x.data_ptr(), n, radius, 0.0, t_pairs, None, off.data_ptr(), idx.data_ptr(), nrm.data_ptr(),
                                            edges.data_ptr(), w.data_ptr(), C.byref(n_e), C.byref(total), ws.data_ptr(), ws.numel(), None))

    out.update(run=True, edges_call_ms=timed(call, repeats))
    rows = []
    with hip.stage_timer("pcseg_radius") as timer:
        for _ in range(3):
            call()
            rows.append(timer.read())
    names = timer.names
    us =np.median(np.asarray(rows), 0)
    length = (off[1:] - off[:-1])
    out.update(stages_us={nm: round(float(u), 1) for nm, u in zip(names, us)}, mean_row=round(float(length.double().mean()), 2),
               max_row=int(length.max()), sum_row_squared_over_64=float((length.double() ** 2).sum() / 64.0))
    records = 2.0 * (t_pairs + n)
    out["normals_records_per_s"] = round(records / (float(us[names.index("normals")]) * 1e-6))
    out["normals_gathered_bytes_per_s"] = round(16.0 * records / (float(us[names.index("normals")]) * 1e-6))
    h_edges, h_w = edges[:n_e.value].cpu().numpy(), w[:n_e.value].cpu().numpy()
    t0 = time.perf_counter()
    seg = oversegment.merge_edges(h_edges, h_w, n)
    out["host_chain_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    del ws, edges, w, idx
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    seg2 = oversegment.segment_pointcloud(d_x, radius=radius, device="cuda:0")
    out["whole_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert np.array_equal(seg, seg2)
    sizes = np.unique(seg, return_counts=True)[1]
    out.update(segments=int(sizes.shape[0]), largest_segment=int(sizes.max()))
    return out


def table(doc):
    gs = doc["clouds"]
    ran = lambda g, f: f(g) if g.get("run") else "not run"          # noqa: E731
    ms = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"     # noqa: E731
    lines = ["| what | " + " | ".join(f"{g['cloud']}, radius {g['radius']:g}" for g in gs) + " |", "|---|" + "---|" * len(gs)]
    lines.append("| T (ordered pairs); edges E; workspace, GB | " + " | ".join(f"{g['T']:,}; {g['E']:,}; {g['workspace_bytes'] / 1e9:.2f}" for g in gs) + " |")
    lines.append("| row length: mean; max | " + " | ".join(ran(g, lambda g: f"{g['mean_row']:,}; {g['max_row']:,}") for g in gs) + " |")
    first = next((g for g in gs if g.get("run")), None)
    if first:
        lines.append(f"| `sg_pcseg_edges_radius` between events, ms: median (min .. max) of {first['edges_call_ms']['repeats']} | " +
                     " | ".join(ran(g, lambda g: ms(g["edges_call_ms"])) for g in gs) + " |")
        for nm in first["stages_us"]:
            lines.append(f"| `{nm}` (the library's events), µs | " + " | ".join(ran(g, lambda g: f"{g['stages_us'][nm]:,.1f}") for g in gs) + " |")
        lines.append("| `normals`: packed records gathered per second; bytes per second | " + " | ".join(
            ran(g, lambda g: f"{g['normals_records_per_s']:.3g}; {g['normals_gathered_bytes_per_s']:.3g}") for g in gs) + " |")
    lines.append("| host chain (`sg_overseg_merge`), ms, one run | " + " | ".join(ran(g, lambda g: f"{g['host_chain_ms']:,}") for g in gs) + " |")
    lines.append("| the whole call `segment_pointcloud(radius=)`, ms, one run; segments; the largest | " + " | ".join(
        ran(g, lambda g: f"{g['whole_call_ms']:,}; {g['segments']:,}; {g['largest_segment']:,}") for g in gs) + " |")
    lines.append("| the parent commit on the same cloud, `segment_pointcloud(index=\"grid\", k=10)` -- ANOTHER GRAPH: ms; segments; the largest | " +
                 " | ".join(f"{g['parent_knn10_grid']['whole_call_ms']:,}; {g['parent_knn10_grid']['segments']:,}; "
                            f"{g['parent_knn10_grid']['largest_segment']:,}" for g in gs) + " |")
    lines += ["", "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-pairs", type=int, default=400_000_000, help="a case with more ordered pairs than this is reported, not run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcseg_radius_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import thin_ref
    from seggroup_amd import synthetic
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; host figures are one run", not_measured=list(NOT_MEASURED),
               clouds=[])
    clouds = {"big": thin_ref.big_cloud()[0], "room": synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz}
    for label, which, radius in CLOUDS:
        m = measure(label, np.ascontiguousarray(clouds[which], dtype=np.float32), radius, a.repeats, a.max_pairs)
        if not m["run"]:
            doc["not_measured"].append("%s at radius %g (%s)" % (label, radius, m["why"]))
        doc["clouds"].append(m)
        print(json.dumps(m), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                              # after every cloud: a long case that is cut off loses only itself
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
