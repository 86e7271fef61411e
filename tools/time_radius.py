#!/usr/bin/env python3
"""The radius graph, measured -> profiles/radius_time.json, and the DESIGN table generated from that file.

    python tools/time_radius.py [--repeats 5] [--out profiles/radius_time.json]
    python tools/time_radius.py --table profiles/radius_time.json      # prints the markdown table of DESIGN.md 8k (no GPU needed)

One process, one GPU, one stream.  Per (cloud, radius): sg_components_radius and sg_radius_count_grid between two events on the stream after
a warm-up, the median (min .. max) of the repeats; every stage of the components call by the library's own events (sg_radius_grid_set_timing)
from three further repeats, with the pair tests evaluated and the pairs passed of a timed call.  Beside it what the library offered before:
sg_pointcloud_knn_grid (k = 10) + sg_components_knn cut at the same length -- a DIFFERENT graph, its component count is reported beside the
radius graph's -- and the host route, scipy's cKDTree.query_pairs + csgraph.connected_components, run once; the kd-tree and the pair list are
built outside the host's clock, the labelling and the relabelling to the lowest index inside it.  The host route is run where the radius
graph has at most --host-pairs edges (its pair list is 16 bytes an edge); where it is not run the file says so.
Clouds: tests/thin_ref.big_cloud() (1,058,050 points: a 0.025 lattice, every site 50 times within 0.004) at 0.03 and at a quarter of that,
and the 150,000-point room cloud of tools/time_pcseg.py (a 0.04 lattice with a jitter of 5e-4) at 0.048.
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

NOT_MEASURED = ["the number of CAS retries (no counter is compiled in)", "several streams in flight", "clouds near 2^24 points", "real scans",
                "forced cells with R > 1 on the large clouds", "the label filter's cost",
                "the hook visitor with a root comparison in front of the distance test (not built: see DESIGN.md 8k)"]


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


def host_route(xyz, radius, edges, host_pairs):
    """-> dict: cKDTree.query_pairs (outside the clock) + connected_components + the lowest-index relabelling (inside it), once"""
    if edges > host_pairs:
        return dict(run=False, why="%d edges: above --host-pairs %d" % (edges, host_pairs))
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = xyz.shape[0]
    t0 = time.perf_counter()
    e = cKDTree(xyz.astype(np.float64)).query_pairs(float(np.float32(radius)), output_type="ndarray")
    t1 = time.perf_counter()
    print("host: %d pairs in %.1f s" % (e.shape[0], t1 - t0), flush=True)
    c, lab = connected_components(coo_matrix((np.ones(e.shape[0], np.int8), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    low = np.full(c, n, np.int64)
    np.minimum.at(low, lab, np.arange(n))
    comp = low[lab].astype(np.int32)
    t2 = time.perf_counter()
    return dict(run=True, pairs=int(e.shape[0]), pairs_s=round(t1 - t0, 2), components_ms=round((t2 - t1) * 1e3, 1), C=int(c), comp=comp)


def measure(label, xyz, radius, repeats, host_pairs):
    import torch
    from seggroup_amd import components as M
    from seggroup_amd import hip, prepare
    lib = hip.lib()
    n = xyz.shape[0]
    d_x = torch.from_numpy(xyz).cuda()
    comp = torch.empty(n, dtype=torch.int32, device="cuda")
    size = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sg_radius_grid_ws_bytes(n), dtype=torch.uint8, device="cuda")
    c = C.c_int(0)

    def components():
        hip.check(lib.sg_components_radius(d_x.data_ptr(), 3, n, radius, 0.0, None, comp.data_ptr(), size.data_ptr(), C.byref(c), ws.data_ptr(),
                                           ws.numel(), None))

    def count():
        hip.check(lib.sg_radius_count_grid(d_x.data_ptr(), 3, n, radius, 0.0, cnt.data_ptr(), ws.data_ptr(), ws.numel(), None))

    out = dict(cloud=label, N=int(n), radius=radius, components_ms=timed(components, repeats), count_ms=timed(count, repeats))
    rows = []
    with hip.stage_timer("radius_grid") as timer:
        for _ in range(3):
            components()
            rows.append(timer.read())
    names, stats = timer.names, M.radius_stats()
    us = np.median(np.asarray(rows), 0)
    got = comp.cpu().numpy()
    sizes = np.sort(np.bincount(got)[np.unique(got)])[::-1]
    med = out["components_ms"]["median"]
    out.update(C=int(c.value), largest_sizes=sizes[:5].tolist(), stages_us={nm: round(float(u), 1) for nm, u in zip(names, us)},
               cells=stats["cells"], occupied=stats["occupied"], largest_cell=stats["largest_cell"], cell=stats["cell"], R=stats["R"],
               pair_tests=stats["pair_tests"], pairs_passed=stats["pairs_passed"], share_of_n2=stats["pair_tests"] / float(n) / float(n),
               pair_tests_per_s=round(stats["pair_tests"] / (float(us[names.index("search")]) * 1e-6)),
               max_count=int(cnt.max()), mean_count=round(float(cnt.double().mean()), 2), workspace_bytes=int(ws.numel()))
    assert int(cnt.long().sum()) == stats["pairs_passed"]
    # what the library offered before: the kNN-10 table of the grid index, cut at the same length -- another graph
    state = {}

    def knn_route():
        state["table"] = prepare.pointcloud_knn(d_x, 10, device="cuda:0", index="grid")
        state["out"] = M.components(n, knn=state["table"], xyz=d_x, max_edge=radius, device="cuda:0")

    out["knn10_ms"] = timed(knn_route, repeats)
    out["knn10_C"] = int(state["out"][2])
    out["knn10_over_radius"] = round(out["knn10_ms"]["median"] / med, 2)
    host = host_route(xyz, radius, stats["pairs_passed"] // 2, host_pairs)
    if host["run"]:
        want = host.pop("comp")
        host["equal_to_the_device"] = bool(np.array_equal(want, got) and host["C"] == c.value)
        host["components_over_device"] = round(host["components_ms"] / med, 1)
    out["host"] = host
    return out


def table(doc):
    gs = doc["clouds"]
    ms = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"     # noqa: E731
    lines = ["| what | " + " | ".join(f"{g['cloud']}, radius {g['radius']:g}" for g in gs) + " |", "|---|" + "---|" * len(gs)]
    lines.append("| points; cells per axis; occupied; the largest cell; cell edge; R | " + " | ".join(
        f"{g['N']:,}; {'x'.join(map(str, g['cells']))}; {g['occupied']:,}; {g['largest_cell']:,}; {g['cell']:.5g}; {g['R']}" for g in gs) + " |")
    lines.append("| components of the radius graph; the largest | " + " | ".join(
        f"{g['C']:,}; {', '.join(format(s, ',') for s in g['largest_sizes'][:3])}" for g in gs) + " |")
    lines.append("| neighbours per point: mean; max | " + " | ".join(f"{g['mean_count']:,}; {g['max_count']:,}" for g in gs) + " |")
    lines.append(f"| `sg_components_radius` between events, ms: median (min .. max) of {gs[0]['components_ms']['repeats']} | " +
                 " | ".join(ms(g["components_ms"]) for g in gs) + " |")
    lines.append("| `sg_radius_count_grid`, ms | " + " | ".join(ms(g["count_ms"]) for g in gs) + " |")
    for nm in gs[0]["stages_us"]:
        lines.append(f"| `{nm}` (the library's events, components call), µs | " + " | ".join(f"{g['stages_us'][nm]:,.1f}" for g in gs) + " |")
    lines.append("| pair tests; share of N^2; pairs passed (ordered) | " + " | ".join(
        f"{g['pair_tests']:.4g}; {g['share_of_n2']:.3g}; {g['pairs_passed']:.4g}" for g in gs) + " |")
    lines.append("| pair tests per second of `search` | " + " | ".join(f"{g['pair_tests_per_s']:.3g}" for g in gs) + " |")
    lines.append("| kNN-10 on the grid + `sg_components_knn` cut at the radius (another graph), ms; its components | " + " | ".join(
        f"{ms(g['knn10_ms'])}; {g['knn10_C']:,}" for g in gs) + " |")
    lines.append("| host: `connected_components` on `query_pairs`' list, ms (ratio to the device call); the list itself, s | " + " | ".join(
        (f"{g['host']['components_ms']:,} ({g['host']['components_over_device']:,} x); {g['host']['pairs_s']:,}" +
         ("" if g["host"]["equal_to_the_device"] else " -- OUTPUTS DIFFER")) if g["host"]["run"] else "not run (" + g["host"]["why"] + ")" for g in gs) + " |")
    lines += ["", "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=60_000_000, help="run the host route where the radius graph has at most this many edges")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import thin_ref
    from seggroup_amd import synthetic
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; the host figure is one run", not_measured=list(NOT_MEASURED),
               clouds=[])
    big, _ = thin_ref.big_cloud()
    room = synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz
    for label, xyz, radius in (("1,058,050 points", big, 0.03), ("1,058,050 points", big, 0.0075), ("150,000-point room", room, 0.048)):
        m = measure(label, np.ascontiguousarray(xyz, dtype=np.float32), radius, a.repeats, a.host_pairs)
        if not m["host"]["run"]:
            doc["not_measured"].append("the host route on %s at radius %g (%s)" % (label, radius, m["host"]["why"]))
        doc["clouds"].append(m)
        print(json.dumps(m), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
