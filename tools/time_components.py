#!/usr/bin/env python3
"""Connected components, measured -> profiles/components_time.json, and the DESIGN table generated from that file.

    python tools/time_components.py [--repeats 5] [--out profiles/components_time.json]
    python tools/time_components.py --table profiles/components_time.json      # prints the markdown table of DESIGN.md 8j (no GPU needed)

Per graph, all taken in one run: the device call between two events on its stream after a warm-up, the median (min .. max) of the repeats;
every stage by the library's own events (sg_components_set_timing) from three further repeats; and the host alternative a user has without
this module for the same answer -- scipy.sparse.csgraph.connected_components on the same pairs plus the relabelling to the lowest index
(the NumPy statement of tests/components_ref.py where scipy is missing; `host` says which), once, on the same host.  The pair list handed
to the host is built outside its clock.  Pairs per second and the bytes of the pair source per second are taken at the device median.
The outputs of the two are compared while at it.  The graphs: the 150,000-vertex room mesh of tests/overseg_ref.py through its faces and
through its unique edge list, and tests/thin_ref.py's 1,058,050 points with the grid index's kNN table (k = 10), cut and uncut.
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

NOT_MEASURED = ["the number of CAS retries (no counter is compiled in)", "several streams in flight", "graphs near SG_MAX_CLOUD_POINTS",
                "edge lists of 2^29 rows and more, where the offsets pass 2^31", "the label filter's cost"]


def host_answer(num_vertices, a, b):
    """-> (comp, which, seconds)"""
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        import components_ref as R
        t0 = time.perf_counter()
        comp, _, _ = R.components(num_vertices, a, b)
        return comp, "the NumPy statement (scipy is not importable)", time.perf_counter() - t0
    t0 = time.perf_counter()
    g = sp.coo_matrix((np.ones(a.shape[0], np.int8), (a, b)), shape=(num_vertices, num_vertices))
    count, lab = connected_components(g, directed=False)
    low = np.full(count, num_vertices, np.int64)
    np.minimum.at(low, lab, np.arange(num_vertices))
    comp = low[lab].astype(np.int32)
    return comp, "scipy.sparse.csgraph.connected_components + lowest-index relabelling", time.perf_counter() - t0


def measure(label, num_vertices, launch, pairs, source_bytes, host_pairs, repeats):
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    comp = torch.empty(num_vertices, dtype=torch.int32, device="cuda")
    size = torch.empty(num_vertices, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sg_components_ws_bytes(num_vertices), dtype=torch.uint8, device="cuda")
    c = C.c_int(0)
    tail = (None, comp.data_ptr(), size.data_ptr(), C.byref(c), ws.data_ptr(), ws.numel(), None)
    launch(lib, tail)                                           # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(lib, tail)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rows = []
    with hip.stage_timer("components") as timer:
        for _ in range(3):
            launch(lib, tail)
            rows.append(timer.read())
    names = timer.names
    us =np.median(np.asarray(rows), 0)
    a, b = host_pairs()
    want, which, host_s = host_answer(num_vertices, a, b)
    got = comp.cpu().numpy()
    med = float(np.median(ms))
    sizes = np.sort(np.bincount(got)[np.unique(got)])[::-1]
    return dict(graph=label, V=int(num_vertices), pairs=int(pairs), source_bytes=int(source_bytes), C=int(c.value), largest_sizes=sizes[:5].tolist(),
                device_ms=dict(median=round(med, 4), min=round(float(min(ms)), 4), max=round(float(max(ms)), 4), repeats=repeats),
                stages_us={nm: round(float(u), 1) for nm, u in zip(names, us)}, pairs_per_s=round(pairs / (med * 1e-3)),
                source_gb_per_s=round(source_bytes / (med * 1e-3) / 1e9, 2), host=which, host_ms=round(host_s * 1e3, 1),
                host_over_device=round(host_s * 1e3 / med, 1), equal_to_the_host_answer=bool(np.array_equal(got, want) and c.value == np.unique(want).shape[0]),
                workspace_bytes=int(ws.numel()))


def table(doc):
    gs = doc["graphs"]
    lines = ["| what | " + " | ".join(g["graph"] for g in gs) + " |", "|---|" + "---|" * len(gs)]
    lines.append("| vertices; pairs; bytes of the pair source | " + " | ".join(f"{g['V']:,}; {g['pairs']:,}; {g['source_bytes']:,}" for g in gs) + " |")
    lines.append("| components; the largest | " + " | ".join(f"{g['C']:,}; {', '.join(format(s, ',') for s in g['largest_sizes'][:3])}" for g in gs) + " |")
    lines.append(f"| device call between events, ms: median (min .. max) of {gs[0]['device_ms']['repeats']} | " + " | ".join(
        f"{g['device_ms']['median']:.3f} ({g['device_ms']['min']:.3f} .. {g['device_ms']['max']:.3f})" for g in gs) + " |")
    for nm in gs[0]["stages_us"]:
        lines.append(f"| `{nm}` (the library's events), µs | " + " | ".join(f"{g['stages_us'][nm]:,.1f}" for g in gs) + " |")
    lines.append("| pairs per second; GB/s of the pair source | " + " | ".join(f"{g['pairs_per_s']:.3g}; {g['source_gb_per_s']:,}" for g in gs) + " |")
    lines.append("| the host alternative, ms (ratio to the device median) | " + " | ".join(f"{g['host_ms']:,} ({g['host_over_device']:,} x)" for g in gs) + " |")
    lines.append("| outputs equal to the host's | " + " | ".join("yes" if g["equal_to_the_host_answer"] else "NO" for g in gs) + " |")
    lines += ["", "Host alternative: " + "; ".join(sorted({g["host"] for g in gs})) + ".  Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cut", type=float, default=0.004, help="max_edge of the cut kNN graph of the large cloud")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import components_ref as R
    import overseg_ref
    import thin_ref
    from seggroup_amd import hip, prepare
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream; the host figure is one run", not_measured=NOT_MEASURED, graphs=[])

    xyz, faces = overseg_ref.case_meshes(include_large=True)["room_150k"]
    v = xyz.shape[0]
    edges = overseg_ref.mesh_edges(faces, v)
    d_f, d_e = torch.from_numpy(faces).cuda(), torch.from_numpy(edges).cuda()
    jobs = [("room mesh, faces", v, lambda lib, tail: hip.check(lib.sg_components_faces(d_f.data_ptr(), faces.shape[0], v, *tail)),
             3 * faces.shape[0], faces.nbytes, lambda: R.pairs_from_faces(faces, v)),
            ("room mesh, unique edges", v, lambda lib, tail: hip.check(lib.sg_components_edges(d_e.data_ptr(), edges.shape[0], v, *tail)),
             edges.shape[0], edges.nbytes, lambda: R.pairs_from_edges(edges, v))]
    big, _ = thin_ref.big_cloud()
    n = big.shape[0]
    d_x = torch.from_numpy(big).cuda()
    d_t = prepare.pointcloud_knn(d_x, 10, device="cuda:0", index="grid")
    table_host = d_t.cpu().numpy()
    row = int(d_t.shape[1])
    for cut, name in ((float("inf"), "1,058,050 points, kNN-10, no cut"), (a.cut, "1,058,050 points, kNN-10, cut at %g" % a.cut)):
        jobs.append((name, n, (lambda lib, tail, cut=cut: hip.check(lib.sg_components_knn(d_x.data_ptr(), 3, d_t.data_ptr(), n, row, cut, *tail))),
                     n * (row - 1), table_host.nbytes + big.nbytes, (lambda cut=cut: R.pairs_from_knn(big, table_host, cut))))
    for job in jobs:
        m = measure(*job, a.repeats)
        doc["graphs"].append(m)
        print(json.dumps(m), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
