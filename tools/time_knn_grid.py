#!/usr/bin/env python3
"""The exact grid-indexed kNN against the brute-force kNN, measured -> profiles/knn_grid_time.json, and the DESIGN table
generated from that file.

    python tools/time_knn_grid.py [--iters 5] [--no-large] [--out profiles/knn_grid_time.json]
    python tools/time_knn_grid.py --table profiles/knn_grid_time.json     # prints the markdown table of DESIGN.md 8h (no GPU needed)

One process; per cloud the two paths ALTERNATE: a warm-up call each, then `iters` timed repeats each of sg_pcseg_edges (brute force) and
sg_pcseg_edges_indexed (grid), whose `knn` stage is taken by HIP events (sg_pcseg_set_timing) and whose call by the host's wall clock.
The grid's own stages and its pair-score count come from further repeats with sg_pointcloud_knn_grid_set_timing on (the count costs one
atomic per block, so those repeats are not the ones the ratio is taken from).  The two tables are compared wherever both paths run.
Clouds: the lattices of tools/time_pcseg.py (150,000 and 500,000 points; k = 5, 10, 20 on the first), the first 1,000,000 points of
tests/thin_ref.big_cloud(), and grid only: the whole big_cloud() and the 4.4 M-point cloud of tools/time_thin.py.  Last, a sweep of the
target occupancy and of the ring limit on the 150,000-point lattice and on the 1,000,000 points.
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


class Bench:
    def __init__(self, xyz, k):
        import torch
        from seggroup_amd import hip
        self.hip, self.lib, self.torch = hip, hip.lib(), torch
        self.N, self.k = xyz.shape[0], k
        n, lib = self.N, self.lib
        self.brute_ok = n <= (1 << 20)
        self.d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).cuda()
        self.nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        self.edges = torch.empty((n * k, 2), dtype=torch.int32, device="cuda")
        self.wts = torch.empty(n * k, dtype=torch.float32, device="cuda")
        self.knn = {w: torch.empty((n, k + 1), dtype=torch.int32, device="cuda") for w in ("brute", "grid") if w == "grid" or self.brute_ok}
        self.ws = torch.empty(lib.sg_pcseg_ws_bytes_indexed(n, k, hip.KNN_GRID), dtype=torch.uint8, device="cuda")
        self.n_e = C.c_int(0)

    def call(self, which):
        lib, hip = self.lib, self.hip
        a = (self.d_xyz.data_ptr(), self.N, self.k, None)
        b = (self.knn[which].data_ptr(), self.nrm.data_ptr(), self.edges.data_ptr(), self.wts.data_ptr(), C.byref(self.n_e), self.ws.data_ptr(),
             self.ws.numel(), None)
        t0 = time.perf_counter()
        hip.check(lib.sg_pcseg_edges(*a, *b) if which == "brute" else lib.sg_pcseg_edges_indexed(*a, hip.KNN_GRID, 0.0, *b))
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(self, which, timer):
        """-> (knn stage us, all stages us, wall ms); `timer`: the pcseg family's, on"""
        wall = self.call(which)
        us = timer.read()
        return us[timer.names.index("knn")], float(sum(us)), wall * 1e3

    def grid_detail(self, iters):
        from seggroup_amd import oversegment
        rows = []
        with self.hip.stage_timer("pointcloud_knn_grid") as timer:
            for _ in range(iters):
                self.call("grid")
                rows.append(timer.read())
            st = oversegment.knn_grid_stats()
        us = np.median(np.asarray(rows), 0)
        return {nm: round(float(u), 1) for nm, u in zip(timer.names, us)}, st


def spread(v, digits=1):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), digits), min=round(float(v.min()), digits), max=round(float(v.max()), digits))


def measure(label, xyz, k, iters):
    b = Bench(xyz, k)
    lib, hip = b.lib, b.hip
    paths = ["brute", "grid"] if b.brute_ok else ["grid"]
    for w in paths:
        b.call(w)                                               # warm-up
    rec = {w: [] for w in paths}
    with hip.stage_timer("pcseg") as timer:
        for _ in range(iters):
            for w in paths:                                     # alternating
                rec[w].append(b.timed(w, timer))
    out = dict(cloud=label, N=b.N, k=k, E=int(b.n_e.value))
    for w in paths:
        r = np.asarray(rec[w])
        out[w] = dict(knn_stage_us=spread(r[:, 0]), device_stages_us=spread(r[:, 1]), sg_pcseg_edges_wall_ms=spread(r[:, 2], 3))
    stages, st = b.grid_detail(max(iters // 2, 3))
    out["grid"]["stages_us"] = stages
    out["grid"]["stats"] = st
    out["grid"]["pair_scores"] = st["scores"]
    out["grid"]["pair_scores_over_N2"] = float("%.3g" % (st["scores"] / float(b.N) ** 2))
    if b.brute_ok:
        out["tables_equal"] = bool(b.torch.equal(b.knn["brute"], b.knn["grid"]))
        bk, gk = out["brute"]["knn_stage_us"], out["grid"]["knn_stage_us"]
        out["knn_brute_over_grid"] = round(bk["median"] / gk["median"], 1)
        out["gap_us"] = round(bk["min"] - gk["max"], 1)                         # the slowest grid repeat against the fastest brute repeat
        out["brute_spread_us"] = round(bk["max"] - bk["min"], 1)
        out["grid_is_faster_beyond_the_spread"] = bool(out["gap_us"] > out["brute_spread_us"])
        out["edges_wall_brute_over_grid"] = round(out["brute"]["sg_pcseg_edges_wall_ms"]["median"] / out["grid"]["sg_pcseg_edges_wall_ms"]["median"], 2)
    return out, b


def sweep(b, iters):
    """the grid's knn stage against the target occupancy (at the default ring limit) and the ring limit (at the default occupancy)"""
    lib, hip = b.lib, b.hip
    from seggroup_amd import oversegment
    rows = []
    with hip.stage_timer("pcseg") as timer:
        for target, limit in [(t, 0) for t in (8, 16, 32, 48, 64, 96, 160)] + [(0, r) for r in (1, 2, 4, 8, 16)]:
            hip.check(lib.sg_pointcloud_knn_grid_set_tuning(target, limit))
            b.call("grid")
            us = [b.timed("grid", timer)[0] for _ in range(iters)]
            st = oversegment.knn_grid_stats()
            rows.append(dict(target_occupancy=target or "default", ring_limit=limit or "default", knn_stage_us=spread(us),
                             cell=round(st["cell"], 5), occupied=st["occupied"], largest_cell=st["largest_cell"], max_ring=st["max_ring"],
                             fallback=st["fallback"]))
        hip.check(lib.sg_pointcloud_knn_grid_set_tuning(0, 0))
    return rows


def table(doc):
    cs = doc["clouds"]
    head = "| what | " + " | ".join(f"{m['N']:,} points, k = {m['k']}" for m in cs) + " |"
    lines = [head, "|---|" + "---|" * len(cs)]
    lines.append("| brute-force `knn` stage, µs: median (min .. max) | " + " | ".join(
        "-" if "brute" not in m else f"{m['brute']['knn_stage_us']['median']:,.0f} ({m['brute']['knn_stage_us']['min']:,.0f} .. {m['brute']['knn_stage_us']['max']:,.0f})"
        for m in cs) + " |")
    lines.append("| grid `knn` stage, µs: median (min .. max) | " + " | ".join(
        f"{m['grid']['knn_stage_us']['median']:,.0f} ({m['grid']['knn_stage_us']['min']:,.0f} .. {m['grid']['knn_stage_us']['max']:,.0f})" for m in cs) + " |")
    lines.append("| brute / grid; faster beyond the brute-force spread | " + " | ".join(
        "-" if "brute" not in m else f"{m['knn_brute_over_grid']:,} x; {'yes' if m['grid_is_faster_beyond_the_spread'] else 'NO'}" for m in cs) + " |")
    for nm in cs[0]["grid"]["stages_us"]:
        lines.append(f"| grid `{nm}`, µs | " + " | ".join(f"{m['grid']['stages_us'][nm]:,.0f}" for m in cs) + " |")
    lines.append("| cell edge; occupied cells; largest cell | " + " | ".join(
        f"{m['grid']['stats']['cell']:.4g}; {m['grid']['stats']['occupied']:,}; {m['grid']['stats']['largest_cell']:,}" for m in cs) + " |")
    lines.append("| largest ring count; queries finished by the fallback | " + " | ".join(
        f"{m['grid']['stats']['max_ring']}; {m['grid']['stats']['fallback']:,}" for m in cs) + " |")
    lines.append("| pair scores evaluated; share of N^2 | " + " | ".join(f"{m['grid']['pair_scores']:,}; {m['grid']['pair_scores_over_N2']:.2g}" for m in cs) + " |")
    lines.append("| `sg_pcseg_edges` host wall, ms: brute; grid | " + " | ".join(
        (f"{m['brute']['sg_pcseg_edges_wall_ms']['median']:,.2f}" if "brute" in m else "-") + f"; {m['grid']['sg_pcseg_edges_wall_ms']['median']:,.2f}" for m in cs) + " |")
    lines.append("| tables equal | " + " | ".join(("yes" if m["tables_equal"] else "NO") if "tables_equal" in m else "-" for m in cs) + " |")
    for s in doc.get("sweeps", []):
        lines += ["", f"Sweep at {s['N']:,} points (grid `knn` stage, median µs): " + "; ".join(
            f"occupancy {r['target_occupancy']} / limit {r['ring_limit']}: {r['knn_stage_us']['median']:,.0f} (cell {r['cell']:.3g}, fallback {r['fallback']:,})"
            for r in s["rows"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-large", action="store_true", help="leave out the clouds above 2^20 points")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_grid_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import pcseg_ref
    import thin_ref
    from seggroup_amd import synthetic
    iters = max(a.iters, 5)
    doc = dict(device=torch.cuda.get_device_name(0), iters=iters, clouds=[], sweeps=[],
               runs="one process, one GPU; brute force and grid alternate; a warm-up call each, then the timed repeats")
    small = synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz
    mid = synthetic.make_room_scan(800, 625, 11, jitter=5e-4, name="scene0000_00").xyz
    big = thin_ref.big_cloud()[0]
    jobs = [("make_room_scan(400, 375)", small, 10, True), ("make_room_scan(400, 375)", small, 5, False), ("make_room_scan(400, 375)", small, 20, False),
            ("make_room_scan(800, 625)", mid, 10, False), ("big_cloud()[:1000000]", big[:1000000], 10, True)]
    if not a.no_large:
        jobs += [("big_cloud()", big, 10, False), ("make_room_cloud(1150, 0.0025, 2.5e-5, seed=9)", None, 10, False)]
    for label, xyz, k, swept in jobs:
        if xyz is None:
            xyz = pcseg_ref.make_room_cloud(1150, 0.0025, 2.5e-5, seed=9)[0]
        m, b = measure(label, xyz, k, iters)
        doc["clouds"].append(m)
        print(json.dumps(m), flush=True)
        if swept:
            s = dict(cloud=label, N=m["N"], k=k, rows=sweep(b, 3))
            doc["sweeps"].append(s)
            print(json.dumps(s), flush=True)
        del b, xyz
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
