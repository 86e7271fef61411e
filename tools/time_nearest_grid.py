#!/usr/bin/env python3
"""The exact grid-indexed nearest point between two clouds against the brute-force search, measured ->
profiles/nearest_grid_time.json, and the DESIGN table generated from that file.

    python tools/time_nearest_grid.py [--iters 5] [--no-large] [--out profiles/nearest_grid_time.json]
    python tools/time_nearest_grid.py --table profiles/nearest_grid_time.json     # prints the markdown table of DESIGN.md 8i (no GPU needed)

One process; per shape the two paths ALTERNATE: a warm-up call each, then `iters` timed repeats each of sg_nearest_point (brute force)
and sg_nearest_point_grid, each call between two HIP events and under the host's wall clock.  The grid's own stages, its ring counts
and its pair-score count come from further repeats with sg_nearest_point_grid_set_timing on (the count costs one atomic per wave, so
those repeats are not the ones the comparison is taken from).  The two index tables are compared wherever both paths run.
Shapes (queries U, candidates N): get_unmapper's own -- 100,000 unsampled vertices of a 500,000-point lattice against 150,000 sampled
ones --, tests/thin_ref.big_cloud() (1,058,050 points) against 150,000 of its points and against every third (352,684), and grid only:
the 4.4 M-point cloud of tools/time_thin.py against 1,000,000 of its points.
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


def spread(v, digits=1):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), digits), min=round(float(v.min()), digits), max=round(float(v.max()), digits))


class Bench:
    def __init__(self, x, y):
        import torch
        from seggroup_amd import hip
        self.hip, self.lib, self.torch = hip, hip.lib(), torch
        self.U, self.N = int(x.shape[0]), int(y.shape[0])
        self.d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        self.d_y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()
        self.idx = {w: torch.empty(self.U, dtype=torch.int64, device="cuda") for w in ("brute", "grid")}
        self.d2 = torch.empty(self.U, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(max(self.lib.sg_nearest_point_grid_ws_bytes(self.U, self.N), self.lib.sg_nearest_point_ws_bytes(self.N)),
                              dtype=torch.uint8, device="cuda")

    def call(self, which):
        """-> (device us between two events, host wall ms)"""
        lib, hip, torch = self.lib, self.hip, self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if which == "brute":
            hip.check(lib.sg_nearest_point(self.d_x.data_ptr(), self.U, self.d_y.data_ptr(), 3, self.N, self.idx[which].data_ptr(),
                                           self.ws.data_ptr(), self.ws.numel(), None))
        else:
            hip.check(lib.sg_nearest_point_grid(self.d_x.data_ptr(), 3, self.U, self.d_y.data_ptr(), 3, self.N, 0.0, self.idx[which].data_ptr(),
                                                self.d2.data_ptr(), self.ws.data_ptr(), self.ws.numel(), None))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e3

    def grid_detail(self, iters):
        from seggroup_amd import prepare
        rows = []
        with self.hip.stage_timer("nearest_point_grid") as timer:
            for _ in range(iters):
                self.call("grid")
                rows.append(timer.read())
            st = prepare.nearest_grid_stats()
        return {nm: round(float(u), 1) for nm, u in zip(timer.names, np.median(np.asarray(rows), 0))}, st


def measure(label, x, y, iters, brute):
    b = Bench(x, y)
    paths = ["brute", "grid"] if brute else ["grid"]
    for w in paths:
        b.call(w)                                               # warm-up
    rec = {w: [] for w in paths}
    for _ in range(iters):
        for w in paths:                                         # alternating
            rec[w].append(b.call(w))
    out = dict(shape=label, U=b.U, N=b.N)
    for w in paths:
        r = np.asarray(rec[w])
        out[w] = dict(device_us=spread(r[:, 0]), wall_ms=spread(r[:, 1], 3))
    stages, st = b.grid_detail(max(iters // 2, 3))
    out["grid"].update(stages_us=stages, stats=st, pair_scores=st["scores"], pair_scores_over_UN=float("%.3g" % (st["scores"] / (float(b.U) * b.N))))
    if brute:
        out["tables_equal"] = bool(b.torch.equal(b.idx["brute"], b.idx["grid"]))
        bd, gd = out["brute"]["device_us"], out["grid"]["device_us"]
        out["brute_over_grid"] = round(bd["median"] / gd["median"], 2)
        out["slowest_grid_below_fastest_brute"] = bool(gd["max"] < bd["min"])
    return out


def table(doc):
    cs = doc["shapes"]
    rng = lambda d: f"{d['median']:,.0f} ({d['min']:,.0f} .. {d['max']:,.0f})"          # noqa: E731
    lines = ["| what | " + " | ".join(f"U = {m['U']:,}, N = {m['N']:,}" for m in cs) + " |", "|---|" + "---|" * len(cs)]
    lines.append("| brute force, device µs: median (min .. max) | " + " | ".join(rng(m["brute"]["device_us"]) if "brute" in m else "-" for m in cs) + " |")
    lines.append("| grid, device µs: median (min .. max) | " + " | ".join(rng(m["grid"]["device_us"]) for m in cs) + " |")
    lines.append("| brute / grid; slowest grid repeat below fastest brute-force repeat | " + " | ".join(
        f"{m['brute_over_grid']:,} x; {'yes' if m['slowest_grid_below_fastest_brute'] else 'NO'}" if "brute" in m else "-" for m in cs) + " |")
    for nm in cs[0]["grid"]["stages_us"]:
        lines.append(f"| grid `{nm}`, µs | " + " | ".join(f"{m['grid']['stages_us'][nm]:,.0f}" for m in cs) + " |")
    lines.append("| cell edge; occupied cells; largest cell | " + " | ".join(
        f"{m['grid']['stats']['cell']:.4g}; {m['grid']['stats']['occupied']:,}; {m['grid']['stats']['largest_cell']:,}" for m in cs) + " |")
    lines.append("| largest ring count; queued queries | " + " | ".join(f"{m['grid']['stats']['max_ring']}; {m['grid']['stats']['fallback']:,}" for m in cs) + " |")
    lines.append("| pair scores evaluated; share of U N | " + " | ".join(f"{m['grid']['pair_scores']:,}; {m['grid']['pair_scores_over_UN']:.2g}" for m in cs) + " |")
    lines.append("| host wall, ms: brute; grid | " + " | ".join(
        (f"{m['brute']['wall_ms']['median']:,.2f}" if "brute" in m else "-") + f"; {m['grid']['wall_ms']['median']:,.2f}" for m in cs) + " |")
    lines.append("| tables equal | " + " | ".join(("yes" if m["tables_equal"] else "NO") if "tables_equal" in m else "-" for m in cs) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-large", action="store_true", help="leave out the 4.4 M-point shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_grid_time.json"))
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
    doc = dict(device=torch.cuda.get_device_name(0), iters=iters, shapes=[],
               runs="one process, one GPU; brute force and grid alternate; a warm-up call each, then the timed repeats")
    mid = synthetic.make_room_scan(800, 625, 11, jitter=5e-4, name="scene0000_00").xyz
    perm = np.random.RandomState(21).permutation(mid.shape[0])
    big = thin_ref.big_cloud()[0]
    bperm = np.random.RandomState(22).permutation(big.shape[0])
    jobs = [("100,000 unsampled vertices of make_room_scan(800, 625) against 150,000 sampled ones", mid[perm[150000:250000]], mid[perm[:150000]], True),
            ("big_cloud() against 150,000 of its points", big, big[np.sort(bperm[:150000])], True),
            ("big_cloud() against big_cloud()[::3]", big, big[::3], True)]
    if not a.no_large:
        jobs.append(("make_room_cloud(1150, 0.0025, 2.5e-5, seed=9) against 1,000,000 of its points", None, None, False))
    for label, x, y, brute in jobs:
        if x is None:
            x = pcseg_ref.make_room_cloud(1150, 0.0025, 2.5e-5, seed=9)[0]
            y = x[np.sort(np.random.RandomState(23).permutation(x.shape[0])[:1000000])]
        m = measure(label, x, y, iters, brute)
        doc["shapes"].append(m)
        print(json.dumps(m), flush=True)
        del x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
