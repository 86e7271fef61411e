#!/usr/bin/env python3
"""The two-cloud k-nearest search and the vote over its rows, measured -> profiles/knn_cross_time.json, and the DESIGN
table generated from that file.

    python tools/time_knn_cross.py [--iters 5] [--out profiles/knn_cross_time.json]
    python tools/time_knn_cross.py --table profiles/knn_cross_time.json     # prints the markdown table of DESIGN.md 8o (no GPU needed)

One process; per pair a warm-up call of every path, then `iters` repeats with the family's stage timer on, the paths ALTERNATING inside a
repeat: sg_cloud_knn_cross_grid at k = 5, 10, 20, sg_nearest_point_grid on the same pair, sg_pointcloud_knn_grid on the candidate cloud
alone at the same k, and sg_knn_vote over the rows just written (between two HIP events).  Pairs: the queries are
synthetic.make_room_scan(400, 375) (150,000 points), make_room_scan(800, 625) (500,000) and tests/thin_ref.big_cloud() (1,058,050); the
candidates are their [::2] rows, labelled by their 0.25-unit block with 15 % of the labels redrawn at random.  The comparison DESIGN.md
8o quotes is the `search` stage PER QUERY of the cross search against the self-kNN's at the nearest list length (5 against 6, 10 against
11, 20 against 21): the walk is the same code; the cross search's stage also holds the queries' binning and sort.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KS = (5, 10, 20)


def spread(v, digits=1):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), digits), min=round(float(v.min()), digits), max=round(float(v.max()), digits))


class Bench:
    def __init__(self, x, y, labels):
        import torch
        from seggroup_amd import hip
        self.hip, self.lib, self.torch = hip, hip.lib(), torch
        lib = self.lib
        self.U, self.N = int(x.shape[0]), int(y.shape[0])
        self.d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        self.d_y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()
        self.d_lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
        self.knn = torch.empty((self.U, max(KS)), dtype=torch.int32, device="cuda")
        self.d2 = torch.empty((self.U, max(KS)), dtype=torch.float32, device="cuda")
        self.self_knn = torch.empty((self.N, max(KS) + 1), dtype=torch.int32, device="cuda")
        self.idx = torch.empty(self.U, dtype=torch.int64, device="cuda")
        self.out = torch.empty((4, self.U), dtype=torch.int32, device="cuda")
        need = max([lib.sg_cloud_knn_cross_grid_ws_bytes(self.U, self.N, k) for k in KS] + [lib.sg_nearest_point_grid_ws_bytes(self.U, self.N)] +
                   [lib.sg_pointcloud_knn_grid_ws_bytes(self.N, k) for k in KS])
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def cross(self, k):
        self.hip.check(self.lib.sg_cloud_knn_cross_grid(self.d_x.data_ptr(), 3, self.U, self.d_y.data_ptr(), 3, self.N, k, 0.0, self.knn.data_ptr(),
                                                        self.d2.data_ptr(), self.ws.data_ptr(), self.ws.numel(), None))

    def nearest(self):
        self.hip.check(self.lib.sg_nearest_point_grid(self.d_x.data_ptr(), 3, self.U, self.d_y.data_ptr(), 3, self.N, 0.0, self.idx.data_ptr(),
                                                      self.d2.data_ptr(), self.ws.data_ptr(), self.ws.numel(), None))

    def self_search(self, k):
        self.hip.check(self.lib.sg_pointcloud_knn_grid(self.d_y.data_ptr(), 3, self.N, k, 0.0, self.self_knn.data_ptr(), self.ws.data_ptr(),
                                                       self.ws.numel(), None))

    def vote(self, k):
        """-> device us between two events; the rows are the last cross(k)'s"""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p = [self.out[i].data_ptr() for i in range(4)]
        torch.cuda.synchronize()
        e0.record()
        self.hip.check(self.lib.sg_knn_vote(self.knn.data_ptr(), self.U, k, self.d_lab.data_ptr(), self.N, *p, None))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3


def block_labels(y, seed=7):
    """the candidates' 0.25-unit blocks as labels, 15 % of them redrawn among the labels present (the vote's time does not depend on them)"""
    b = np.floor((y - y.min(0)) / np.float32(0.25)).astype(np.int64)
    lab = ((b[:, 2] * 1024 + b[:, 1]) * 1024 + b[:, 0]).astype(np.int32)
    rng = np.random.default_rng(seed)
    noisy = rng.random(y.shape[0]) < 0.15
    present = np.unique(lab)
    lab[noisy] = present[rng.integers(0, present.shape[0], int(noisy.sum()))]
    return lab


def _stages(names, rows):
    return {nm: round(float(u), 1) for nm, u in zip(names, np.median(np.asarray(rows), 0))}


def measure(label, x, y, labels, iters):
    from seggroup_amd import oversegment, prepare
    b = Bench(x, y, labels)
    hip = b.hip
    out = dict(pair=label, U=b.U, N=b.N, k={})
    b.nearest()
    for k in KS:
        b.cross(k), b.self_search(k), b.vote(k)                 # warm-up
    near_rows = []
    for k in KS:
        rows = {"cross": [], "self": []}
        votes = []
        for _ in range(iters):
            with hip.stage_timer("cloud_knn_cross_grid") as t:
                b.cross(k)
                rows["cross"].append(t.read())
                cross_names, cross_stats = t.names, prepare.knn_cross_stats()
            votes.append(b.vote(k))
            with hip.stage_timer("pointcloud_knn_grid") as t:
                b.self_search(k)
                rows["self"].append(t.read())
                self_names, self_stats = t.names, oversegment.knn_grid_stats()
            with hip.stage_timer("nearest_point_grid") as t:
                b.nearest()
                near_rows.append(t.read())
                near_names, near_stats = t.names, prepare.nearest_grid_stats()
        cross, own = _stages(cross_names, rows["cross"]), _stages(self_names, rows["self"])
        per_q, per_p = cross["search"] * 1e3 / b.U, own["search"] * 1e3 / b.N
        out["k"][str(k)] = dict(cross=dict(stages_us=cross, all_stages_us=round(sum(cross.values()), 1), stats=cross_stats),
                                self_knn=dict(list_length=k + 1, stages_us=own, all_stages_us=round(sum(own.values()), 1), stats=self_stats),
                                vote_us=spread(votes),
                                search_ns_per_query=dict(cross=round(per_q, 2), self_knn=round(per_p, 2), cross_over_self=round(per_q / per_p, 3)))
    near = _stages(near_names, near_rows)
    out["nearest_point_grid"] = dict(stages_us=near, all_stages_us=round(sum(near.values()), 1), stats=near_stats,
                                     search_ns_per_query=round(near["search"] * 1e3 / b.U, 2))
    return out


def table(doc):
    ps = doc["pairs"]
    cols = [(m, k) for m in ps for k in sorted(m["k"], key=int)]
    lines = ["| what | " + " | ".join(f"U = {m['U']:,}, k = {k}" for m, k in cols) + " |", "|---|" + "---|" * len(cols)]
    g = lambda m, k: m["k"][k]                                                                              # noqa: E731
    lines.append("| cross, all stages, µs | " + " | ".join(f"{g(m, k)['cross']['all_stages_us']:,.0f}" for m, k in cols) + " |")
    lines.append("| cross `search`, µs | " + " | ".join(f"{g(m, k)['cross']['stages_us']['search']:,.0f}" for m, k in cols) + " |")
    lines.append("| cross `fallback` (queue and d2), µs | " + " | ".join(f"{g(m, k)['cross']['stages_us']['fallback']:,.0f}" for m, k in cols) + " |")
    lines.append("| self-kNN of the candidates at k + 1, `search`, µs | " + " | ".join(f"{g(m, k)['self_knn']['stages_us']['search']:,.0f}" for m, k in cols) + " |")
    lines.append("| `search` per query, ns: cross; self; cross / self | " + " | ".join(
        "{cross:,.1f}; {self_knn:,.1f}; {cross_over_self:.2f}".format(**g(m, k)["search_ns_per_query"]) for m, k in cols) + " |")
    lines.append("| nearest point (one entry), `search`, µs | " + " | ".join(f"{m['nearest_point_grid']['stages_us']['search']:,.0f}" for m, k in cols) + " |")
    lines.append("| cross: largest ring count; queued queries | " + " | ".join(
        f"{g(m, k)['cross']['stats']['max_ring']}; {g(m, k)['cross']['stats']['fallback']:,}" for m, k in cols) + " |")
    lines.append("| cross: pair scores per query | " + " | ".join(f"{g(m, k)['cross']['stats']['scores'] / m['U']:,.0f}" for m, k in cols) + " |")
    lines.append("| vote, µs: median (min .. max) | " + " | ".join(
        "{median:,.0f} ({min:,.0f} .. {max:,.0f})".format(**g(m, k)["vote_us"]) for m, k in cols) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_cross_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import thin_ref
    from seggroup_amd import synthetic
    iters = max(a.iters, 3)
    doc = dict(device=torch.cuda.get_device_name(0), iters=iters, pairs=[],
               runs="one process, one GPU; the paths alternate inside a repeat; a warm-up call each; stage times by events with the family's "
                    "timer on (the pair-score count costs one atomic per wave)")
    jobs = [("make_room_scan(400, 375) against its [::2]", lambda: synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz),
            ("make_room_scan(800, 625) against its [::2]", lambda: synthetic.make_room_scan(800, 625, 11, jitter=5e-4, name="scene0000_00").xyz),
            ("big_cloud() against its [::2]", lambda: thin_ref.big_cloud()[0])]
    for label, make in jobs:
        x = np.ascontiguousarray(make()[:, :3], dtype=np.float32)
        y = np.ascontiguousarray(x[::2])
        m = measure(label, x, y, block_labels(y), iters)
        doc["pairs"].append(m)
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
