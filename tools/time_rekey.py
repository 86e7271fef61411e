#!/usr/bin/env python3
"""The segment vote, measured -> profiles/rekey_time.json.

    python tools/time_rekey.py [--sizes 400x375,800x625] [--iters 20] [--out profiles/rekey_time.json]

Per lattice (150,000 and 500,000 vertices; 7 x 7 source blocks with synthetic annotations, re-keyed onto 10 x 10 blocks) and per vote of
a scan -- rows = new segments / columns = groups, rows = source segments / columns = new segments -- every stage of sg_segment_vote by HIP
events (sg_segment_vote_set_timing; three warm-up calls, the median of `iters` calls), the host's wall time around the call, and the
NumPy statement of the same vote (tests/rekey_ref.py) on the host beside it.  The figures are recorded, not gated: nothing depends on
them.
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


def time_vote(ids, cols, n_cols, iters):
    import torch
    import rekey_ref
    from seggroup_amd import hip
    lib = hip.lib()
    v = ids.shape[0]
    d_ids, d_cols = torch.from_numpy(ids.astype(np.int32)).cuda(), torch.from_numpy(cols.astype(np.int32)).cuda()
    out = torch.empty((9, v), dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sg_segment_vote_ws_bytes(v), dtype=torch.uint8, device="cuda")
    n_r = C.c_int(0)

    def call():
        hip.check(lib.sg_segment_vote(d_ids.data_ptr(), d_cols.data_ptr(), v, n_cols, *[out[i].data_ptr() for i in range(9)], C.byref(n_r),
                                      ws.data_ptr(), ws.numel(), None))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    rows, wall = [], []
    with hip.stage_timer("segment_vote") as timer:
        for _ in range(iters):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            rows.append(timer.read())
    names = timer.names
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = rekey_ref.vote(ids, cols, n_cols)
        host.append(time.perf_counter() - t0)
    assert np.array_equal(out[4, :n_r.value].cpu().numpy(), ref["winner"]) and np.array_equal(out[0].cpu().numpy(), ref["rank"])
    us = np.median(np.asarray(rows), 0)
    rbits, cbits = max(int(n_r.value) - 1, 0).bit_length(), max(n_cols - 1, 0).bit_length()
    return dict(rows=int(n_r.value), n_cols=int(n_cols), pair_key_bits=rbits + cbits, stages_us={n: round(float(u), 1) for n, u in zip(names, us)},
                event_sum_us=round(float(us.sum()), 1), host_wall_us=round(float(np.median(wall)) * 1e6, 1),
                numpy_statement_on_the_host_us=round(float(np.median(host)) * 1e6, 1))


def measure(w, h, iters):
    import rekey_ref
    from seggroup_amd import synthetic
    scan = synthetic.make_raw_scan(w, h, 11, name="scene0000_00", cell=7, dup_frac=0.0, degenerate_faces=0)
    ann = synthetic.make_annotations(scan, 3, blocks_per_row=-(-w // 7))
    new = synthetic.make_raw_scan(w, h, 11, name="scene0000_00", cell=10, dup_frac=0.0, degenerate_faces=0).seg_indices.astype(np.int64)
    src = scan.seg_indices.astype(np.int64)
    grp = rekey_ref.vertex_groups(src, ann["aggregation"], scan.name)
    n_groups = len(ann["aggregation"]["segGroups"])
    new_rank = np.unique(new, return_inverse=True)[1].reshape(-1)
    return dict(lattice=f"{w}x{h}", V=int(src.shape[0]), groups=n_groups,
                new_segments_over_groups=time_vote(new, grp, n_groups + 1, iters),
                source_segments_over_new_segments=time_vote(src, new_rank, int(new_rank.max()) + 1, iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="400x375,800x625", help="lattices of make_raw_scan: 150,000 and 500,000 vertices")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rekey_time.json"))
    a = ap.parse_args()
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warm_up_calls=3, scans=[])
    for w, h in (tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")):
        doc["scans"].append(measure(w, h, a.iters))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
