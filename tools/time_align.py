#!/usr/bin/env python3
"""The pieces of one ICP iteration, measured -> profiles/align_time.json, and the DESIGN table generated from that file.

    python tools/time_align.py [--iters 8] [--out profiles/align_time.json]
    python tools/time_align.py --table profiles/align_time.json     # prints the markdown table of DESIGN.md 8p (no GPU needed)

One process.  Per shape the ICP's own loop (seggroup_amd/align.py) is walked by hand for `iters` iterations after one warm-up iteration:
sg_rigid_apply, sg_nearest_point_grid and sg_align_moments each between two HIP events, sg_align_solve under the host's clock.  The
question the file answers: do apply + moments cost less than the search they sit beside?  Shapes (moving -> fixed): the 150,000-point
lattice of tools/time_pcseg.py against itself and tests/thin_ref.big_cloud() (1,058,050 points) against itself, the moving copy turned by
3 degrees about the cloud's middle and shifted by 4 cm; max_dist 0.25.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PIECES = ("apply", "search", "moments", "solve")


def spread(v, digits=1):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), digits), min=round(float(v.min()), digits), max=round(float(v.max()), digits))


def measure(label, fixed, iters, max_dist=0.25):
    import torch
    import align_ref
    from seggroup_amd import align, hip
    lib = hip.lib()
    mid = 0.5 * (fixed.min(0) + fixed.max(0)).astype(np.float64)
    to_mid, back = np.eye(4), np.eye(4)
    to_mid[:3, 3], back[:3, 3] = -mid, mid
    P = back @ align_ref.pose(3.0, 0.04) @ to_mid                       # about the cloud's middle
    moving = align_ref.apply(fixed, align_ref.inverse(P))
    u, n = int(moving.shape[0]), int(fixed.shape[0])
    d_mov, d_fix = torch.from_numpy(moving).cuda(), torch.from_numpy(np.ascontiguousarray(fixed, dtype=np.float32)).cuda()
    moved = torch.empty((u, 3), dtype=torch.float32, device="cuda")
    idx, d2 = torch.empty(u, dtype=torch.int64, device="cuda"), torch.empty(u, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(lib.sg_nearest_point_grid_ws_bytes(u, n), lib.sg_align_moments_ws_bytes(u)), dtype=torch.uint8, device="cuda")
    om, of = (0.5 * (c.min(0) + c.max(0)).astype(np.float64) for c in (moving, fixed))
    corners = align.box_corners(moving.min(0), moving.max(0))
    m, T = np.zeros(17), np.eye(4)
    max_d2 = float(np.float32(max_dist * max_dist))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        hip.check(fn())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    rows = []
    for it in range(iters + 1):                                         # iteration 0 is the warm-up: its times are dropped, its pose is kept
        T34 = np.ascontiguousarray(T[:3])
        us = [timed(lambda: lib.sg_rigid_apply(d_mov.data_ptr(), 3, u, T34.ctypes.data, moved.data_ptr(), None)),
              timed(lambda: lib.sg_nearest_point_grid(moved.data_ptr(), 3, u, d_fix.data_ptr(), 3, n, 0.0, idx.data_ptr(), d2.data_ptr(), ws.data_ptr(),
                                                      ws.numel(), None)),
              timed(lambda: lib.sg_align_moments(d_mov.data_ptr(), 3, u, d_fix.data_ptr(), 3, n, idx.data_ptr(), d2.data_ptr(), max_d2, om.ctypes.data,
                                                 of.ctypes.data, m.ctypes.data, ws.data_ptr(), ws.numel(), None))]
        t0 = time.perf_counter()
        T_new = align.solve(m, om, of)
        us.append((time.perf_counter() - t0) * 1e6)
        shift = align.corner_shift(corners, T, T_new)
        T = T_new
        if it:
            rows.append(dict(zip(PIECES, (round(v, 1) for v in us)), inliers=int(m[0]), rms=float("%.4g" % np.sqrt(m[16] / max(m[0], 1))),
                             corner_shift=float("%.3g" % shift)))
    out = dict(shape=label, U=u, N=n, max_dist=max_dist, iterations=rows, pose_error=float("%.3g" % align_ref.corner_shift(corners, T, P)))
    for p in PIECES:
        out[p + "_us"] = spread([r[p] for r in rows])
    out["apply_plus_moments_us"] = spread([r["apply"] + r["moments"] for r in rows])
    out["apply_plus_moments_over_search"] = round(out["apply_plus_moments_us"]["median"] / out["search_us"]["median"], 3)
    out["cheaper_than_the_search_in_every_iteration"] = bool(all(r["apply"] + r["moments"] < r["search"] for r in rows))
    return out


def table(doc):
    cs = doc["shapes"]
    rng = lambda d: f"{d['median']:,.0f} ({d['min']:,.0f} .. {d['max']:,.0f})"          # noqa: E731
    lines = ["| per iteration, µs: median (min .. max) | " + " | ".join(f"{m['U']:,} -> {m['N']:,}" for m in cs) + " |", "|---|" + "---|" * len(cs)]
    for p, what in (("apply", "`sg_rigid_apply`"), ("search", "`sg_nearest_point_grid`"), ("moments", "`sg_align_moments`"),
                    ("solve", "`sg_align_solve` (host)")):
        lines.append(f"| {what} | " + " | ".join(rng(m[p + "_us"]) for m in cs) + " |")
    lines.append("| apply + moments | " + " | ".join(rng(m["apply_plus_moments_us"]) for m in cs) + " |")
    lines.append("| (apply + moments) / search; below the search in every iteration | " + " | ".join(
        f"{m['apply_plus_moments_over_search']:.3f}; {'yes' if m['cheaper_than_the_search_in_every_iteration'] else 'NO'}" for m in cs) + " |")
    lines.append("| iterations timed; corner distance from the true pose after them | " + " | ".join(f"{len(m['iterations'])}; {m['pose_error']:.3g}" for m in cs) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    import thin_ref
    from seggroup_amd import synthetic
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, shapes=[],
               runs="one process, one GPU; one warm-up iteration, then the timed ones; every device call between two HIP events")
    for label, xyz in (("make_room_scan(400, 375)", synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz),
                       ("big_cloud()", thin_ref.big_cloud()[0])):
        m = measure(label, np.ascontiguousarray(xyz[:, :3], dtype=np.float32), a.iters)
        doc["shapes"].append(m)
        print(json.dumps(m), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
