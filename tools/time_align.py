#!/usr/bin/env python3
"""The pieces of one ICP iteration, measured -> profiles/align_time.json, and the DESIGN table generated from that file.

    python tools/time_align.py [--iters 8] [--out profiles/align_time.json]
    python tools/time_align.py --table profiles/align_time.json     # prints the markdown table of DESIGN.md 8p (no GPU needed)
    python tools/time_align.py --plane [--out profiles/align_plane_time.json]      # the point-to-plane leg
    python tools/time_align.py --plane-table profiles/align_plane_time.json        # prints the markdown table of DESIGN.md 8q

One process.  Per shape the ICP's own loop (seggroup_amd/align.py) is walked by hand for `iters` iterations after one warm-up iteration:
sg_rigid_apply, sg_nearest_point_grid and sg_align_moments each between two HIP events, sg_align_solve under the host's clock.  The
question the file answers: do apply + moments cost less than the search they sit beside?  Shapes (moving -> fixed): the 150,000-point
lattice of tools/time_pcseg.py against itself and tests/thin_ref.big_cloud() (1,058,050 points) against itself, the moving copy turned by
3 degrees about the cloud's middle and shifted by 4 cm; max_dist 0.25.

--plane: the same two shapes, the same process rules, both metrics walked by hand until align.icp's own stopping rules say `converged`
(50 searches at most).  In the plane loop every iteration also times sg_align_moments on the same pairs, so that the two moment kernels
and the search stand side by side; per metric the file holds the searches, the device time summed over every call until the stop, the
corner distance from the true pose at the end and after every iteration.  The fixed cloud's normals are the lattice's face normals (oversegment.vertex_normals)
and, for big_cloud() -- 50 copies of one room within 4 mm, where a 10-neighbour covariance sees only the copies' jitter --, the
least-squares normal of each of its 8 labelled planes, passed as a caller's normals would be.
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


def plane_normals(xyz, plane):
    """per labelled plane the least-squares normal of its points -> float32 [N,3]"""
    out = np.zeros(xyz.shape, np.float32)
    for p in np.unique(plane):
        q = xyz[plane == p].astype(np.float64)
        q -= q.mean(0)
        out[plane == p] = np.linalg.eigh(q.T @ q)[1][:, 0].astype(np.float32)
    return out


def measure_plane(label, fixed, normals, how, max_iter=50, max_dist=0.25):
    """both metrics on one shape, each until align.icp's own rules stop it -> the shape's entry of align_plane_time.json"""
    import torch
    import align_ref
    from seggroup_amd import align, hip
    lib = hip.lib()
    flo, fhi = fixed.min(0).astype(np.float64), fixed.max(0).astype(np.float64)
    mid = 0.5 * (flo + fhi)
    to_mid, back = np.eye(4), np.eye(4)
    to_mid[:3, 3], back[:3, 3] = -mid, mid
    P = back @ align_ref.pose(3.0, 0.04) @ to_mid                       # about the cloud's middle
    moving = align_ref.apply(fixed, align_ref.inverse(P))
    u, n = int(moving.shape[0]), int(fixed.shape[0])
    d_mov, d_fix = torch.from_numpy(moving).cuda(), torch.from_numpy(np.ascontiguousarray(fixed, dtype=np.float32)).cuda()
    d_nrm = normals.cuda().contiguous() if hasattr(normals, "cuda") else torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32)).cuda()
    moved = torch.empty((u, 3), dtype=torch.float32, device="cuda")
    idx, d2 = torch.empty(u, dtype=torch.int64, device="cuda"), torch.empty(u, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(lib.sg_nearest_point_grid_ws_bytes(u, n), lib.sg_align_moments_ws_bytes(u), lib.sg_align_plane_moments_ws_bytes(u)),
                     dtype=torch.uint8, device="cuda")
    mlo, mhi = moving.min(0).astype(np.float64), moving.max(0).astype(np.float64)
    om, of = 0.5 * (mlo + mhi), mid
    length = 0.5 * float(np.sqrt(((fhi - flo) ** 2).sum()))
    corners = align.box_corners(mlo, mhi)
    min_delta = 2.0 ** -23 * float(max(np.abs(v).max() for v in (mlo, mhi, flo, fhi)))
    max_d2 = float(np.float32(max_dist * max_dist))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        hip.check(fn())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def walk(metric):
        T, rows, prev, converged = np.eye(4), [], None, False
        m17, m31 = np.zeros(17), np.zeros(31)
        for _ in range(max_iter):
            T34 = np.ascontiguousarray(T[:3])
            row = dict(apply=timed(lambda: lib.sg_rigid_apply(d_mov.data_ptr(), 3, u, T34.ctypes.data, moved.data_ptr(), None)),
                       search=timed(lambda: lib.sg_nearest_point_grid(moved.data_ptr(), 3, u, d_fix.data_ptr(), 3, n, 0.0, idx.data_ptr(), d2.data_ptr(),
                                                                      ws.data_ptr(), ws.numel(), None)),
                       moments=timed(lambda: lib.sg_align_moments(d_mov.data_ptr(), 3, u, d_fix.data_ptr(), 3, n, idx.data_ptr(), d2.data_ptr(), max_d2,
                                                                  om.ctypes.data, of.ctypes.data, m17.ctypes.data, ws.data_ptr(), ws.numel(), None)))
            if metric == "plane":
                row["plane_moments"] = timed(lambda: lib.sg_align_plane_moments(d_mov.data_ptr(), 3, u, T34.ctypes.data, d_fix.data_ptr(), 3, n,
                                                                                d_nrm.data_ptr(), int(d_nrm.shape[1]), idx.data_ptr(), d2.data_ptr(),
                                                                                max_d2, of.ctypes.data, m31.ctypes.data, ws.data_ptr(), ws.numel(), None))
                t0 = time.perf_counter()
                T_new = align.plane_solve(m31, T, of, length)
                row.update(solve=(time.perf_counter() - t0) * 1e6, inliers=int(m31[0]), skipped=int(m31[1]),
                           plane_rms=float("%.4g" % np.sqrt(m31[29] / max(m31[0], 1))), rms=float("%.4g" % np.sqrt(m31[30] / max(m31[0], 1))))
            else:
                inlier = d2 <= max_d2
                same = prev is not None and bool(torch.equal(idx, prev[0])) and bool(torch.equal(inlier, prev[1]))
                prev = (idx.clone(), inlier)
                row.update(inliers=int(m17[0]), rms=float("%.4g" % np.sqrt(m17[16] / max(m17[0], 1))))
                if same:
                    rows.append(row)
                    converged = "fixed point"
                    break
                t0 = time.perf_counter()
                T_new = align.solve(m17, om, of)
                row["solve"] = (time.perf_counter() - t0) * 1e6
            shift = align.corner_shift(corners, T, T_new)
            row["corner_shift"] = float("%.3g" % shift)
            T = T_new
            row["pose_error"] = float("%.3g" % align_ref.corner_shift(corners, T, P))        # after this iteration's update
            rows.append(row)
            if shift <= min_delta:
                converged = "min_delta"
                break
        used = ("apply", "search", "plane_moments") if metric == "plane" else ("apply", "search", "moments")    # what the metric's own loop runs
        for r in rows:
            for k in ("apply", "search", "moments", "plane_moments", "solve"):
                if k in r:
                    r[k] = round(r[k], 1)
        final = float("%.3g" % align_ref.corner_shift(corners, T, P))
        # the first search after whose update the pose is as close as it will be at the end (within a factor of two): where a loop that
        # hovers above min_delta could have stopped
        settled = next(i + 1 for i, r in enumerate(rows) if r.get("pose_error", final) <= 2.0 * final)
        return dict(searches=len(rows), converged=converged, device_us=round(sum(r[k] for r in rows for k in used), 1), pose_error=final,
                    settled_after=settled, iterations=rows)

    walk("point")                                                       # the warm-up: every kernel and the allocator have run once
    out = dict(shape=label, U=u, N=n, max_dist=max_dist, normals=how, min_delta=float("%.3g" % min_delta), point=walk("point"), plane=walk("plane"))
    rows = out["plane"]["iterations"]
    for k in ("search", "moments", "plane_moments"):
        out[k + "_us"] = spread([r[k] for r in rows])
    out["plane_moments_over_search"] = round(out["plane_moments_us"]["median"] / out["search_us"]["median"], 3)
    out["plane_moments_below_the_search_in_every_iteration"] = bool(all(r["plane_moments"] < r["search"] for r in rows))
    out["fewer_searches_than_point"] = bool(out["plane"]["searches"] < out["point"]["searches"])
    return out


def plane_table(doc):
    cs = doc["shapes"]
    rng = lambda d: f"{d['median']:,.0f} ({d['min']:,.0f} .. {d['max']:,.0f})"          # noqa: E731
    lines = ["| | " + " | ".join(f"{m['U']:,} -> {m['N']:,}" for m in cs) + " |", "|---|" + "---|" * len(cs)]
    lines.append("| normals of the fixed cloud | " + " | ".join(m["normals"] for m in cs) + " |")
    for p, what in (("search", "`sg_nearest_point_grid`"), ("moments", "`sg_align_moments`"), ("plane_moments", "`sg_align_plane_moments`")):
        lines.append(f"| {what}, µs per iteration of the plane loop: median (min .. max) | " + " | ".join(rng(m[p + "_us"]) for m in cs) + " |")
    lines.append("| plane moments / search; below the search in every iteration | " + " | ".join(
        f"{m['plane_moments_over_search']:.3f}; {'yes' if m['plane_moments_below_the_search_in_every_iteration'] else 'NO'}" for m in cs) + " |")
    for metric in ("point", "plane"):
        lines.append(f"| `{metric}`: searches; stop; device ms until it; corner distance from the true pose | " + " | ".join(
            f"{m[metric]['searches']}; {m[metric]['converged'] or 'none in 50'}; {m[metric]['device_us'] / 1e3:,.1f}; {m[metric]['pose_error']:.3g}"
            for m in cs) + " |")
    lines.append("| `plane`: searches until the pose is within twice its final distance | " + " | ".join(str(m["plane"]["settled_after"]) for m in cs) + " |")
    lines.append("| fewer searches than `point` | " + " | ".join("yes" if m["fewer_searches_than_point"] else "NO" for m in cs) + " |")
    return "\n".join(lines)


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
    ap.add_argument("--plane", action="store_true", help="the point-to-plane leg: both metrics until they stop -> profiles/align_plane_time.json")
    ap.add_argument("--plane-table", default=None, help="print the DESIGN 8q table of an existing --plane result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    if a.plane_table:
        print(plane_table(json.load(open(a.plane_table))))
        return
    if a.plane:
        return main_plane(a.out if a.out != os.path.join(ROOT, "profiles", "align_time.json") else os.path.join(ROOT, "profiles", "align_plane_time.json"))
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


def main_plane(out_path):
    import torch
    import thin_ref
    from seggroup_amd import oversegment, synthetic
    doc = dict(device=torch.cuda.get_device_name(0), shapes=[],
               runs="one process, one GPU; one untimed point-to-point walk as the warm-up, then each metric until align.icp's rules stop it "
                    "(50 searches at most); every device call between two HIP events")
    scan = synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00")
    big, plane = thin_ref.big_cloud()
    for label, xyz, nrm, how in (("make_room_scan(400, 375)", scan.xyz, lambda: oversegment.vertex_normals(scan.xyz, scan.faces), "faces"),
                                 ("big_cloud()", big, lambda: plane_normals(big, plane), "least-squares plane of each of the 8 labelled planes")):
        m = measure_plane(label, np.ascontiguousarray(xyz[:, :3], dtype=np.float32), nrm(), how)
        doc["shapes"].append(m)
        print(json.dumps({k: v for k, v in m.items() if k not in ("point", "plane")}), flush=True)
        print(json.dumps({k: {kk: vv for kk, vv in m[k].items() if kk != "iterations"} for k in ("point", "plane")}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(plane_table(doc))


if __name__ == "__main__":
    main()
