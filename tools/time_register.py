#!/usr/bin/env python3
"""The global registration, measured stage by stage -> profiles/register_time.json.

    python tools/time_register.py [--repeats 5] [--voxel 0.11] [--out profiles/register_time.json]
    python tools/time_register.py --table profiles/register_time.json      # prints the markdown table of DESIGN.md 8r (no GPU needed)

One process, one GPU, one stream.  The cloud is make_room_scan(400, 375) (150,000 points on a 0.04 lattice with a jitter of 5e-4) thinned
at --voxel, which leaves roughly 20,000 points; the moving cloud is the same scan under the inverse of 150 degrees and 1.5 m, thinned on
its own.  Every device stage runs between two events on the stream after a warm-up, the median (min .. max) of the repeats: the radius
lists and the normals of both clouds, sg_fpfh of both, sg_feature_nearest, sg_ransac_count at 2^18, 2^20 and 2^22 hypotheses -- its
filter and its count by the library's own events (hip.stage_timer("ransac")), the count with a wave and with a thread per survivor -- and the
16 verification searches (align.apply + prepare.nearest_point_grid each).  The survivor fraction and the whole global_registration call
by the host's clock stand beside them.  EXPECTED was written down before the first run.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HYPOTHESES = (1 << 18, 1 << 20, 1 << 22)
EXPECTED = ("sg_feature_nearest: 4e8 descriptor pairs of 33 channels, brute force, on ~160 workgroups of two waves, so one workgroup a CU and "
            "every LDS read waited for -- a few ms to 20 ms; the 16 verification searches second (each builds a grid index and synchronises); "
            "sg_ransac_count below 1 ms up to 2^20 and its count kernel (0.4 % x H survivors x 20,000 correspondences in double) only "
            "near the search at 2^22; lists, normals and sg_fpfh (1.6e6 pairs) well under a millisecond each")
NOT_MEASURED = ["real scans", "two clouds of different density", "partial overlap below the test fixture's (a quarter of the room missing)",
                "several streams in flight", "clouds near the 2^18-point limit of the descriptor search", "mutual=True",
                "the host's share of a call beyond the one wall-clock figure (uploads, torch.topk, sg_triangle_pose)"]


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


def pose(deg, shift, axis=(0.3, -0.5, 1.0), direction=(0.6, -0.64, 0.48)):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T[:3, 3] = shift * np.asarray(direction, np.float64)
    return T


def measure(voxel, repeats):
    import torch
    from seggroup_amd import align, hip, register, synthetic
    from seggroup_amd.components import radius_neighbours
    from seggroup_amd.oversegment import pointcloud_normals
    from seggroup_amd.prepare import nearest_point_grid
    from seggroup_amd.thin import thin_cloud
    dev = "cuda:0"
    lib = hip.lib()
    room = np.ascontiguousarray(synthetic.make_room_scan(400, 375, 11, jitter=5e-4, name="scene0000_00").xyz, dtype=np.float32)
    P = pose(150.0, 1.5)
    Pinv = np.eye(4)
    Pinv[:3, :3], Pinv[:3, 3] = P[:3, :3].T, -P[:3, :3].T @ P[:3, 3]
    d_fix_full = torch.from_numpy(room).to(dev)
    d_mov_full = align.apply(d_fix_full, Pinv, device=dev)
    normal_radius, feature_radius, max_dist = 2.0 * voxel, 5.0 * voxel, 1.5 * voxel
    out = dict(voxel=voxel, normal_radius=normal_radius, feature_radius=feature_radius, max_dist=max_dist, full_points=int(room.shape[0]))
    out["thin_ms"] = timed(lambda: (thin_cloud(d_mov_full, voxel, device=dev), thin_cloud(d_fix_full, voxel, device=dev)), repeats)
    d_mov = d_mov_full[thin_cloud(d_mov_full, voxel, device=dev)[0].long()].contiguous()
    d_fix = d_fix_full[thin_cloud(d_fix_full, voxel, device=dev)[0].long()].contiguous()
    out.update(moving_points=int(d_mov.shape[0]), fixed_points=int(d_fix.shape[0]))
    state = {}

    def lists():
        state["nl"] = [radius_neighbours(c, normal_radius, device=dev) for c in (d_mov, d_fix)]
        state["fl"] = [radius_neighbours(c, feature_radius, device=dev) for c in (d_mov, d_fix)]

    def normals():
        state["n"] = [pointcloud_normals(c, radius=normal_radius, lists=l, device=dev) for c, l in zip((d_mov, d_fix), state["nl"])]

    def fpfh():
        state["f"] = [register.fpfh(c, n, None, lists=l, device=dev) for c, n, l in zip((d_mov, d_fix), state["n"], state["fl"])]

    out["lists_ms"] = timed(lists, repeats)
    out["normals_ms"] = timed(normals, repeats)
    out["fpfh_ms"] = timed(fpfh, repeats)
    out["feature_row_entries"] = [round(float(l[1].numel()) / c.shape[0], 1) for c, l in zip((d_mov, d_fix), state["fl"])]
    um, uf = (torch.nonzero((f != 0).any(1)).reshape(-1) for f in state["f"])
    fm, ff = state["f"][0][um].contiguous(), state["f"][1][uf].contiguous()

    def nearest():
        state["near"] = register.feature_nearest(fm, ff, device=dev)[0]

    out["feature_nearest_ms"] = timed(nearest, repeats)
    ci, cj = um, uf[state["near"]]
    c = int(ci.numel())
    moved_right = align.apply(d_mov, P, device=dev)
    right = int((((moved_right[ci] - d_fix[cj]) ** 2).sum(1).sqrt() < max_dist).sum())
    out.update(correspondences=c, right_correspondences=right)
    out["ransac"] = []
    for h in HYPOTHESES:
        row = dict(hypotheses=h)
        for lanes in (64, 1):
            def count():
                state["count"], state["surv"] = register.ransac_count(d_mov, d_fix, ci, cj, h, max_dist, device=dev, want_survivors=True)

            try:
                hip.check(lib.sg_ransac_set_tuning(lanes))
                row["call_ms_%d_lanes" % lanes] = timed(count, repeats)
                with hip.stage_timer("ransac") as t:                      # the library's own events around its three stages
                    rows = []
                    for _ in range(3):
                        count()
                        rows.append(t.read())
                us = np.median(np.asarray(rows), 0)
                row["stages_us_%d_lanes" % lanes] = {name: round(float(u), 1) for name, u in zip(t.names, us)}
                state["bytes_%d" % lanes] = state["count"].cpu().numpy().tobytes()
            finally:
                hip.check(lib.sg_ransac_set_tuning(0))
        assert state["bytes_64"] == state["bytes_1"]
        row.update(survivors=int(state["surv"]), survivor_fraction=state["surv"] / float(h), best_count=int(state["count"].max()))
        out["ransac"].append(row)
        print(json.dumps(row), flush=True)
    T = np.eye(4)
    T[:3] = P[:3]

    def verify():
        for _ in range(16):
            nearest_point_grid(align.apply(d_mov, T, device=dev), d_fix, device=dev)

    out["verify16_ms"] = timed(verify, repeats)
    lo, hi = d_mov.min(0).values.double().cpu().numpy(), d_mov.max(0).values.double().cpu().numpy()
    corners = align.box_corners(lo, hi)
    out["whole_call"] = []
    for h in HYPOTHESES:
        register.global_registration(d_mov_full, d_fix_full, voxel=voxel, hypotheses=h, device=dev)
        torch.cuda.synchronize()
        wall = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            coarse = register.global_registration(d_mov_full, d_fix_full, voxel=voxel, hypotheses=h, device=dev)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out["whole_call"].append(dict(hypotheses=h, wall_ms=dict(median=round(float(np.median(wall)), 1), min=round(min(wall), 1), max=round(max(wall), 1)),
                                      corner_distance_from_the_true_pose=round(align.corner_shift(corners, coarse.T, P), 4), count=coarse.count,
                                      verified_inliers=coarse.verified_inliers, ranked=coarse.ranked[:4]))
        print(json.dumps(out["whole_call"][-1]), flush=True)
    return out


def table(doc):
    m = doc["measured"]
    ms = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"     # noqa: E731
    lines = ["| stage | ms between events: median (min .. max) of %d |" % m["lists_ms"]["repeats"], "|---|---|"]
    lines.append(f"| points after thinning at {m['voxel']:g}: moving; fixed; correspondences; of them right | {m['moving_points']:,}; {m['fixed_points']:,}; "
                 f"{m['correspondences']:,}; {m['right_correspondences']:,} |")
    for key, what in (("thin_ms", "`thin_cloud`, both clouds"), ("lists_ms", "radius lists, both radii, both clouds"), ("normals_ms", "normals, both clouds"),
                      ("fpfh_ms", "`sg_fpfh`, both clouds"), ("feature_nearest_ms", "`sg_feature_nearest`"), ("verify16_ms", "16 verification searches")):
        lines.append(f"| {what} | {ms(m[key])} |")
    for r in m["ransac"]:
        s64, s1 = r["stages_us_64_lanes"], r["stages_us_1_lanes"]
        lines.append(f"| `sg_ransac_count`, H = 2^{int(math.log2(r['hypotheses']))}: call; gather, filter, count (µs, a wave per survivor); count with a thread "
                     f"per survivor (µs); survivors (share) | {ms(r['call_ms_64_lanes'])}; {s64['gather']:,.1f}, {s64['filter']:,.1f}, {s64['count']:,.1f}; "
                     f"{s1['count']:,.1f}; {r['survivors']:,} ({100 * r['survivor_fraction']:.2f} %) |")
    for w in m["whole_call"]:
        lines.append(f"| `global_registration`, H = 2^{int(math.log2(w['hypotheses']))}: host clock, ms; corner distance from the true pose, m | "
                     f"{w['wall_ms']['median']:,} ({w['wall_ms']['min']:,} .. {w['wall_ms']['max']:,}); {w['corner_distance_from_the_true_pose']:g} |")
    lines += ["", "Expected before the run: " + doc["expected"] + ".", "", "Not measured: " + "; ".join(doc["not_measured"]) + "."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_time.json"))
    ap.add_argument("--table", default=None, help="print the DESIGN table of an existing result file and exit")
    a = ap.parse_args()
    if a.table:
        print(table(json.load(open(a.table))))
        return
    import torch
    doc = dict(device=torch.cuda.get_device_name(0), runs="one process, one GPU, one stream", expected=EXPECTED, not_measured=list(NOT_MEASURED),
               measured=measure(a.voxel, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(table(doc))


if __name__ == "__main__":
    main()
