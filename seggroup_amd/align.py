"""Rigid alignment of two clouds of one scene: point-to-point ICP on the exact grid index.

`transfer`, `transfer --vote` and `thin --lift` assume that both geometries are in one frame.  A photogrammetry cloud beside a laser scan,
a re-export in a slightly different pose or a rescan after a coarse manual registration are centimetres to decimetres off; this module
finds the rigid transform that brings the MOVING cloud into the FIXED cloud's frame.  The search is `sg_nearest_point_grid`, unchanged
and exact; around it `sg_rigid_apply` moves the cloud (double arithmetic, one rounding to fp32), `sg_align_moments` folds the matched
pairs inside the radius into the 17 sums of a closed-form fit (deterministic: no floating-point atomics, a tree that depends on the size
alone) and `sg_align_solve` is Kabsch on the host.  Every iteration fits the ORIGINAL moving coordinates, so transforms are never
composed and nothing drifts; the loop ends when the correspondences and the inlier set repeat (a fixed point of the data, not a
tolerance) or when the fit no longer moves the cloud's box by `min_delta`.

    python -m seggroup_amd.align --moving-scans A --fixed-scans B --max-dist D --out DIR
                                 [--init DIR] [--max-iter 50] [--scenes FILE] [--workers W] [--device D]
        for every scene present in both trees: DIR/<scene>.align.json (T as 4 rows of 4, mapping A's coordinates into B's frame, the
        Alignment's scalars, both vertex counts and max_dist) and one DIR/align_report.json.  --init DIR: start from the T of
        DIR/<scene>.align.json (a file of the same form; only T is read).  `transfer --align DIR` reads these files.

Not here, on purpose: point-to-plane, trimmed fractions, robust weights, scale, and any global (init-free) registration.  This is
point-to-point ICP with a fixed inlier radius: it refines a pose that is already inside its basin, and takes an initial transform for
everything else.  `max_dist` has no default: like `--max-edge` it depends on the scan's unit and on how wrong the pose may be.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import hip, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace
from .prepare import mesh_arrays, nearest_point_grid, read_ply

ALIGN_SUFFIX = ".align.json"
REPORT_NAME = "align_report.json"
SCALARS = ("iterations", "converged", "inliers", "rms_before", "rms_after", "rotation_deg", "translation")


@dataclass
class Alignment:
    """What icp returns.  `T` [4,4] float64 maps MOVING coordinates into the FIXED cloud's frame; `converged` is "fixed point" (the
    correspondences and the inlier set repeated), "min_delta" (the last fit moved the box by no more than min_delta) or False (max_iter
    searches); `rms_before` / `rms_after` are sqrt(sum d2 / n) over the inliers of the first / the last search (the last search ran at
    the pose before a final sub-min_delta update); `idx`, `d2`, `inlier` are the last search's device tensors."""
    T: np.ndarray
    iterations: int
    converged: object
    inliers: int
    rms_before: float
    rms_after: float
    rotation_deg: float
    translation: list
    idx: object = None
    d2: object = None
    inlier: object = None

    def scalars(self) -> dict:
        return {k: getattr(self, k) for k in SCALARS}


def as_transform(T, who: str = "align") -> np.ndarray:
    """a [4,4] or [3,4] matrix -> float64 [4,4] with the last row 0 0 0 1; anything else, or a non-finite entry, is a ValueError"""
    T = np.asarray(T, dtype=np.float64)
    if T.shape not in ((4, 4), (3, 4)) or not np.isfinite(T).all():
        raise ValueError(f"{who}: a transform is a finite [4,4] (or [3,4]) matrix")
    out = np.eye(4)
    out[:3] = T[:3]
    return out


def _vec3(v, who: str):
    v = np.ascontiguousarray(np.zeros(3) if v is None else v, dtype=np.float64)
    if v.shape != (3,):
        raise ValueError(f"{who}: an origin is 3 numbers")
    return v


def _rows(a, dev, who: str):
    import torch
    d = device_tensor(a, torch.float32, dev)
    if d.dim() != 2 or d.shape[1] < 3:
        raise ValueError(f"{who}: a cloud is [N, >= 3] rows with xyz first")
    return d


def apply(xyz, T, device=None, stream=None):
    """sg_rigid_apply: out[u][r] = (float)(((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r]) in double, one rounding to fp32 -> float32 [U,3]
    device tensor.  xyz is [U, >= 3]; T any finite [4,4] / [3,4] matrix."""
    import torch
    T = np.ascontiguousarray(as_transform(T, "apply")[:3])
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_x = _rows(xyz, dev, "apply")
        u = int(d_x.shape[0])
        out = torch.empty((u, 3), dtype=torch.float32, device=dev)
        hip.check_arg(lib.sg_rigid_apply(d_x.data_ptr(), int(d_x.shape[1]), u, T.ctypes.data, out.data_ptr(), stream_ptr(stream)))
        sync(stream)
    return out


def moments(x, y, idx, d2, max_dist, origin_x=None, origin_y=None, device=None, stream=None) -> np.ndarray:
    """sg_align_moments over the pairs (x[u], y[idx[u]]) with d2[u] <= (float32)(max_dist * max_dist) -> float64 [17]:
    n | sum a [3] | sum b [3] | sum a b^T [9] | sum d2, with a = x - origin_x and b = y - origin_y in double (origins default to 0).
    Deterministic: the same input gives the same bytes.  An index outside 0..N-1 is a ValueError."""
    import torch
    ox, oy = _vec3(origin_x, "moments"), _vec3(origin_y, "moments")
    max_d2 = float(np.float32(float(max_dist) * float(max_dist)))
    dev = torch_device(device)
    lib = hip.lib()
    out = np.zeros(17, np.float64)
    with torch.cuda.device(dev), on_stream(stream):
        d_x, d_y = _rows(x, dev, "moments"), _rows(y, dev, "moments")
        d_idx, d_d2 = device_tensor(idx, torch.int64, dev), device_tensor(d2, torch.float32, dev)
        u = int(d_x.shape[0])
        if d_idx.shape != (u,) or d_d2.shape != (u,):
            raise ValueError("moments: idx and d2 hold one entry per row of x")
        ws = workspace(lib.sg_align_moments_ws_bytes(u), dev)
        hip.check_arg(lib.sg_align_moments(d_x.data_ptr(), int(d_x.shape[1]), u, d_y.data_ptr(), int(d_y.shape[1]), int(d_y.shape[0]),
                                           d_idx.data_ptr(), d_d2.data_ptr(), max_d2, ox.ctypes.data, oy.ctypes.data, out.ctypes.data,
                                           ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return out


def solve(m, origin_x=None, origin_y=None) -> np.ndarray:
    """sg_align_solve (host only, runs without a GPU): the 17 moments and their origins -> T float64 [4,4], the proper rigid transform
    that minimises sum |R x + t - y|^2, for un-shifted coordinates.  Fewer than 3 pairs, or pairs on a line, raise hip.SgError
    (SG_EUNSUP, "degenerate"); a non-finite moment is a ValueError."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (17,):
        raise ValueError("solve: 17 moments")
    ox, oy = _vec3(origin_x, "solve"), _vec3(origin_y, "solve")
    T = np.eye(4)
    hip.check_arg(hip.lib().sg_align_solve(m.ctypes.data, ox.ctypes.data, oy.ctypes.data, T.ctypes.data))
    return T


def box_corners(lo, hi) -> np.ndarray:
    """the 8 corners of the box lo..hi -> float64 [8,3]"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float64)


def corner_shift(corners, T0, T1) -> float:
    """the largest distance between a corner moved by T0 and the same corner moved by T1"""
    p0, p1 = corners @ T0[:3, :3].T + T0[:3, 3], corners @ T1[:3, :3].T + T1[:3, 3]
    return float(np.sqrt(((p1 - p0) ** 2).sum(1)).max())


def rotation_deg(T) -> float:
    return math.degrees(math.acos(min(1.0, max(-1.0, (float(np.trace(np.asarray(T)[:3, :3])) - 1.0) / 2.0))))


def icp(moving_xyz, fixed_xyz, max_dist, init=None, max_iter: int = 50, min_delta=None, index: str = "grid", device=None,
        stream=None) -> Alignment:
    """Point-to-point ICP with a fixed inlier radius -> Alignment; T maps MOVING coordinates into the FIXED cloud's frame.

        T = init or identity
        repeat up to max_iter times:
            p       = apply(moving, T)
            idx, d2 = nearest_point_grid(p, fixed)
            inlier  = d2 <= (float32)(max_dist * max_dist)
            (idx, inlier) equal to the previous iteration's: converged = "fixed point", stop
            T_new   = solve(moments(moving, fixed, idx, d2, ...))           # the ORIGINAL moving coordinates; origins = the box centres
            the moving box's 8 corners move by <= min_delta between T and T_new: T = T_new, converged = "min_delta", stop
            T = T_new

    `min_delta` defaults to one fp32 ulp of the largest absolute coordinate of either cloud (2^-23 max|c|): below it the moved fp32 points
    cannot change by more than their own rounding.  No inliers, or a degenerate fit (fewer than 3 pairs, pairs on a line), is a
    ValueError that names max_dist."""
    import torch
    if index != "grid":
        raise ValueError("icp: the search runs through the grid index only (index='grid'), not %r" % (index,))
    max_dist = float(max_dist)
    if not max_dist > 0.0:
        raise ValueError("icp: max_dist must be > 0 (the inlier radius, in the scan's unit)")
    if int(max_iter) < 1:
        raise ValueError("icp: max_iter must be at least 1")
    T = np.eye(4) if init is None else as_transform(init, "icp: init")
    dev = torch_device(device)
    with torch.cuda.device(dev), on_stream(stream):
        d_mov, d_fix = _rows(moving_xyz, dev, "icp"), _rows(fixed_xyz, dev, "icp")
        if d_mov.shape[0] < 1 or d_fix.shape[0] < 1:
            raise ValueError("icp: a cloud needs at least one point")
        box = [(c[:, :3].min(0).values.double().cpu().numpy(), c[:, :3].max(0).values.double().cpu().numpy()) for c in (d_mov, d_fix)]
    if not all(np.isfinite(b).all() for lo_hi in box for b in lo_hi):
        raise ValueError("icp: a coordinate that is not finite")
    (mlo, mhi), (flo, fhi) = box
    origin_m, origin_f = 0.5 * (mlo + mhi), 0.5 * (flo + fhi)
    corners = box_corners(mlo, mhi)
    if min_delta is None:
        min_delta = 2.0 ** -23 * float(max(np.abs(b).max() for lo_hi in box for b in lo_hi))
    max_d2 = float(np.float32(max_dist * max_dist))
    prev = None
    converged = False
    rms_before = rms_after = None
    iterations = 0
    for _ in range(int(max_iter)):
        moved = apply(d_mov, T, device=dev, stream=stream)
        idx, d2 = nearest_point_grid(moved, d_fix, device=dev, stream=stream)
        with torch.cuda.device(dev), on_stream(stream):
            inlier = d2 <= max_d2
            same = prev is not None and bool(torch.equal(idx, prev[0])) and bool(torch.equal(inlier, prev[1]))
        iterations += 1
        m = moments(d_mov, d_fix, idx, d2, max_dist, origin_m, origin_f, device=dev, stream=stream)
        n = int(m[0])
        if n == 0:
            raise ValueError("icp: no point of the moving cloud has a fixed point within max_dist = %g -- a larger max_dist, or an initial "
                             "transform (init=, --init) that brings the clouds closer" % max_dist)
        rms_after = math.sqrt(m[16] / n)
        if rms_before is None:
            rms_before = rms_after
        prev = (idx, inlier)
        if same:
            converged = "fixed point"
            break
        try:
            T_new = solve(m, origin_m, origin_f)
        except hip.SgError as e:
            if e.code != hip.SG_EUNSUP:
                raise
            raise ValueError("icp: the %d pairs within max_dist = %g do not determine a pose (%s)" % (n, max_dist, e)) from None
        shift = corner_shift(corners, T, T_new)
        T = T_new
        if shift <= min_delta:
            converged = "min_delta"
            break
    return Alignment(T=T, iterations=iterations, converged=converged, inliers=n, rms_before=rms_before, rms_after=rms_after,
                     rotation_deg=rotation_deg(T), translation=[float(v) for v in T[:3, 3]], idx=idx, d2=d2, inlier=inlier)


# ---- files --------------------------------------------------------------------------------------------------------------------------
def align_path(directory: str, scene: str) -> str:
    return os.path.join(directory, scene + ALIGN_SUFFIX)


def read_align(path: str) -> dict:
    """a <scene>.align.json -> its document, with T as float64 [4,4]; a file without a usable T is a ValueError"""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or "T" not in doc:
        raise ValueError(f"{path}: no T")
    doc["T"] = as_transform(doc["T"], path)
    return doc


def write_align(path: str, al: Alignment, moving_v: int, fixed_v: int, max_dist: float) -> dict:
    doc = dict(al.scalars(), T=[[float(v) for v in row] for row in al.T], moving_V=int(moving_v), fixed_V=int(fixed_v), max_dist=float(max_dist))
    scans.write_report(path, doc)
    return doc


def _scan_xyz(scans_dir: str, scene: str):
    return mesh_arrays(read_ply(os.path.join(scans_dir, scene, scene + scans.PLY_SUFFIX)))[0]


def align_scene(scene: str, moving_scans: str, fixed_scans: str, max_dist: float, out_dir: str, init_dir=None, max_iter: int = 50, device=None,
                stream=None) -> dict:
    """One scene: <moving_scans>/<scene> onto <fixed_scans>/<scene> -> its entry of align_report.json; writes <out_dir>/<scene>.align.json"""
    init = read_align(align_path(init_dir, scene))["T"] if init_dir else None
    mov, fix = _scan_xyz(moving_scans, scene), _scan_xyz(fixed_scans, scene)
    al = icp(mov, fix, max_dist, init=init, max_iter=max_iter, device=device, stream=stream)
    os.makedirs(out_dir, exist_ok=True)
    doc = write_align(align_path(out_dir, scene), al, mov.shape[0], fix.shape[0], max_dist)
    del doc["T"]
    return doc


def align_scans(moving_scans: str, fixed_scans: str, max_dist: float, out_dir: str, init_dir=None, max_iter: int = 50, scenes=None,
                workers: int = 4, device=None):
    """Every scene that both trees hold (or the named ones) -> (report {scene: entry}, missing {scene: why}); writes
    <out_dir>/align_report.json.  Workers are threads, each with its own stream."""
    dev = torch_device(device)
    have_m, have_f = set(scans.scan_names(moving_scans)), set(scans.scan_names(fixed_scans))
    if scenes is None:
        scenes = sorted(have_m | have_f)
    missing, todo = {}, []
    for s in scenes:
        if s not in have_m:
            missing[s] = "no scan under --moving-scans"
        elif s not in have_f:
            missing[s] = "no scan under --fixed-scans"
        elif init_dir and not os.path.isfile(align_path(init_dir, s)):
            missing[s] = "no %s under --init" % (s + ALIGN_SUFFIX)
        else:
            todo.append(s)
    report = dict(scans.map_scans(todo, workers, dev, lambda scene, stream: align_scene(scene, moving_scans, fixed_scans, max_dist, out_dir,
                                                                                        init_dir, max_iter, device=dev, stream=stream)))
    os.makedirs(out_dir, exist_ok=True)
    scans.write_report(os.path.join(out_dir, REPORT_NAME), {"max_dist": float(max_dist), "max_iter": int(max_iter), "scenes": report,
                                                            "missing": missing})
    return report, missing


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.align", description=__doc__.split("\n\n")[0])
    ap.add_argument("--moving-scans", required=True, help="the scans that are moved (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--fixed-scans", required=True, help="the scans whose frame T maps into")
    ap.add_argument("--max-dist", type=float, required=True, help="the inlier radius, in the scans' unit; there is no default")
    ap.add_argument("--out", required=True, help="the directory that receives <scene>.align.json and align_report.json")
    ap.add_argument("--init", default=None, help="a directory of <scene>.align.json files whose T the search starts from")
    ap.add_argument("--max-iter", type=int, default=50, help="searches at most (default 50)")
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line")
    scans.add_workers_argument(ap)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    if not a.max_dist > 0.0 or a.max_iter < 1:
        ap.error("--max-dist must be > 0 and --max-iter at least 1")
    try:
        report, missing = align_scans(a.moving_scans, a.fixed_scans, a.max_dist, a.out, a.init, a.max_iter, scans.scene_list(a.scenes),
                                      a.workers, a.device)
    except ValueError as e:
        if "max_dist" not in str(e):
            raise
        ap.error(str(e))
    for scene, e in report.items():
        print("aligned", scene, "%d searches" % e["iterations"], "converged: %s" % e["converged"], "rms %.4g -> %.4g" % (e["rms_before"], e["rms_after"]),
              "%.4g deg" % e["rotation_deg"])
    for scene, why in sorted(missing.items()):
        print("skipped", scene, "(" + why + ")")
    print(f"{len(report)} scenes aligned, {len(missing)} skipped")
    return 0


if __name__ == "__main__":
    sys.exit(main())
