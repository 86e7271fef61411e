"""Rigid alignment of two clouds of one scene: point-to-point and point-to-plane ICP on the exact grid index.

`transfer`, `transfer --vote` and `thin --lift` assume that both geometries are in one frame.  A photogrammetry cloud beside a laser scan,
a re-export in a slightly different pose or a rescan after a coarse manual registration are centimetres to decimetres off; this module
finds the rigid transform that brings the MOVING cloud into the FIXED cloud's frame.  The search is `sg_nearest_point_grid`, unchanged
and exact; around it `sg_rigid_apply` moves the cloud (double arithmetic, one rounding to fp32), `sg_align_moments` folds the matched
pairs inside the radius into the 17 sums of a closed-form fit (deterministic: no floating-point atomics, a tree that depends on the size
alone) and `sg_align_solve` is Kabsch on the host.  Every iteration fits the ORIGINAL moving coordinates, so transforms are never
composed and nothing drifts; the loop ends when the correspondences and the inlier set repeat (a fixed point of the data, not a
tolerance) or when the fit no longer moves the cloud's box by `min_delta`.

Rooms are floors, walls and furniture faces, and on those point-to-point pairs slide along the planes.  `metric="plane"`
minimises the distance to the FIXED cloud's tangent planes instead: the search is the same, `sg_align_plane_moments` folds the candidate
pairs into the 31 sums of one Gauss-Newton step (the same deterministic trees), `sg_align_plane_solve` solves the 6x6 system on the host
and composes the step onto T.  The fixed cloud's normals are the caller's, or `oversegment.pointcloud_normals` over the grid kNN.

    python -m seggroup_amd.align --moving-scans A --fixed-scans B --max-dist D --out DIR
                                 [--init DIR] [--max-iter 50] [--metric {point,plane}] [--normals-k K] [--scenes FILE] [--workers W]
                                 [--global-init --voxel H [--hypotheses N] [--seed S] [--verify K] [--mutual]] [--device D]
        for every scene present in both trees: DIR/<scene>.align.json (T as 4 rows of 4, mapping A's coordinates into B's frame, the
        Alignment's scalars, both vertex counts and max_dist) and one DIR/align_report.json.  --init DIR: start from the T of
        DIR/<scene>.align.json (a file of the same form; only T is read).  `transfer --align DIR` reads these files.  --metric plane:
        the fixed scan's normals come from its faces (`oversegment.vertex_normals`) when its PLY has any, else from the covariance of
        its --normals-k (default 10) nearest points; the files then also hold metric, normals ("faces" | "knn-K"), skipped,
        plane_rms_before and plane_rms_after.  --global-init --voxel H: the search starts from `register.global_registration` of the two
        scans thinned at H (no starting pose is needed; exclusive with --init), and the files gain a `global` record with
        the Coarse's scalars.

Not here, on purpose: trimmed fractions, robust weights and scale.  This is ICP with a fixed inlier radius: it refines a pose that is
already inside its basin, and takes an initial transform -- a caller's, or register.py's coarse one -- for everything else.  `max_dist`
has no default: like `--max-edge` it depends on the scan's unit and on how wrong the pose may be.
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
from .device import cloud_box, device_rows, device_tensor, on_stream, stream_ptr, sync, torch_device, vec3, workspace
from .prepare import mesh_arrays, nearest_point_grid, read_ply

ALIGN_SUFFIX = ".align.json"
REPORT_NAME = "align_report.json"
SCALARS = ("iterations", "converged", "inliers", "rms_before", "rms_after", "rotation_deg", "translation")
PLANE_SCALARS = ("metric", "skipped", "plane_rms_before", "plane_rms_after")     # what metric="plane" adds to them
METRICS = ("point", "plane")


@dataclass
class Alignment:
    """What icp returns.  `T` [4,4] float64 maps MOVING coordinates into the FIXED cloud's frame; `converged` is "fixed point" (the
    correspondences and the inlier set repeated), "min_delta" (the last fit moved the box by no more than min_delta) or False (max_iter
    searches); `rms_before` / `rms_after` are sqrt(sum d2 / n) over the inliers of the first / the last search (the last search ran at
    the pose before a final sub-min_delta update); `idx`, `d2`, `inlier` are the last search's device tensors.  With metric="plane"
    (never "fixed point" there) `inliers` counts the candidates with a usable normal, `skipped` those without at the last search, and
    `plane_rms_before` / `plane_rms_after` are sqrt(sum r^2 / n) of the point-to-plane residual at the first / the last search; a
    point-to-point Alignment and its scalars() carry none of these."""
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
    metric: str = "point"
    skipped: object = None
    plane_rms_before: object = None
    plane_rms_after: object = None

    def scalars(self) -> dict:
        return {k: getattr(self, k) for k in SCALARS + (PLANE_SCALARS if self.metric == "plane" else ())}


def as_transform(T, who: str = "align") -> np.ndarray:
    """a [4,4] or [3,4] matrix -> float64 [4,4] with the last row 0 0 0 1; anything else, or a non-finite entry, is a ValueError"""
    T = np.asarray(T, dtype=np.float64)
    if T.shape not in ((4, 4), (3, 4)) or not np.isfinite(T).all():
        raise ValueError(f"{who}: a transform is a finite [4,4] (or [3,4]) matrix")
    out = np.eye(4)
    out[:3] = T[:3]
    return out


def apply(xyz, T, device=None, stream=None):
    """sg_rigid_apply: out[u][r] = (float)(((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r]) in double, one rounding to fp32 -> float32 [U,3]
    device tensor.  xyz is [U, >= 3]; T any finite [4,4] / [3,4] matrix."""
    import torch
    T = np.ascontiguousarray(as_transform(T, "apply")[:3])
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_x = device_rows(xyz, dev, "apply")
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
    ox, oy = vec3(origin_x, "moments"), vec3(origin_y, "moments")
    max_d2 = float(np.float32(float(max_dist) * float(max_dist)))
    dev = torch_device(device)
    lib = hip.lib()
    out = np.zeros(17, np.float64)
    with torch.cuda.device(dev), on_stream(stream):
        d_x, d_y = device_rows(x, dev, "moments"), device_rows(y, dev, "moments")
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
    ox, oy = vec3(origin_x, "solve"), vec3(origin_y, "solve")
    T = np.eye(4)
    hip.check_arg(hip.lib().sg_align_solve(m.ctypes.data, ox.ctypes.data, oy.ctypes.data, T.ctypes.data))
    return T


def plane_moments(x, T, y, normals, idx, d2, max_dist, origin=None, device=None, stream=None) -> np.ndarray:
    """sg_align_plane_moments over the pairs (T x[u], y[idx[u]]) with d2[u] <= (float32)(max_dist * max_dist) -> float64 [31]:
    usable | skipped | upper triangle of sum J J^T [21] | sum J r [6] | sum r r | sum d2, with a = T x - origin, b = y - origin,
    n = normals[idx[u]], r = (a - b) . n and J = [a x n, n] in double (origin defaults to 0).  x is the ORIGINAL moving cloud; `normals`
    [N, >= 3] belong to y.  A candidate whose normal is not finite or has a squared length outside 0.25..4 is counted in [1] and adds
    nothing else.  Deterministic: the same input gives the same bytes.  An index outside 0..N-1 is a ValueError."""
    import torch
    T = np.ascontiguousarray(as_transform(T, "plane_moments")[:3])
    o = vec3(origin, "plane_moments")
    max_d2 = float(np.float32(float(max_dist) * float(max_dist)))
    dev = torch_device(device)
    lib = hip.lib()
    out = np.zeros(31, np.float64)
    with torch.cuda.device(dev), on_stream(stream):
        d_x, d_y, d_n = device_rows(x, dev, "plane_moments"), device_rows(y, dev, "plane_moments"), device_rows(normals, dev, "plane_moments")
        d_idx, d_d2 = device_tensor(idx, torch.int64, dev), device_tensor(d2, torch.float32, dev)
        u = int(d_x.shape[0])
        if d_idx.shape != (u,) or d_d2.shape != (u,):
            raise ValueError("plane_moments: idx and d2 hold one entry per row of x")
        if d_n.shape[0] != d_y.shape[0]:
            raise ValueError("plane_moments: one normal per row of y (%d normals, %d points)" % (d_n.shape[0], d_y.shape[0]))
        ws = workspace(lib.sg_align_plane_moments_ws_bytes(u), dev)
        hip.check_arg(lib.sg_align_plane_moments(d_x.data_ptr(), int(d_x.shape[1]), u, T.ctypes.data, d_y.data_ptr(), int(d_y.shape[1]),
                                                 int(d_y.shape[0]), d_n.data_ptr(), int(d_n.shape[1]), d_idx.data_ptr(), d_d2.data_ptr(), max_d2,
                                                 o.ctypes.data, out.ctypes.data, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return out


def plane_solve(m, T, origin, length) -> np.ndarray:
    """sg_align_plane_solve (host only, runs without a GPU): the 31 moments taken at the pose T about `origin` -> T_new float64 [4,4], T
    with one Gauss-Newton step of the point-to-plane fit composed onto it (rotation re-orthonormalised).  `length` > 0 scales the
    rotational unknowns into length units for the degeneracy rule.  Fewer than 6 usable pairs, or planes that leave a motion free, raise
    hip.SgError (SG_EUNSUP, "degenerate"); a non-finite moment, origin, length or T is a ValueError."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (31,):
        raise ValueError("plane_solve: 31 moments")
    T34 = np.asarray(T, dtype=np.float64)
    if T34.shape not in ((4, 4), (3, 4)):
        raise ValueError("plane_solve: a transform is a [4,4] (or [3,4]) matrix")
    T34 = np.ascontiguousarray(T34[:3])
    o = vec3(origin, "plane_solve")
    out = np.zeros((4, 4))
    hip.check_arg(hip.lib().sg_align_plane_solve(m.ctypes.data, o.ctypes.data, float(length), T34.ctypes.data, out.ctypes.data, None))
    return out


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
        stream=None, metric: str = "point", normals=None, normals_k: int = 10) -> Alignment:
    """ICP with a fixed inlier radius -> Alignment; T maps MOVING coordinates into the FIXED cloud's frame.  metric="point":

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
    ValueError that names max_dist.

    metric="plane" (DESIGN.md 8q): `normals` is the FIXED cloud's [N, >= 3] array, or None for pointcloud_normals(fixed, normals_k) over
    the grid kNN, computed once before the loop; c is the fixed box's centre and L half its diagonal:

        repeat up to max_iter times:
            p       = apply(moving, T);  idx, d2 = nearest_point_grid(p, fixed);  inlier = d2 <= (float32)(max_dist * max_dist)
            T_new   = plane_solve(plane_moments(moving, T, fixed, normals, idx, d2, max_dist, c), T, c, L)
            the moving box's 8 corners move by <= min_delta between T and T_new: T = T_new, converged = "min_delta", stop
            T = T_new

    There is no "fixed point" rule: a Gauss-Newton step is not closed-form, so repeated pairs do not imply a zero step.  No usable
    candidate, or planes that leave a motion free, is a ValueError that names max_dist (the latter also "plane")."""
    import torch
    if metric not in METRICS:
        raise ValueError("icp: metric must be 'point' or 'plane', not %r" % (metric,))
    if metric == "point" and normals is not None:
        raise ValueError("icp: normals belong to metric='plane'; point-to-point ICP does not use them")
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
        d_mov, d_fix = device_rows(moving_xyz, dev, "icp"), device_rows(fixed_xyz, dev, "icp")
        if d_mov.shape[0] < 1 or d_fix.shape[0] < 1:
            raise ValueError("icp: a cloud needs at least one point")
        if normals is not None:
            normals = device_rows(normals, dev, "icp: normals")
            if normals.shape[0] != d_fix.shape[0]:
                raise ValueError("icp: one normal per point of the FIXED cloud (%d normals, %d points)" % (normals.shape[0], d_fix.shape[0]))
        (mlo, mhi), (flo, fhi) = cloud_box(d_mov, "icp"), cloud_box(d_fix, "icp")
    origin_m, origin_f = 0.5 * (mlo + mhi), 0.5 * (flo + fhi)
    corners = box_corners(mlo, mhi)
    if min_delta is None:
        min_delta = 2.0 ** -23 * float(max(np.abs(b).max() for b in (mlo, mhi, flo, fhi)))
    max_d2 = float(np.float32(max_dist * max_dist))
    # what a metric supplies: its sums at a pose, its fit, where the skipped count and the rms terms sit in the sums, whether repeated pairs
    # end the loop, and what its fit finds
    if metric == "point":
        sums = lambda T, idx, d2: moments(d_mov, d_fix, idx, d2, max_dist, origin_m, origin_f, device=dev, stream=stream)
        fit = lambda m, T: solve(m, origin_m, origin_f)
        at_skipped, at_rms, fixed_point, finds = None, (16,), True, "a pose"
    else:
        if normals is None:
            normals = fixed_normals(d_fix, int(normals_k), device=dev)
        length = 0.5 * float(np.sqrt(((fhi - flo) ** 2).sum()))
        if not length > 0.0:
            raise ValueError("icp: the fixed cloud is a single point; metric='plane' needs planes (max_dist = %g)" % max_dist)
        sums = lambda T, idx, d2: plane_moments(d_mov, T, d_fix, normals, idx, d2, max_dist, origin_f, device=dev, stream=stream)
        fit = lambda m, T: plane_solve(m, T, origin_f, length)
        at_skipped, at_rms, fixed_point, finds = 1, (30, 29), False, "a point-to-plane pose"
    prev = first = None
    converged = False
    iterations = 0
    for _ in range(int(max_iter)):
        moved = apply(d_mov, T, device=dev, stream=stream)
        idx, d2 = nearest_point_grid(moved, d_fix, device=dev, stream=stream)
        with torch.cuda.device(dev), on_stream(stream):
            inlier = d2 <= max_d2
            same = fixed_point and prev is not None and bool(torch.equal(idx, prev[0])) and bool(torch.equal(inlier, prev[1]))
        iterations += 1
        m = sums(T, idx, d2)
        n, skipped = int(m[0]), None if at_skipped is None else int(m[at_skipped])
        if n == 0:
            if skipped:
                raise ValueError("icp: every pair within max_dist = %g was skipped for its normal (%d pairs: the fixed cloud's normals there "
                                 "are zero, not finite or far from unit length)" % (max_dist, skipped))
            raise ValueError("icp: no point of the moving cloud has a fixed point within max_dist = %g -- a larger max_dist, or an initial "
                             "transform (init=, --init) that brings the clouds closer" % max_dist)
        last = [math.sqrt(m[i] / n) for i in at_rms]
        if first is None:
            first = last
        prev = (idx, inlier)
        if same:
            converged = "fixed point"
            break
        try:
            T_new = fit(m, T)
        except hip.SgError as e:
            if e.code != hip.SG_EUNSUP:
                raise
            raise ValueError("icp: the %d pairs within max_dist = %g do not determine %s (%s)" % (n, max_dist, finds, e)) from None
        shift = corner_shift(corners, T, T_new)
        T = T_new
        if shift <= min_delta:
            converged = "min_delta"
            break
    plane = {} if metric == "point" else dict(metric="plane", skipped=skipped, plane_rms_before=first[1], plane_rms_after=last[1])
    return Alignment(T=T, iterations=iterations, converged=converged, inliers=n, rms_before=first[0], rms_after=last[0],
                     rotation_deg=rotation_deg(T), translation=[float(v) for v in T[:3, 3]], idx=idx, d2=d2, inlier=inlier, **plane)


def fixed_normals(fixed_xyz, k: int = 10, device=None):
    """the normals metric="plane" uses when the caller has none -> float32 [N,3] device tensor: oversegment.pointcloud_normals over the
    exact grid kNN-k of the cloud itself"""
    from .oversegment import pointcloud_normals
    from .prepare import pointcloud_knn
    if int(k) < 3:
        raise ValueError("icp: normals_k must be at least 3 (a plane through fewer neighbours has no normal)")
    import torch
    dev = torch_device(device)
    with torch.cuda.device(dev):
        xyz = device_tensor(fixed_xyz, torch.float32, dev)[:, :3].contiguous()
    return pointcloud_normals(xyz, int(k), knn=pointcloud_knn(xyz, int(k), device=dev, index="grid"), device=dev)


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


def write_align(path: str, al: Alignment, moving_v: int, fixed_v: int, max_dist: float, normals=None, coarse=None) -> dict:
    """`normals`: where a plane Alignment's normals came from ("faces" | "knn-K"); a point-to-point file has no such key.  `coarse`: the
    register.Coarse the search started from; a file without one has no `global` key"""
    doc = dict(al.scalars(), T=[[float(v) for v in row] for row in al.T], moving_V=int(moving_v), fixed_V=int(fixed_v), max_dist=float(max_dist))
    if normals is not None:
        doc["normals"] = normals
    if coarse is not None:
        doc["global"] = dict(coarse.scalars(), T=[[float(v) for v in row] for row in coarse.T])
    scans.write_report(path, doc)
    return doc


def _scan_xyz(scans_dir: str, scene: str):
    return mesh_arrays(read_ply(os.path.join(scans_dir, scene, scene + scans.PLY_SUFFIX)))[0]


def scan_normals(xyz, faces, k: int = 10, device=None):
    """the normals of a scan as the FIXED cloud of metric="plane" -> (float32 [V,3] device tensor, "faces" | "knn-K"): from its faces
    (oversegment.vertex_normals; a vertex without a face gets zeros, which the fit skips) when it has any, else from the kNN covariance"""
    if faces is not None and len(faces):
        from .oversegment import vertex_normals
        return vertex_normals(xyz, faces, device=device), "faces"
    return fixed_normals(xyz, k, device=device), "knn-%d" % int(k)


def check_metric(metric, normals_k) -> None:
    """the combinations of metric and normals_k that are refused before anything runs (ValueError)"""
    if metric not in METRICS:
        raise ValueError("--metric (metric=) must be 'point' or 'plane', not %r" % (metric,))
    if normals_k is not None:
        if metric != "plane":
            raise ValueError("--normals-k (normals_k=) needs --metric plane (metric='plane'): point-to-point ICP uses no normals")
        if int(normals_k) < 3:
            raise ValueError("--normals-k (normals_k=) must be at least 3")


def check_global(global_init, voxel, init_dir, hypotheses=None, seed=None, verify=None, mutual=None) -> None:
    """the combinations of --global-init and its options that are refused before anything runs (ValueError)"""
    if not global_init:
        for name, v in (("--voxel", voxel), ("--hypotheses", hypotheses), ("--seed", seed), ("--verify", verify), ("--mutual", mutual or None)):
            if v is not None:
                raise ValueError("%s needs --global-init (global_init=True): without the coarse stage there is nothing it sets" % name)
        return
    if init_dir:
        raise ValueError("--global-init and --init are two starting poses; give one")
    if voxel is None or not float(voxel) > 0.0:
        raise ValueError("--global-init needs --voxel (voxel=) > 0: the edge both scans are thinned at, in the scans' unit; it has no default")
    if hypotheses is not None and not 1 <= int(hypotheses) <= 1 << 24:
        raise ValueError("--hypotheses (hypotheses=) must be in 1..2^24")
    if verify is not None and int(verify) < 1:
        raise ValueError("--verify (verify=) must be at least 1")


def global_options(hypotheses=None, seed=None, verify=None, mutual=None) -> dict:
    """the options of --global-init that were given, as global_registration's keywords"""
    given = dict(hypotheses=hypotheses, seed=seed, verify=verify, mutual=mutual or None)
    return {k: v for k, v in given.items() if v is not None}


def align_scene(scene: str, moving_scans: str, fixed_scans: str, max_dist: float, out_dir: str, init_dir=None, max_iter: int = 50, device=None,
                stream=None, metric: str = "point", normals_k=None, global_init: bool = False, voxel=None, **coarse_options) -> dict:
    """One scene: <moving_scans>/<scene> onto <fixed_scans>/<scene> -> its entry of align_report.json; writes <out_dir>/<scene>.align.json.
    `global_init` with `voxel` (and hypotheses=, seed=, verify=, mutual=): the ICP starts from register.global_registration's pose."""
    check_metric(metric, normals_k)
    check_global(global_init, voxel, init_dir, **coarse_options)
    init = read_align(align_path(init_dir, scene))["T"] if init_dir else None
    mov = _scan_xyz(moving_scans, scene)
    fix, _, faces = mesh_arrays(read_ply(os.path.join(fixed_scans, scene, scene + scans.PLY_SUFFIX)))
    coarse = None
    if global_init:
        from .register import global_registration
        coarse = global_registration(mov, fix, voxel=float(voxel), device=device, stream=stream, **global_options(**coarse_options))
        init = coarse.T
    if metric == "plane":
        nrm, how = scan_normals(fix, faces, 10 if normals_k is None else normals_k, device=device)
        al = icp(mov, fix, max_dist, init=init, max_iter=max_iter, device=device, stream=stream, metric="plane", normals=nrm)
    else:
        how = None
        al = icp(mov, fix, max_dist, init=init, max_iter=max_iter, device=device, stream=stream)
    os.makedirs(out_dir, exist_ok=True)
    doc = write_align(align_path(out_dir, scene), al, mov.shape[0], fix.shape[0], max_dist, normals=how, coarse=coarse)
    del doc["T"]
    return doc


def align_scans(moving_scans: str, fixed_scans: str, max_dist: float, out_dir: str, init_dir=None, max_iter: int = 50, scenes=None,
                workers: int = 4, device=None, metric: str = "point", normals_k=None, global_init: bool = False, voxel=None, **coarse_options):
    """Every scene that both trees hold (or the named ones) -> (report {scene: entry}, missing {scene: why}); writes
    <out_dir>/align_report.json.  Workers are threads, each with its own stream.  `metric`, `normals_k`, `global_init`, `voxel` and the
    coarse stage's options: align_scene's."""
    check_metric(metric, normals_k)
    check_global(global_init, voxel, init_dir, **coarse_options)
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
                                                                                        init_dir, max_iter, device=dev, stream=stream,
                                                                                        metric=metric, normals_k=normals_k,
                                                                                        global_init=global_init, voxel=voxel, **coarse_options)))
    os.makedirs(out_dir, exist_ok=True)
    head = {"max_dist": float(max_dist), "max_iter": int(max_iter)}
    if metric == "plane":
        head["metric"] = metric
    if global_init:
        head["global_init"] = dict(global_options(**coarse_options), voxel=float(voxel))
    scans.write_report(os.path.join(out_dir, REPORT_NAME), dict(head, scenes=report, missing=missing))
    return report, missing


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.align", description=__doc__.split("\n\n")[0])
    ap.add_argument("--moving-scans", required=True, help="the scans that are moved (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--fixed-scans", required=True, help="the scans whose frame T maps into")
    ap.add_argument("--max-dist", type=float, required=True, help="the inlier radius, in the scans' unit; there is no default")
    ap.add_argument("--out", required=True, help="the directory that receives <scene>.align.json and align_report.json")
    ap.add_argument("--init", default=None, help="a directory of <scene>.align.json files whose T the search starts from")
    ap.add_argument("--max-iter", type=int, default=50, help="searches at most (default 50)")
    ap.add_argument("--metric", choices=METRICS, default="point",
                    help="point: point-to-point (the default); plane: point-to-plane on the fixed scan's normals (its faces, else its kNN covariance)")
    ap.add_argument("--normals-k", type=int, default=None, metavar="K",
                    help="the neighbours of the kNN covariance normals of a face-less fixed scan (--metric plane only; default 10)")
    ap.add_argument("--global-init", action="store_true",
                    help="start from the coarse pose of a global registration (FPFH + RANSAC on the scans thinned at --voxel); no --init needed")
    ap.add_argument("--voxel", type=float, default=None, metavar="H", help="the edge both scans are thinned at for --global-init (required with it)")
    ap.add_argument("--hypotheses", type=int, default=None, metavar="N", help="RANSAC triples of --global-init (default 2^20)")
    ap.add_argument("--seed", type=int, default=None, metavar="S", help="the seed of --global-init's triples (default 0)")
    ap.add_argument("--verify", type=int, default=None, metavar="K", help="hypotheses --global-init re-scores against the whole scan (default 16)")
    ap.add_argument("--mutual", action="store_true", help="--global-init keeps only correspondences that are nearest in both directions")
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line")
    scans.add_workers_argument(ap)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    if not a.max_dist > 0.0 or a.max_iter < 1:
        ap.error("--max-dist must be > 0 and --max-iter at least 1")
    coarse_options = dict(hypotheses=a.hypotheses, seed=a.seed, verify=a.verify, mutual=a.mutual or None)
    try:
        check_metric(a.metric, a.normals_k)
        check_global(a.global_init, a.voxel, a.init, **coarse_options)
    except ValueError as e:
        ap.error(str(e))
    try:
        report, missing = align_scans(a.moving_scans, a.fixed_scans, a.max_dist, a.out, a.init, a.max_iter, scans.scene_list(a.scenes),
                                      a.workers, a.device, metric=a.metric, normals_k=a.normals_k, global_init=a.global_init, voxel=a.voxel,
                                      **coarse_options)
    except ValueError as e:
        if "max_dist" not in str(e) and "global_registration" not in str(e):
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
