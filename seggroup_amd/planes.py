"""The dominant planes of a cloud on the GPU: hypothesise-and-count RANSAC, a least-squares refit, levelling on the floor
and scans without their structure.

Rooms are floors, walls and furniture faces.  A photogrammetry or hand-held scan arrives with gravity pointing anywhere, and in a scan that
still has its floor every piece of furniture is one component with it.  `detect_planes` finds the planes one after another:

    labels = -1 everywhere; origin = the centre of the cloud's box
    round p = 0, 1, .. max_planes - 1:
        count, plane, best = plane_ransac(still-free points, seed + p)      -- sg_plane_ransac: `hypotheses` triples of free points from
                                                                               splitmix64, slivers and short edges rejected, the free
                                                                               points within `dist` of every kept plane counted
        best < 0 or count[best] < min_points: stop
        m    = plane_moments(free inliers of plane[best], origin)           -- sg_plane_moments: 11 sums, deterministic trees
        fit  = plane_fit(m, origin)                                         -- sg_plane_fit (host): covariance, Jacobi, smallest eigenvector
        n    = plane_assign(fit, id = p) on a copy of labels                -- sg_plane_assign: the free points within `dist` of the REFIT
        n < min_points: stop, the copy is dropped;  else labels = the copy

Every stage is deterministic: the same cloud and seed give the same Planes.  `level_transform` turns a detected plane into the rigid
transform that puts it at z = 0 with the cloud above it (`align.apply` takes it).

    python -m seggroup_amd.planes --scans DIR --out DIR --dist D --min-points M
                                  [--max-planes P --hypotheses H --seed S --min-edge E --normal-angle DEG --normals-k K]
                                  [--level [largest|INDEX]] [--remove] [--scenes FILE --workers W --device D --force]
        per scene DIR/<scene>.planes.npz (the Planes arrays and parameters) and one DIR/planes_report.json (per scene V, the planes with
        equation / points / rms, unlabelled).  --normal-angle DEG: a point also needs a normal within DEG of the plane's (either sign); the
        normals are `align.scan_normals`': the faces' when the scan has any, else the covariance of the --normals-k (default 10) nearest
        points.  --level: DIR/<scene>/ is the scan with its vertices moved by `level_transform` of the largest plane (or plane INDEX) --
        faces and colours kept, segs.json and the aggregation file copied, T in the report.  --remove: DIR/<scene>/ is the scan without
        the points of any plane, as `components` writes a cleaned scan (<scene>.clean.npz holds kept, new_of_old and the plane of every raw
        vertex); what is made on it goes back to the raw scan with `python -m seggroup_amd.transfer --from-scans DIR --to-scans RAW`.
        The two are exclusive.  `--dist` and `--min-points` have no default: both depend on the scan's unit and density.

Not here: cylinders and spheres, region growing, early termination, merging of coplanar patches.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import shutil
import sys
from dataclasses import dataclass

import numpy as np

from . import hip, scans
from .device import cloud_box, device_rows, device_tensor, on_stream, stream_ptr, sync, torch_device, vec3, workspace

MAX_POINTS = 1 << 24
MAX_HYPOTHESES = 1 << 20
NPZ_SUFFIX = ".planes.npz"
REPORT_NAME = "planes_report.json"
PARAMETERS = ("dist", "max_planes", "min_points", "hypotheses", "seed", "min_edge", "min_sine", "normal_angle")


@dataclass
class Planes:
    """What detect_planes returns.  `labels` int32 [N]: the plane of every point, -1 for none.  Per plane p, in the order found: `planes`
    float64 [P,4] the refitted (n, d) with n.x + d = 0, `points` how many points carry p, `ransac_count` the winning hypothesis' count and
    `h` its index, `rms` the labelled-from inliers' rms distance to the refit, `centroid` float64 [P,3] their mean.  The rest are the
    parameters used."""
    labels: np.ndarray
    planes: np.ndarray
    points: np.ndarray
    ransac_count: np.ndarray
    h: np.ndarray
    rms: np.ndarray
    centroid: np.ndarray
    dist: float
    max_planes: int
    min_points: int
    hypotheses: int
    seed: int
    min_edge: float
    min_sine: float
    normal_angle: object = None

    def arrays(self) -> dict:
        """everything as arrays, as <scene>.planes.npz holds it (normal_angle: NaN when there is none)"""
        out = {k: getattr(self, k) for k in ("labels", "planes", "points", "ransac_count", "h", "rms", "centroid")}
        out.update(dist=np.float64(self.dist), max_planes=np.int32(self.max_planes), min_points=np.int32(self.min_points),
                   hypotheses=np.int32(self.hypotheses), seed=np.int64(self.seed), min_edge=np.float64(self.min_edge),
                   min_sine=np.float64(self.min_sine), normal_angle=np.float64(np.nan if self.normal_angle is None else self.normal_angle))
        return out


def _side(labels, normals, n: int, dev, who: str):
    """the optional per-point inputs on the device, checked -> (labels int32 [N] or None, normals float32 [N,3] or None)"""
    import torch
    d_lab = d_nrm = None
    if labels is not None:
        d_lab = device_tensor(labels, torch.int32, dev)
        if tuple(d_lab.shape) != (n,):
            raise ValueError("%s: labels must be [%d], not %r" % (who, n, tuple(d_lab.shape)))
    if normals is not None:
        d_nrm = device_tensor(normals, torch.float32, dev)
        if d_nrm.dim() != 2 or d_nrm.shape[0] != n or d_nrm.shape[1] < 3:
            raise ValueError("%s: one normal [3] per point (%r for %d points)" % (who, tuple(d_nrm.shape), n))
        d_nrm = d_nrm[:, :3].contiguous()
    return d_lab, d_nrm


def _plane4(plane, who: str) -> np.ndarray:
    p = np.ascontiguousarray(plane, dtype=np.float64)
    if p.shape != (4,):
        raise ValueError(f"{who}: a plane is 4 numbers (n, d)")
    return p


def plane_ransac(xyz, dist, hypotheses, seed=0, labels=None, min_edge=None, min_sine=0.1, triples=None, normals=None, min_cos=0.0, device=None,
                 stream=None):
    """sg_plane_ransac -> (count int32 [H], plane float64 [H,4] device tensors, free, best).  The FREE points are those with labels < 0 (all
    of them without labels); `triples` int32 [H,3] are positions in the list of free points in ascending index, None: generated on the
    device from `seed`.  count[h] = -1 and plane[h] = 0 for a rejected hypothesis; `best` is the h of the highest count, the lowest among
    equals, -1 when nothing was kept.  `min_edge` defaults to 10 * dist; `normals` [N, >= 3] with `min_cos` add |n.nrm| >= min_cos to the
    inlier test."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    h = int(hypotheses)
    min_edge = 10.0 * float(dist) if min_edge is None else float(min_edge)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "plane_ransac", MAX_POINTS)
        n = int(d_xyz.shape[0])
        d_lab, d_nrm = _side(labels, normals, n, dev, "plane_ransac")
        d_tri = None
        if triples is not None:
            d_tri = device_tensor(triples, torch.int32, dev)
            if tuple(d_tri.shape) != (h, 3):
                raise ValueError("plane_ransac: triples are [hypotheses, 3]")
        need = lib.sg_plane_ransac_ws_bytes(n, h, int(d_nrm is not None))
        if need == 0:
            raise hip.SgError(hip.SG_EUNSUP, "plane_ransac: %d points and %d hypotheses; a call takes at most 2^24 and 2^20" % (n, h))
        count = torch.empty(h, dtype=torch.int32, device=dev)
        plane = torch.empty((h, 4), dtype=torch.float64, device=dev)
        ws = workspace(need, dev)
        free, best = C.c_int(0), C.c_int(-1)
        hip.check_arg(lib.sg_plane_ransac(d_xyz.data_ptr() if n else None, int(d_xyz.shape[1]), n, hip.ptr(d_lab) if n else None,
                                          hip.ptr(d_nrm) if n else None, float(min_cos), h, int(seed) % (1 << 64),
                                          d_tri.data_ptr() if d_tri is not None and h else None, float(dist), min_edge, float(min_sine),
                                          count.data_ptr() if h else None, plane.data_ptr() if h else None, C.byref(free), C.byref(best),
                                          ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return count, plane, int(free.value), int(best.value)


def plane_moments(xyz, plane, dist, origin=None, labels=None, normals=None, min_cos=0.0, device=None, stream=None) -> np.ndarray:
    """sg_plane_moments over the free points within `dist` of `plane` (n, d) -> float64 [11]: count | sum q [3] | sum q q^T as xx xy xz yy
    yz zz | sum r^2, with q = p - origin and r = n.p + d in double.  Deterministic: the same input gives the same bytes."""
    import torch
    pl, o = _plane4(plane, "plane_moments"), vec3(origin, "plane_moments")
    dev = torch_device(device)
    lib = hip.lib()
    out = np.zeros(11, np.float64)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "plane_moments", MAX_POINTS)
        n = int(d_xyz.shape[0])
        d_lab, d_nrm = _side(labels, normals, n, dev, "plane_moments")
        ws = workspace(lib.sg_plane_moments_ws_bytes(n), dev)
        hip.check_arg(lib.sg_plane_moments(d_xyz.data_ptr() if n else None, int(d_xyz.shape[1]), n, hip.ptr(d_lab) if n else None,
                                           hip.ptr(d_nrm) if n else None, float(min_cos), pl.ctypes.data, float(dist), o.ctypes.data,
                                           out.ctypes.data, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return out


def plane_fit(m, origin=None):
    """sg_plane_fit (host only, runs without a GPU): the 11 moments and their origin -> (plane float64 [4], centroid float64 [3], rms): the
    least-squares plane, its normal's largest component positive.  Fewer than 3 points, or points on a line, raise hip.SgError
    (SG_EUNSUP, "degenerate"); a non-finite moment is a ValueError."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (11,):
        raise ValueError("plane_fit: 11 moments")
    o = vec3(origin, "plane_fit")
    plane, centroid, rms = np.zeros(4), np.zeros(3), C.c_double(0.0)
    hip.check_arg(hip.lib().sg_plane_fit(m.ctypes.data, o.ctypes.data, plane.ctypes.data, centroid.ctypes.data, C.byref(rms)))
    return plane, centroid, float(rms.value)


def plane_assign(xyz, labels, plane, dist, plane_id, normals=None, min_cos=0.0, device=None, stream=None):
    """sg_plane_assign: `plane_id` (>= 0) written at the free points within `dist` of `plane` -> (labels int32 [N] device tensor, how many
    were labelled).  An int32 tensor that is already on the device is updated in place and returned; anything else is copied first."""
    import torch
    pl = _plane4(plane, "plane_assign")
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "plane_assign", MAX_POINTS)
        n = int(d_xyz.shape[0])
        if labels is None:
            raise ValueError("plane_assign: labels [N] are needed (-1: free)")
        d_lab, d_nrm = _side(labels, normals, n, dev, "plane_assign")
        ws = workspace(lib.sg_plane_assign_ws_bytes(n), dev)
        done = C.c_int(0)
        hip.check_arg(lib.sg_plane_assign(d_xyz.data_ptr() if n else None, int(d_xyz.shape[1]), n, hip.ptr(d_nrm) if n else None, float(min_cos),
                                          pl.ctypes.data, float(dist), int(plane_id), d_lab.data_ptr() if n else None, C.byref(done),
                                          ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return d_lab, int(done.value)


def check_parameters(dist, min_points, max_planes=16, hypotheses=4096, min_edge=None, min_sine=0.1, normal_angle=None, has_normals=None):
    """what detect_planes and the command refuse before anything runs (ValueError) -> (dist, min_points, min_edge, min_cos)"""
    if min_points is None:
        raise ValueError("detect_planes: min_points (min_points=, --min-points) is required: the fewest points a plane may have depends on "
                         "the scan's density; there is no default")
    if dist is None or not (float(dist) > 0.0 and math.isfinite(float(dist))):
        raise ValueError("detect_planes: dist (dist=, --dist) must be a finite length > 0, in the scan's unit")
    if int(min_points) < 3:
        raise ValueError("detect_planes: min_points (--min-points) must be at least 3")
    if int(max_planes) < 1:
        raise ValueError("detect_planes: max_planes (--max-planes) must be at least 1")
    if not 1 <= int(hypotheses) <= MAX_HYPOTHESES:
        raise ValueError("detect_planes: hypotheses (--hypotheses) must be in 1..2^20")
    min_edge = 10.0 * float(dist) if min_edge is None else float(min_edge)
    if not (min_edge > 0.0 and math.isfinite(min_edge)):
        raise ValueError("detect_planes: min_edge (--min-edge) must be a finite length > 0")
    if not 0.0 < float(min_sine) <= 1.0:
        raise ValueError("detect_planes: min_sine must be in (0, 1]")
    min_cos = 0.0
    if normal_angle is not None:
        if not 0.0 <= float(normal_angle) <= 90.0:
            raise ValueError("detect_planes: normal_angle (--normal-angle) is an angle in 0..90 degrees")
        min_cos = math.cos(math.radians(float(normal_angle)))
    if has_normals is not None and has_normals != (normal_angle is not None):
        raise ValueError("detect_planes: normals and normal_angle go together: give both or neither")
    return float(dist), int(min_points), min_edge, min_cos


def detect_planes(xyz, dist, max_planes=16, min_points=None, hypotheses=4096, seed=0, min_edge=None, min_sine=0.1, normals=None,
                  normal_angle=None, device=None, stream=None) -> Planes:
    """The dominant planes of a cloud [N, >= 3], largest first as far as RANSAC finds them -> Planes (the module's docstring has the loop).
    `dist`: how far a point may lie from its plane; `min_points` (required): the fewest points of a plane; `min_edge` (default 10 * dist) and
    `min_sine`: the shortest edge and the smallest sine of the corner at the first point of a triple that may propose a plane;
    `normals` [N, >= 3] with `normal_angle` degrees: a point also needs a normal within that angle of the plane's, either sign."""
    import torch
    dist, min_points, min_edge, min_cos = check_parameters(dist, min_points, max_planes, hypotheses, min_edge, min_sine, normal_angle,
                                                           normals is not None)
    max_planes, hypotheses, seed, min_sine = int(max_planes), int(hypotheses), int(seed), float(min_sine)
    dev = torch_device(device)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "detect_planes", MAX_POINTS)
        n = int(d_xyz.shape[0])
        _, d_nrm = _side(None, normals, n, dev, "detect_planes")
        d_lab = torch.full((n,), -1, dtype=torch.int32, device=dev)
        origin = np.zeros(3)
        if n:
            lo, hi = cloud_box(d_xyz, "detect_planes")
            origin = 0.5 * (lo + hi)
    found = []
    for p in range(max_planes if n >= 3 else 0):
        count, plane, _, best = plane_ransac(d_xyz, dist, hypotheses, seed + p, d_lab, min_edge, min_sine, None, d_nrm, min_cos, dev, stream)
        if best < 0:
            break
        with torch.cuda.device(dev), on_stream(stream):
            votes, proposal = int(count[best]), plane[best].cpu().numpy()
        if votes < min_points:
            break
        m = plane_moments(d_xyz, proposal, dist, origin, d_lab, d_nrm, min_cos, dev, stream)
        try:
            fit, centroid, rms = plane_fit(m, origin)
        except hip.SgError as e:
            if e.code != hip.SG_EUNSUP:
                raise
            break
        with torch.cuda.device(dev), on_stream(stream):
            trial = d_lab.clone()
        trial, labelled = plane_assign(d_xyz, trial, fit, dist, p, d_nrm, min_cos, dev, stream)
        if labelled < min_points:
            break
        d_lab = trial
        found.append((fit, labelled, votes, best, rms, centroid))
    with torch.cuda.device(dev), on_stream(stream):
        labels = d_lab.cpu().numpy()
    col = lambda i, dtype, shape: np.array([f[i] for f in found], dtype=dtype).reshape(shape)
    return Planes(labels=labels, planes=col(0, np.float64, (-1, 4)), points=col(1, np.int64, (-1,)), ransac_count=col(2, np.int64, (-1,)),
                  h=col(3, np.int64, (-1,)), rms=col(4, np.float64, (-1,)), centroid=col(5, np.float64, (-1, 3)), dist=dist,
                  max_planes=max_planes, min_points=min_points, hypotheses=hypotheses, seed=seed, min_edge=min_edge, min_sine=min_sine,
                  normal_angle=None if normal_angle is None else float(normal_angle))


def level_index(planes: Planes, which="largest") -> int:
    """the plane `which` names: "largest" (most points, the first found among equals) or an index into the planes found"""
    count = int(planes.planes.shape[0])
    if count == 0:
        raise ValueError("level_transform: no plane was found; there is nothing to level on")
    if which == "largest":
        return int(np.argmax(planes.points))
    if isinstance(which, (int, np.integer)) and not isinstance(which, bool) and 0 <= int(which) < count:
        return int(which)
    raise ValueError("level_transform: which (--level) is 'largest' or an index in 0..%d, not %r" % (count - 1, which))


def level_transform(planes: Planes, xyz, which="largest") -> np.ndarray:
    """The rigid transform that levels the cloud on one of its planes -> T float64 [4,4], for `align.apply`: T x = R (x - c) + (c_x, c_y,
    0) with c the plane's centroid and R the smallest rotation that takes the plane's normal onto +z (the antiparallel case: a half turn
    about x).  The normal is first turned so that the mean of `xyz` [N, >= 3] lies on its positive side: a floor has its room above it.
    Host double arithmetic."""
    i = level_index(planes, which)
    pts = np.asarray(xyz.detach().cpu().numpy() if hasattr(xyz, "detach") else xyz, dtype=np.float64)[:, :3]
    if pts.ndim != 2 or pts.shape[0] < 1:
        raise ValueError("level_transform: xyz is the cloud the planes were found in, [N >= 1, >= 3]")
    n = planes.planes[i, :3] / np.linalg.norm(planes.planes[i, :3])
    c = planes.centroid[i]
    if float(np.dot(n, pts.mean(0) - c)) < 0.0:
        n = -n
    v = np.array([n[1], -n[0], 0.0])                                     # n x z
    s2, cth = float(v @ v), float(n[2])
    if s2 < 1e-30:
        R = np.eye(3) if cth > 0.0 else np.diag([1.0, -1.0, -1.0])
    else:
        K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
        R = np.eye(3) + K + (K @ K) * ((1.0 - cth) / s2)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.array([c[0], c[1], 0.0]) - R @ c
    return T


# ---- scans ----------------------------------------------------------------------------------------------------------------------------
def _level_arg(text):
    if text == "largest":
        return text
    try:
        i = int(text)
    except ValueError:
        i = -1
    if i < 0:
        raise argparse.ArgumentTypeError("largest or a plane index >= 0 is needed, not %s" % text)
    return i


def check_command(level, remove, normal_angle, normals_k) -> None:
    """the combinations of the command's options that are refused before anything runs (ValueError)"""
    if level is not None and remove:
        raise ValueError("--level and --remove each write the scan directory: give one")
    if normals_k is not None:
        if normal_angle is None:
            raise ValueError("--normals-k needs --normal-angle: without it no normals are made")
        if int(normals_k) < 3:
            raise ValueError("--normals-k must be at least 3")


def planes_scan(scene_path: str, out_dir: str, dist, min_points, max_planes=16, hypotheses=4096, seed=0, min_edge=None, normal_angle=None,
                normals_k=None, level=None, remove: bool = False, force: bool = False, device=None, stream=None):
    """One scan directory -> <out_dir>/<scene>.planes.npz (and, with `level` or `remove`, the scan directory <out_dir>/<scene>/) -> its
    entry of planes_report.json, or None when the .npz was there already (never overwritten without `force`)."""
    import torch
    from .prepare import mesh_arrays, read_ply, write_ply
    check_command(level, remove, normal_angle, normals_k)
    check_parameters(dist, min_points, max_planes, hypotheses, min_edge, 0.1, normal_angle)
    scene = scans.scene_name(scene_path)
    npz = os.path.join(out_dir, scene + NPZ_SUFFIX)
    if os.path.exists(npz) and not force:
        return None
    xyz, rgb, faces = mesh_arrays(read_ply(os.path.join(scene_path, scene + scans.PLY_SUFFIX)))
    nrm, how = None, None
    if normal_angle is not None:
        from .align import scan_normals
        nrm, how = scan_normals(xyz, faces, 10 if normals_k is None else int(normals_k), device=device)
    found = detect_planes(xyz, dist, max_planes, min_points, hypotheses, seed, min_edge, normals=nrm, normal_angle=normal_angle, device=device,
                          stream=stream)
    os.makedirs(out_dir, exist_ok=True)
    np.savez(npz, **found.arrays())
    entry = {"V": int(xyz.shape[0]), "unlabelled": int((found.labels < 0).sum()),
             "planes": [{"equation": [float(v) for v in found.planes[p]], "points": int(found.points[p]), "rms": float(found.rms[p])}
                        for p in range(found.planes.shape[0])]}
    if how is not None:
        entry["normals"] = how
    dst = os.path.join(out_dir, scene)
    if level is not None:
        entry["T"] = None
        if found.planes.shape[0]:
            from .align import apply
            i = level_index(found, level)
            T = level_transform(found, xyz, i)
            with torch.cuda.device(torch_device(device)):
                moved = apply(xyz, T, device=device, stream=stream).cpu().numpy()
            os.makedirs(dst, exist_ok=True)
            write_ply(os.path.join(dst, scene + scans.PLY_SUFFIX), moved, rgb, faces)
            for name in (scans.segs_json_name(scene), scene + ".aggregation.json"):
                if os.path.exists(os.path.join(scene_path, name)):
                    shutil.copyfile(os.path.join(scene_path, name), os.path.join(dst, name))
            entry.update(T=[[float(v) for v in row] for row in T], level=i)
    if remove:
        from .components import clean_arrays, kept_segs, write_kept_scan
        dev = torch_device(device)
        with torch.cuda.device(dev), on_stream(stream):
            d_kept, d_new, d_faces = clean_arrays(torch.from_numpy(found.labels < 0).to(dev), torch.from_numpy(faces).to(dev))
            kept, new_of_old, new_faces = d_kept.cpu().numpy(), d_new.cpu().numpy(), d_faces.cpu().numpy()
        doc, _ = kept_segs(scene_path, scene, int(xyz.shape[0]), kept)
        write_kept_scan(scene_path, dst, scene, xyz, rgb, kept, new_of_old, new_faces, doc, plane=found.labels, planes=found.planes,
                        dist=np.float64(found.dist), min_points=np.int32(found.min_points))
        entry.update(M=int(kept.shape[0]), kept_F=int(new_faces.shape[0]))
    return entry


def planes_scans(scans_dir: str, out_dir: str, dist, min_points, scenes=None, workers: int = 4, device=None, **options):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    <out_dir>/planes_report.json.  Workers are threads, each with its own stream; `options` are planes_scan's."""
    check_command(options.get("level"), options.get("remove", False), options.get("normal_angle"), options.get("normals_k"))
    check_parameters(dist, min_points, options.get("max_planes", 16), options.get("hypotheses", 4096), options.get("min_edge"), 0.1,
                     options.get("normal_angle"))
    dev = torch_device(device)
    head = {"dist": float(dist), "min_points": int(min_points)}
    head.update({k: v for k, v in options.items() if v is not None and k != "force"})
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, head,
                           lambda path, stream: planes_scan(path, out_dir, dist, min_points, device=dev, stream=stream, **options))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.planes", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--out", required=True, help="where <scene>.planes.npz, planes_report.json and the written scan directories go")
    ap.add_argument("--dist", type=float, required=True, help="how far a point may lie from its plane, in the scan's unit; there is no default")
    ap.add_argument("--min-points", type=int, required=True, help="the fewest points of a plane; there is no default")
    ap.add_argument("--max-planes", type=int, default=16, help="rounds at most (default 16)")
    ap.add_argument("--hypotheses", type=int, default=4096, help="triples per round, at most 2^20 (default 4096)")
    ap.add_argument("--seed", type=int, default=0, help="the seed of the first round's triples; round p uses seed + p (default 0)")
    ap.add_argument("--min-edge", type=float, default=None, help="the shortest edge of a triple that may propose a plane (default 10 * dist)")
    ap.add_argument("--normal-angle", type=float, default=None, metavar="DEG",
                    help="a point also needs a normal within DEG degrees of the plane's (the scan's faces, else its kNN covariance)")
    ap.add_argument("--normals-k", type=int, default=None, metavar="K", help="the neighbours of the kNN covariance normals (--normal-angle only; default 10)")
    ap.add_argument("--level", nargs="?", const="largest", default=None, type=_level_arg, metavar="largest|INDEX",
                    help="write the scan levelled on its largest plane (or on plane INDEX): that plane at z = 0, the scan above it")
    ap.add_argument("--remove", action="store_true", help="write the scan without the points of any plane")
    scans.add_batch_arguments(ap, "overwrite existing results")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    try:
        check_command(a.level, a.remove, a.normal_angle, a.normals_k)
        check_parameters(a.dist, a.min_points, a.max_planes, a.hypotheses, a.min_edge, 0.1, a.normal_angle)
    except ValueError as e:
        ap.error(str(e))
    report, skipped = planes_scans(a.scans, a.out, a.dist, a.min_points, scans.scene_list(a.scenes), a.workers, a.device, max_planes=a.max_planes,
                                   hypotheses=a.hypotheses, seed=a.seed, min_edge=a.min_edge, normal_angle=a.normal_angle,
                                   normals_k=a.normals_k, level=a.level, remove=a.remove, force=a.force)
    scans.print_outcome(report, skipped, lambda scene, e: ("planes", scene, e["V"], "vertices,", len(e["planes"]), "planes,", e["unlabelled"],
                                                           "unlabelled"), "(its .planes.npz exists; --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
