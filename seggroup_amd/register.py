"""Global (init-free) registration of two clouds: FPFH descriptors, their nearest neighbours and a hypothesise-and-count
RANSAC that leaves a coarse pose inside `align.icp`'s basin.

`align.icp` refines a pose that is already within a few decimetres.  A photogrammetry cloud beside a laser scan, a re-export in another
pose or a second sensor's cloud arrive in arbitrary frames; `global_registration` finds the pose that ICP then starts from:

    thin both clouds (thin.thin_cloud)                      -- voxel=H; the radii then default to 2H (normals), 5H (features), 1.5H (inliers)
    radius lists and covariance normals per cloud           -- components.radius_neighbours, oversegment.pointcloud_normals; the viewpoint
                                                               is the cloud's own box centre, which moves with the cloud
    fpfh            sg_fpfh             33 bins per point   -- one wave per point, double arithmetic, integer histograms
    feature_nearest sg_feature_nearest  moving -> fixed     -- brute force in fp32, bit-equal to the NumPy statement
    ransac_count    sg_ransac_count     2^20 triples        -- generated, pre-rejected and compacted in one kernel, counted in a second
    the `verify` best by count are re-scored against the whole fixed cloud (align.apply + prepare.nearest_point_grid): most points within
    max_dist wins, ties to the better rank

Every stage is deterministic: the same input and seed give the same Coarse.  Not here: scale, other descriptors, a learned matcher, clouds
above 2^18 points after thinning (thin harder).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import align, hip
from .device import device_rows, device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

BINS = 33
MAX_POINTS = 1 << 18
MAX_HYPOTHESES = 1 << 24
COARSE_SCALARS = ("h", "count", "verified_inliers", "correspondences", "survivors", "hypotheses", "seed", "verify", "mutual", "voxel",
                  "normal_radius", "feature_radius", "max_dist", "min_edge", "similarity", "moving_points", "fixed_points")


@dataclass
class Coarse:
    """What global_registration returns.  `T` [4,4] float64 maps MOVING coordinates into the FIXED cloud's frame; `h` is the winning
    hypothesis, `count` its correspondence count, `verified_inliers` the moving points (after thinning) it brings within max_dist of the
    fixed cloud; `correspondences` and `survivors` size the RANSAC's input and what passed its pre-rejection; the rest are the
    parameters used."""
    T: np.ndarray
    h: int
    count: int
    verified_inliers: int
    correspondences: int
    survivors: int
    hypotheses: int
    seed: int
    verify: int
    mutual: bool
    voxel: object
    normal_radius: float
    feature_radius: float
    max_dist: float
    min_edge: float
    similarity: float
    moving_points: int
    fixed_points: int
    ranked: list = field(default_factory=list)             # (h, count, verified inliers) of every verified hypothesis, best count first

    def scalars(self) -> dict:
        return {k: getattr(self, k) for k in COARSE_SCALARS}


def fpfh(xyz, normals, radius, lists=None, want_spfh=False, device=None, stream=None):
    """sg_fpfh -> float32 [N,33] device tensor (with want_spfh: also the int32 [N,34] bin counts and pair count).  xyz [N, >= 3], normals
    [N,3]; the neighbourhoods are `lists` = (indptr int64 [N+1], indices int32 [T]) or components.radius_neighbours(xyz, radius).  Lists
    that do not hold together are a ValueError."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "fpfh")
        n = int(d_xyz.shape[0])
        d_nrm = device_tensor(normals, torch.float32, dev)
        if tuple(d_nrm.shape) != (n, 3):
            raise ValueError("fpfh: one normal [3] per point (%r for %d points)" % (tuple(d_nrm.shape), n))
        hist = torch.zeros((n, BINS + 1), dtype=torch.int32, device=dev)
        out = torch.zeros((n, BINS), dtype=torch.float32, device=dev)
        if n:
            if lists is None:
                from .components import radius_neighbours
                lists = radius_neighbours(d_xyz, radius, device=dev, stream=stream)
            indptr, indices = device_tensor(lists[0], torch.int64, dev), device_tensor(lists[1], torch.int32, dev)
            if indptr.dim() != 1 or indptr.shape[0] != n + 1 or indices.dim() != 1:
                raise ValueError("fpfh: lists are (indptr [N + 1], indices [T])")
            if int(indptr[-1]) != indices.shape[0]:
                raise ValueError("fpfh: indptr[N] = %d, and indices holds %d entries" % (int(indptr[-1]), indices.shape[0]))
            ws = workspace(lib.sg_fpfh_ws_bytes(n), dev)
            hip.check_arg(lib.sg_fpfh(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, d_nrm.data_ptr(), indptr.data_ptr(),
                                      indices.data_ptr() if indices.numel() else None, hist.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      stream_ptr(stream)))
        sync(stream)
    return (out, hist) if want_spfh else out


def feature_nearest(a, b, device=None, stream=None):
    """sg_feature_nearest: for every row of a [U,C] its nearest row of b [N,C] in squared fp32 distance, the lowest index among equals ->
    (idx int64 [U], d2 float32 [U]) device tensors.  1 <= C <= 64; more than 2^18 rows on either side is an hip.SgError (SG_EUNSUP)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_a, d_b = device_tensor(a, torch.float32, dev), device_tensor(b, torch.float32, dev)
        if d_a.dim() != 2 or d_b.dim() != 2 or d_a.shape[1] != d_b.shape[1]:
            raise ValueError("feature_nearest: a [U,C] and b [N,C] with the same C")
        u, n, c = int(d_a.shape[0]), int(d_b.shape[0]), int(d_a.shape[1])
        idx = torch.empty(u, dtype=torch.int64, device=dev)
        d2 = torch.empty(u, dtype=torch.float32, device=dev)
        hip.check_arg(lib.sg_feature_nearest(d_a.data_ptr() if u else None, u, d_b.data_ptr() if n else None, n, c, idx.data_ptr() if u else None,
                                             d2.data_ptr() if u else None, stream_ptr(stream)))
        sync(stream)
    return idx, d2


def ransac_count(moving, fixed, ci, cj, hypotheses, max_dist, seed=0, similarity=0.9, min_edge=None, triples=None, device=None, stream=None,
                 want_survivors=False):
    """sg_ransac_count -> int32 [H] device tensor: per hypothesis the number of correspondences (moving[ci[c]], fixed[cj[c]]) its pose brings
    within max_dist, -1 for a hypothesis the pre-rejection dropped (with want_survivors: also the number that were counted).  `triples`
    int32 [H,3] index the correspondences; None: generated on the device from `seed`.  `min_edge` defaults to 3 * max_dist."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    h = int(hypotheses)
    min_edge = 3.0 * float(max_dist) if min_edge is None else float(min_edge)
    with torch.cuda.device(dev), on_stream(stream):
        d_m, d_f = device_rows(moving, dev, "ransac_count"), device_rows(fixed, dev, "ransac_count")
        d_ci, d_cj = device_tensor(ci, torch.int32, dev), device_tensor(cj, torch.int32, dev)
        c = int(d_ci.shape[0])
        if d_ci.dim() != 1 or tuple(d_cj.shape) != (c,):
            raise ValueError("ransac_count: ci and cj hold one index per correspondence")
        if c < 3:
            raise ValueError("ransac_count: %d correspondences; a pose needs at least 3" % c)
        d_tri = None
        if triples is not None:
            d_tri = device_tensor(triples, torch.int32, dev)
            if tuple(d_tri.shape) != (h, 3):
                raise ValueError("ransac_count: triples are [hypotheses, 3]")
        need = lib.sg_ransac_ws_bytes(c, h)
        if need == 0:
            raise hip.SgError(hip.SG_EUNSUP, "ransac_count: %d correspondences and %d hypotheses; a call takes at most 2^18 and 2^24" % (c, h))
        count = torch.empty(h, dtype=torch.int32, device=dev)
        ws = workspace(need, dev)
        surv = C.c_int(0)
        hip.check_arg(lib.sg_ransac_count(d_m.data_ptr(), int(d_m.shape[1]), int(d_m.shape[0]), d_f.data_ptr(), int(d_f.shape[1]),
                                          int(d_f.shape[0]), d_ci.data_ptr(), d_cj.data_ptr(), c, h, int(seed) % (1 << 64),
                                          d_tri.data_ptr() if d_tri is not None and h else None, float(max_dist), float(similarity), min_edge,
                                          count.data_ptr() if h else None, C.byref(surv), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return (count, int(surv.value)) if want_survivors else count


def triangle_pose(a, b) -> np.ndarray:
    """sg_triangle_pose (host only, runs without a GPU): two triangles [3,3] (rows x0, x1, x2) -> T float64 [4,4], the pose whose rotation
    carries a's frame onto b's and whose translation carries a's centroid onto b's -- the function the RANSAC kernel runs.  A triangle
    without a frame raises hip.SgError (SG_EUNSUP, "degenerate")."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != (3, 3) or b.shape != (3, 3):
        raise ValueError("triangle_pose: a triangle is [3,3]")
    T = np.eye(4)
    hip.check_arg(hip.lib().sg_triangle_pose(a.ctypes.data, b.ctypes.data, T.ctypes.data))
    return T


def splitmix_triple(seed: int, h: int, c: int):
    """the triple the device generates for hypothesis h of c correspondences (Python integers, modulo 2^64)"""
    out, mask = [], (1 << 64) - 1
    for e in range(3):
        z = (int(seed) + (3 * int(h) + e + 1) * 0x9E3779B97F4A7C15) & mask
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        out.append(((z >> 32) * int(c)) >> 32)
    return out


def check_parameters(voxel, normal_radius, feature_radius, max_dist, hypotheses, verify):
    """what global_registration refuses before anything runs (ValueError) -> (normal_radius, feature_radius, max_dist)"""
    if voxel is not None:
        if not float(voxel) > 0.0:
            raise ValueError("global_registration: voxel must be a length > 0 (or None with the three radii given)")
        v = float(voxel)
        normal_radius = 2.0 * v if normal_radius is None else normal_radius
        feature_radius = 5.0 * v if feature_radius is None else feature_radius
        max_dist = 1.5 * v if max_dist is None else max_dist
    elif normal_radius is None or feature_radius is None or max_dist is None:
        raise ValueError("global_registration: without voxel, normal_radius, feature_radius and max_dist are all required")
    radii = tuple(float(r) for r in (normal_radius, feature_radius, max_dist))
    if not all(r > 0.0 and np.isfinite(r) for r in radii):
        raise ValueError("global_registration: normal_radius, feature_radius and max_dist must be finite lengths > 0")
    if not 1 <= int(hypotheses) <= MAX_HYPOTHESES:
        raise ValueError("global_registration: hypotheses must be in 1..2^24")
    if int(verify) < 1:
        raise ValueError("global_registration: verify must be at least 1")
    return radii


def _describe(d_xyz, normal_radius, feature_radius, viewpoint, dev, stream):
    """one cloud [N,3] on the device -> its float32 [N,33] descriptors"""
    from .components import radius_neighbours
    from .oversegment import pointcloud_normals
    nrm = pointcloud_normals(d_xyz, radius=normal_radius, viewpoint=viewpoint, device=dev,
                             lists=radius_neighbours(d_xyz, normal_radius, device=dev, stream=stream))
    return fpfh(d_xyz, nrm, feature_radius, device=dev, stream=stream)


def global_registration(moving_xyz, fixed_xyz, voxel=None, normal_radius=None, feature_radius=None, max_dist=None, hypotheses=2 ** 20, seed=0,
                        verify=16, mutual=False, viewpoint_moving=None, viewpoint_fixed=None, similarity=0.9, min_edge=None, device=None,
                        stream=None) -> Coarse:
    """The coarse pose of the MOVING cloud in the FIXED cloud's frame, from nothing -> Coarse (the module's docstring has the stages).
    `voxel=H` thins both clouds first and sets the radii that are not given to 2H, 5H and 1.5H; `voxel=None` thins nothing and needs all
    three.  `min_edge` defaults to 3 * max_dist.  ValueError, naming the parameter to change: fewer than 3 correspondences
    (feature_radius), no surviving hypothesis (hypotheses / min_edge), a cloud above 2^18 points after thinning (voxel)."""
    import torch
    normal_radius, feature_radius, max_dist = check_parameters(voxel, normal_radius, feature_radius, max_dist, hypotheses, verify)
    min_edge = 3.0 * max_dist if min_edge is None else float(min_edge)
    hypotheses, verify = int(hypotheses), int(verify)
    dev = torch_device(device)
    clouds = []
    with torch.cuda.device(dev), on_stream(stream):
        for name, xyz in (("moving", moving_xyz), ("fixed", fixed_xyz)):
            d = device_rows(xyz, dev, "global_registration")[:, :3].contiguous()
            if d.shape[0] < 3:
                raise ValueError("global_registration: the %s cloud has %d points; a pose needs at least 3" % (name, d.shape[0]))
            if voxel is not None:
                from .thin import thin_cloud
                d = d[thin_cloud(d, float(voxel), device=dev, stream=stream)[0].long()].contiguous()
            if d.shape[0] > MAX_POINTS:
                raise ValueError("global_registration: the %s cloud has %d points%s; the descriptor search takes at most 2^18 -- a larger voxel"
                                 % (name, d.shape[0], " after thinning" if voxel is not None else ""))
            clouds.append(d)
    d_mov, d_fix = clouds
    f_mov = _describe(d_mov, normal_radius, feature_radius, viewpoint_moving, dev, stream)
    f_fix = _describe(d_fix, normal_radius, feature_radius, viewpoint_fixed, dev, stream)
    with torch.cuda.device(dev), on_stream(stream):
        um, uf = (torch.nonzero((f != 0).any(1)).reshape(-1) for f in (f_mov, f_fix))
        ci = cj = torch.zeros(0, dtype=torch.int64, device=dev)
        if um.numel() and uf.numel():
            fm, ff = f_mov[um].contiguous(), f_fix[uf].contiguous()
            near, _ = feature_nearest(fm, ff, device=dev, stream=stream)
            ci, cj = um, uf[near]
            if mutual:
                back, _ = feature_nearest(ff, fm, device=dev, stream=stream)
                ok = back[near] == torch.arange(um.numel(), device=dev)
                ci, cj = ci[ok], cj[ok]
        c = int(ci.numel())
    if c < 3:
        raise ValueError("global_registration: %d correspondences; a pose needs at least 3 -- a larger feature_radius (or voxel), or "
                         "mutual=False" % c)
    count, survivors = ransac_count(d_mov, d_fix, ci, cj, hypotheses, max_dist, seed=seed, similarity=similarity, min_edge=min_edge, device=dev,
                                    stream=stream, want_survivors=True)
    if survivors == 0:
        raise ValueError("global_registration: none of the %d hypotheses passed the pre-rejection -- more hypotheses, or a smaller min_edge "
                         "(%g)" % (hypotheses, min_edge))
    with torch.cuda.device(dev), on_stream(stream):
        # a unique key per hypothesis: the count first, the lower h the larger among equal counts
        key = count.long() * hypotheses + (hypotheses - 1 - torch.arange(hypotheses, device=dev))
        top = torch.topk(key, min(verify, survivors)).values
        best_h = (hypotheses - 1 - top % hypotheses).cpu().numpy()
        best_count = (top // hypotheses).cpu().numpy()
        h_ci, h_cj = ci.cpu().numpy(), cj.cpu().numpy()
        h_mov, h_fix = d_mov.double().cpu().numpy(), d_fix.double().cpu().numpy()
    max_d2 = float(np.float32(max_dist * max_dist))
    ranked, best = [], None
    for h, n_count in zip(best_h.tolist(), best_count.tolist()):
        tri = splitmix_triple(seed, h, c)
        T = triangle_pose(h_mov[h_ci[tri]], h_fix[h_cj[tri]])
        moved = align.apply(d_mov, T, device=dev, stream=stream)
        from .prepare import nearest_point_grid
        _, d2 = nearest_point_grid(moved, d_fix, device=dev, stream=stream)
        with torch.cuda.device(dev), on_stream(stream):
            inliers = int((d2 <= max_d2).sum())
        ranked.append((int(h), int(n_count), inliers))
        if best is None or inliers > best[0]:
            best = (inliers, int(h), int(n_count), T)
    inliers, h, n_count, T = best
    return Coarse(T=T, h=h, count=n_count, verified_inliers=inliers, correspondences=c, survivors=int(survivors), hypotheses=hypotheses,
                  seed=int(seed), verify=verify, mutual=bool(mutual), voxel=None if voxel is None else float(voxel), normal_radius=normal_radius,
                  feature_radius=feature_radius, max_dist=max_dist, min_edge=min_edge, similarity=float(similarity),
                  moving_points=int(d_mov.shape[0]), fixed_points=int(d_fix.shape[0]), ranked=ranked)
