"""The voxel thinning's specification restated in NumPy float32 -- the reference that sg_cloud_thin is held to bit for bit
(tests/test_thin_ref.py, tests/test_gpu_thin.py, tools/capture_thin.py, tools/time_thin.py).

Every array is float32 and every operation is one NumPy call on float32 operands, so each is rounded once, in the order the specification
writes it; NumPy's float32 division is correctly rounded.  `thin` sorts; `thin_by_loop` is a second formulation, a plain loop over the
voxels that takes each one's argmin.  Nothing here calls the library.
"""
import hashlib

import numpy as np

import pcseg_ref

F32 = np.float32
CELL_LIMIT = F32(2097152.0)                                     # 2^21 cells per axis
VOXELS = (0.02, 0.05, 0.075, 0.2)
NS_AT_TILE_EDGES = (2047, 2048, 2049, 4095, 4096, 4097)         # the scan tile and the sort tile of sort_device.h


class CellRange(ValueError):
    """step 2: voxel too small for the cloud's extent"""


def box_min(x):
    """step 1: the minimum per axis; where it is zero and one of the zeros is -0.0, it is -0.0 (the order of the bit patterns: no result
    depends on the sign of that zero, only the returned `lo` shows it)"""
    lo = x.min(0).astype(F32)
    for a in range(3):
        if lo[a] == 0 and np.signbit(x[x[:, a] == 0, a]).any():
            lo[a] = F32(-0.0)
    return lo


def cells(xyz, voxel):
    """steps 1, 2, 4 -> (lo [3] f32, c [N,3] f32 holding integers, d2 [N] f32)"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    h = F32(voxel)
    if x.shape[0] < 1 or not np.isfinite(x).all() or not (np.isfinite(h) and h > 0):
        raise ValueError("thin: a finite cloud of at least one point and a finite voxel edge > 0")
    lo = box_min(x)
    with np.errstate(all="ignore"):
        q = (x - lo) / h
        if not (q < CELL_LIMIT).all():
            raise CellRange("voxel too small for the cloud's extent")
        c = np.floor(q)
        ctr = lo + (c + F32(0.5)) * h
        d = x - ctr
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert q.dtype == F32 and ctr.dtype == F32 and d2.dtype == F32
    return lo, c, d2


def voxel_key(c):
    ci = c.astype(np.int64)
    return (ci[:, 2] << 42) | (ci[:, 1] << 21) | ci[:, 0]


def _outputs(rep_of_point):
    """step 6 from every point's representative"""
    n = rep_of_point.shape[0]
    rep = np.unique(rep_of_point)
    rank = np.full(n, -1, np.int64)
    rank[rep] = np.arange(rep.shape[0])
    return rep.astype(np.int32), rank[rep_of_point].astype(np.int32)


def thin(xyz, voxel):
    """-> (rep int32 [M] ascending, thin_of_point int32 [N], lo f32 [3])"""
    lo, c, d2 = cells(xyz, voxel)
    n = c.shape[0]
    key = voxel_key(c)
    order = np.lexsort((np.arange(n), d2.view(np.uint32), key))            # d2 >= 0 or +inf: its bits ascend with it
    ks = key[order]
    head = np.ones(n, bool)
    head[1:] = ks[1:] != ks[:-1]
    rep_by_voxel = order[head]
    rep_of_point = np.empty(n, np.int64)
    rep_of_point[order] = rep_by_voxel[np.cumsum(head) - 1]
    return _outputs(rep_of_point) + (lo,)


def thin_by_loop(xyz, voxel):
    """the same outputs by a loop over the voxels: members in ascending index, the first strict minimum of d2"""
    lo, c, d2 = cells(xyz, voxel)
    members = {}
    for i, cell in enumerate(map(tuple, c.astype(np.int64).tolist())):
        members.setdefault(cell, []).append(i)
    rep_of_point = np.empty(c.shape[0], np.int64)
    for idx in members.values():
        best = idx[0]
        for i in idx[1:]:
            if d2[i] < d2[best]:
                best = i
        rep_of_point[idx] = best
    return _outputs(rep_of_point) + (lo,)


def lift(values, thin_of_point):
    return np.asarray(values)[np.asarray(thin_of_point)]


def segment_thinned(xyz, voxel, k=10, k_thresh=0.01, seg_min_verts=20):
    """thin, segment the thinned cloud by the statement of 8f, lift -> (ids int32 [N] = rep[seg_thin[thin_of_point]], ids of the thinned
    cloud [M], rep, thin_of_point)"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    rep, top, _ = thin(x, voxel)
    seg_thin = pcseg_ref.segment_pointcloud(x[rep], k, k_thresh, seg_min_verts)
    return rep[seg_thin[top]].astype(np.int32), seg_thin, rep, top


def stats(xyz, voxel, rep, thin_of_point):
    """cells per axis and the largest voxel population, as thin_report.json holds them"""
    _, c, _ = cells(xyz, voxel)
    return [int(v) + 1 for v in c.max(0)], int(np.bincount(thin_of_point, minlength=rep.shape[0]).max())


def array_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


# ---- the clouds ------------------------------------------------------------------------------------------------------------------------
TIE = np.array([[0, 0, 0], [0.25, 0.5, 0.5], [0.75, 0.5, 0.5]], F32)       # at h = 1: points 1 and 2 are equally far from the centre
BIG_COPIES, BIG_SEED, BIG_SHIFT = 50, 7, 0.004


CASE_NAMES = ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup", "n_k_plus_1", "n255", "n256", "n257", "line", "all_equal", "room_20k", "one_point",
              "tie"] + ["room_20k[:%d]" % n for n in NS_AT_TILE_EDGES]


def case_clouds():
    """name -> xyz f32 [N,3]: pcseg_ref's clouds, one point, the crafted tie, and room_20k cut at the tile edges"""
    out = {name: xyz for name, (xyz, _) in pcseg_ref.case_clouds(include_large=True).items()}
    out["one_point"] = out["room_j0"][:1].copy()
    out["tie"] = TIE.copy()
    for n in NS_AT_TILE_EDGES:
        out["room_20k[:%d]" % n] = np.ascontiguousarray(out["room_20k"][:n])
    return out


def big_cloud():
    """room_20k 50 times, every copy shifted by its own offset in [0, 0.004)^3 -> (xyz f32 [1058050,3], plane ids): more points than
    SG_MAX_POINTS, 5,403 voxels at h = 0.05, up to 350 points in one"""
    xyz, plane = pcseg_ref.case_clouds(include_large=True)["room_20k"]
    rng = np.random.default_rng(BIG_SEED)
    off = (rng.random((BIG_COPIES, 1, 3), dtype=F32) * F32(BIG_SHIFT)).astype(F32)
    return np.ascontiguousarray((xyz[None, :, :] + off).reshape(-1, 3).astype(F32)), np.tile(plane, BIG_COPIES)
