"""Rigid alignment of two clouds (seggroup_amd/align.py) restated in NumPy: the element-wise `apply`, the 17 sums with
np.sum in float64, Kabsch with np.linalg.svd, and the ICP loop with the search taken from nearest_grid_ref (the plain statement, which
the device search equals bit for bit, so correspondences compare as integers).  `room` is the deterministic synthetic scene of
tests/test_align_ref.py and tests/test_gpu_align.py.  Nothing here calls the library.
"""
import math

import numpy as np

import nearest_grid_ref as NG

F32, F64 = np.float32, np.float64
LINE_RATIO = 2.0 ** -40
AXIS = (0.3, -0.5, 1.0)
POSES = {"3deg_4cm": (3.0, 0.04), "10deg_15cm": (10.0, 0.15)}       # degrees about AXIS, metres along SHIFT_DIR
SHIFT_DIR = (0.6, -0.64, 0.48)                                      # a unit vector


def as_T(T):
    T = np.asarray(T, F64)
    out = np.eye(4)
    out[:3] = T[:3]
    return out


def pose(deg, shift, axis=AXIS, direction=SHIFT_DIR):
    """Rodrigues' rotation of `deg` degrees about `axis` through the origin, then `shift` metres along `direction` -> float64 [4,4]"""
    k = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
    a = math.radians(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T[:3, 3] = shift * np.asarray(direction, F64)
    return T


def inverse(T):
    T = as_T(T)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def apply(xyz, T):
    """out[u][r] = (float32)(((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r]), the coordinates widened to float64, element-wise"""
    p = np.asarray(xyz, F32)[:, :3].astype(F64)
    T = as_T(T)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(F32) for r in range(3)], 1)


def max_d2_of(max_dist):
    return F32(float(max_dist) * float(max_dist))


def moment_terms(x, y, idx, d2, max_dist, origin_x=(0, 0, 0), origin_y=(0, 0, 0)):
    """the terms of the 17 sums over the inlier pairs -> float64 [n, 17] (column 0 is all ones)"""
    d2 = np.asarray(d2, F32)
    with np.errstate(invalid="ignore"):
        sel = d2 <= max_d2_of(max_dist)
    a = np.asarray(x, F32)[:, :3].astype(F64)[sel] - np.asarray(origin_x, F64)
    b = np.asarray(y, F32)[:, :3].astype(F64)[np.asarray(idx)[sel]] - np.asarray(origin_y, F64)
    ab = (a[:, :, None] * b[:, None, :]).reshape(-1, 9)
    return np.concatenate([np.ones((a.shape[0], 1)), a, b, ab, d2[sel].astype(F64)[:, None]], 1)


def moments(x, y, idx, d2, max_dist, origin_x=(0, 0, 0), origin_y=(0, 0, 0)):
    """-> (the 17 sums float64 [17], the sums of the terms' absolute values float64 [17]: what bounds the distance between two summation
    orders of the same terms)"""
    t = moment_terms(x, y, idx, d2, max_dist, origin_x, origin_y)
    return t.sum(0), np.abs(t).sum(0)


class Degenerate(ValueError):
    pass


def solve(m, origin_x=(0, 0, 0), origin_y=(0, 0, 0)):
    """Kabsch from the moments with LAPACK's SVD -> float64 [4,4]; fewer than 3 pairs or pairs on a line raise Degenerate"""
    m = np.asarray(m, F64)
    n, sa, sb, sab = m[0], m[1:4], m[4:7], m[7:16].reshape(3, 3)
    if n < 3:
        raise Degenerate("fewer than 3 pairs")
    H = sab - np.outer(sa, sb) / n
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > LINE_RATIO * S[0]:
        raise Degenerate("pairs on a line")
    d = 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (sb / n + np.asarray(origin_y, F64)) - R @ (sa / n + np.asarray(origin_x, F64))
    return T


def box_of(xyz):
    p = np.asarray(xyz, F32)[:, :3].astype(F64)
    return p.min(0), p.max(0)


def box_corners(lo, hi):
    return np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], F64)


def corner_shift(corners, T0, T1):
    """the largest distance between a corner moved by T0 and by T1"""
    T0, T1 = as_T(T0), as_T(T1)
    p0, p1 = corners @ T0[:3, :3].T + T0[:3, 3], corners @ T1[:3, :3].T + T1[:3, 3]
    return float(np.sqrt(((p1 - p0) ** 2).sum(1)).max())


def search(p, fixed):
    """the exact nearest point (the best pair score, the lowest index among equals) and its fp32 squared distance"""
    idx = NG.brute(p, fixed)
    return idx, NG.d2_of(p, fixed, idx)


def icp(moving, fixed, max_dist, init=None, max_iter=50, min_delta=None):
    """seggroup_amd.align.icp's loop -> dict(T, iterations, converged, inliers, rms_before, rms_after, idx, d2, inlier)"""
    moving, fixed = np.asarray(moving, F32)[:, :3], np.asarray(fixed, F32)[:, :3]
    T = np.eye(4) if init is None else as_T(init)
    (mlo, mhi), (flo, fhi) = box_of(moving), box_of(fixed)
    om, of = 0.5 * (mlo + mhi), 0.5 * (flo + fhi)
    corners = box_corners(mlo, mhi)
    if min_delta is None:
        min_delta = 2.0 ** -23 * max(np.abs(v).max() for v in (mlo, mhi, flo, fhi))
    prev, converged, rms_before, it = None, False, None, 0
    for _ in range(max_iter):
        p = apply(moving, T)
        idx, d2 = search(p, fixed)
        inlier = d2 <= max_d2_of(max_dist)
        it += 1
        m, _ = moments(moving, fixed, idx, d2, max_dist, om, of)
        if m[0] == 0:
            raise ValueError("no inliers within max_dist")
        rms = math.sqrt(m[16] / m[0])
        rms_before = rms if rms_before is None else rms_before
        same = prev is not None and np.array_equal(idx, prev[0]) and np.array_equal(inlier, prev[1])
        prev = (idx, inlier)
        if same:
            converged = "fixed point"
            break
        T_new = solve(m, om, of)
        shift = corner_shift(corners, T, T_new)
        T = T_new
        if shift <= min_delta:
            converged = "min_delta"
            break
    return dict(T=T, iterations=it, converged=converged, inliers=int(m[0]), rms_before=rms_before, rms_after=rms, idx=idx, d2=d2, inlier=inlier)


# ---- the synthetic scene ----------------------------------------------------------------------------------------------------------------
# faces as (origin, edge u, edge v): a floor, two walls, and the top and two sides of a box standing on the floor; the room is centred
# on the origin so that a rotation about it moves no point farther than a rotation about the room's middle would
_FACES = (((-1.6, -1.2, -1.0), (3.2, 0, 0), (0, 2.4, 0)),            # floor
          ((-1.6, -1.2, -1.0), (0, 2.4, 0), (0, 0, 2.0)),            # wall x = -1.6
          ((-1.6, -1.2, -1.0), (3.2, 0, 0), (0, 0, 2.0)),            # wall y = -1.2
          ((0.1, -0.2, -0.3), (0.9, 0, 0), (0, 0.7, 0)),             # box top
          ((1.0, -0.2, -1.0), (0, 0.7, 0), (0, 0, 0.7)),             # box side x = 1.0
          ((0.1, 0.5, -1.0), (0.9, 0, 0), (0, 0, 0.7)))              # box side y = 0.5
_rooms = {}


def room(seed, n):
    """n points, uniform on the faces in proportion to their areas -> float32 [n,3]; the same array for the same (seed, n)"""
    if (seed, n) not in _rooms:
        rng = np.random.RandomState(seed)
        area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in _FACES])
        face = rng.choice(len(_FACES), size=n, p=area / area.sum())
        s, t = rng.rand(n), rng.rand(n)
        o, u, v = (np.array([f[i] for f in _FACES], F64)[face] for i in range(3))
        pts = (o + s[:, None] * u + t[:, None] * v).astype(F32)
        pts.setflags(write=False)
        _rooms[(seed, n)] = pts
    return _rooms[(seed, n)]
