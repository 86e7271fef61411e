"""Point-to-plane ICP (seggroup_amd/align.py metric="plane") restated in NumPy on top of tests/align_ref.py, which is
imported and not edited: the element-wise terms of the 31 moments in exactly the operation order of include/seggroup_hip.h, the moments
with np.sum together with the sums of the terms' absolute values, the Gauss-Newton solve on np.linalg.eigh, and the loop with
align_ref.search.  `knn_normals` is the plain kNN-covariance normal.  Nothing here calls the library.
"""
import math

import numpy as np

import align_ref as A

F32, F64 = np.float32, np.float64
PLANE_RATIO = 2.0 ** -40
SERIES_BELOW = 1e-8
NMOM = 31
TRI = [(r, c) for r in range(6) for c in range(r, 6)]                 # the upper triangle, row-major: moments 2..22


def knn_normals(xyz, k=10):
    """per point the eigenvector of the smallest eigenvalue of the covariance of its k + 1 nearest points (itself included) -> float64
    [N,3], unit length; the sign is whatever eigh returns, and the point-to-plane fit does not depend on it"""
    p = np.asarray(xyz, F32)[:, :3].astype(F64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    nb = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
    q = p[nb]
    q = q - q.mean(1, keepdims=True)
    _, v = np.linalg.eigh(np.einsum("nki,nkj->nij", q, q))
    return np.ascontiguousarray(v[:, :, 0])


def room_normals(points):
    """the analytic face normal of every point of align_ref.room: the unit normal of the first face whose plane holds the point and whose
    rectangle contains it -> float32 [n,3]"""
    p = np.asarray(points, F64)
    out = np.zeros((p.shape[0], 3))
    done = np.zeros(p.shape[0], bool)
    for o, u, v in A._FACES:
        o, u, v = (np.asarray(t, F64) for t in (o, u, v))
        n = np.cross(u, v)
        n /= np.linalg.norm(n)
        rel = p - o
        s, t = rel @ u / (u @ u), rel @ v / (v @ v)
        on = (np.abs(rel @ n) < 1e-5) & (s > -1e-5) & (s < 1 + 1e-5) & (t > -1e-5) & (t < 1 + 1e-5) & ~done
        out[on] = n
        done |= on
    assert done.all()
    return out.astype(F32)


def usable_normal(n):
    """n float64 [m,3] -> bool [m]: finite and 0.25 <= (n0*n0 + n1*n1) + n2*n2 <= 4"""
    with np.errstate(invalid="ignore", over="ignore"):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        return np.isfinite(n).all(1) & (nn >= 0.25) & (nn <= 4.0)


def moment_terms(x, T, y, normals, idx, d2, max_dist, origin=(0, 0, 0)):
    """-> (terms float64 [usable candidates, 31] with column 1 all zero, the number of skipped candidates).  Every operation is written
    once, in the order of the header, on float64 arrays: NumPy rounds each of them once, as the kernel does."""
    d2 = np.asarray(d2, F32)
    with np.errstate(invalid="ignore"):
        cand = d2 <= A.max_d2_of(max_dist)
    idx = np.asarray(idx)[cand]
    n = np.asarray(normals, F32)[:, :3].astype(F64)[idx]
    ok = usable_normal(n)
    skipped = int((~ok).sum())
    n, idx = n[ok], idx[ok]
    q = np.asarray(x, F32)[:, :3].astype(F64)[cand][ok]
    T = A.as_T(T)
    o = np.asarray(origin, F64)
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    p = [((T[r, 0] * qx + T[r, 1] * qy) + T[r, 2] * qz) + T[r, 3] for r in range(3)]
    a = [p[r] - o[r] for r in range(3)]
    yy = np.asarray(y, F32)[:, :3].astype(F64)[idx]
    b = [yy[:, r] - o[r] for r in range(3)]
    n0, n1, n2 = n[:, 0], n[:, 1], n[:, 2]
    e = [a[r] - b[r] for r in range(3)]
    res = (e[0] * n0 + e[1] * n1) + e[2] * n2
    J = [a[1] * n2 - a[2] * n1, a[2] * n0 - a[0] * n2, a[0] * n1 - a[1] * n0, n0, n1, n2]
    cols = [np.ones(res.shape[0]), np.zeros(res.shape[0])] + [J[r] * J[c] for r, c in TRI] + [J[r] * res for r in range(6)]
    cols += [res * res, d2[cand][ok].astype(F64)]
    return np.stack(cols, 1).reshape(-1, NMOM), skipped


def moments(x, T, y, normals, idx, d2, max_dist, origin=(0, 0, 0)):
    """-> (the 31 sums float64 [31], the sums of the terms' absolute values float64 [31])"""
    t, skipped = moment_terms(x, T, y, normals, idx, d2, max_dist, origin)
    m, mag = t.sum(0), np.abs(t).sum(0)
    m[1] = mag[1] = skipped
    return m, mag


def rodrigues(w):
    w = np.asarray(w, F64)
    th2 = float(w @ w)
    th = math.sqrt(th2)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], F64)
    sa = 1.0 - th2 / 6.0 if th < SERIES_BELOW else math.sin(th) / th
    sb = 0.5 - th2 / 24.0 if th < SERIES_BELOW else (1.0 - math.cos(th)) / th2
    return np.eye(3) + sa * K + sb * (K @ K)


def spectrum(m, length):
    """the eigenvalues of D M D, ascending, and its eigenvectors"""
    m = np.asarray(m, F64)
    M = np.zeros((6, 6))
    for k, (r, c) in enumerate(TRI):
        M[r, c] = M[c, r] = m[2 + k]
    D = np.array([1.0 / length] * 3 + [1.0] * 3)
    lam, V = np.linalg.eigh(D[:, None] * M * D[None, :])
    return lam, V, D


def solve(m, T, origin, length):
    """one Gauss-Newton step with LAPACK's eigh -> (T_new float64 [4,4], the step (w, v)); Degenerate as the library defines it.  The
    rotation is re-orthonormalised with an SVD (the nearest rotation), not with the library's Gram-Schmidt."""
    m = np.asarray(m, F64)
    if m[0] < 6:
        raise A.Degenerate("fewer than 6 usable pairs")
    lam, V, D = spectrum(m, length)
    if not lam[-1] > 0 or not lam[0] > PLANE_RATIO * lam[-1]:
        raise A.Degenerate("a motion is free")
    s = -D * (V @ ((V.T @ (D * m[23:29])) / lam))
    Rw = rodrigues(s[:3])
    T, o = A.as_T(T), np.asarray(origin, F64)
    U, _, Vt = np.linalg.svd(Rw @ T[:3, :3])
    out = np.eye(4)
    out[:3, :3] = U @ Vt
    out[:3, 3] = Rw @ (T[:3, 3] - o) + o + s[3:]
    return out, s


def icp(moving, fixed, normals, max_dist, init=None, max_iter=50, min_delta=None):
    """seggroup_amd.align.icp's metric="plane" loop -> dict(T, iterations, converged, inliers, skipped, rms_*, plane_rms_*, idx, d2, m)"""
    moving, fixed = np.asarray(moving, F32)[:, :3], np.asarray(fixed, F32)[:, :3]
    T = np.eye(4) if init is None else A.as_T(init)
    (mlo, mhi), (flo, fhi) = A.box_of(moving), A.box_of(fixed)
    c, length = 0.5 * (flo + fhi), 0.5 * float(np.sqrt(((fhi - flo) ** 2).sum()))
    corners = A.box_corners(mlo, mhi)
    if min_delta is None:
        min_delta = 2.0 ** -23 * max(np.abs(v).max() for v in (mlo, mhi, flo, fhi))
    converged, first, it = False, None, 0
    for _ in range(max_iter):
        idx, d2 = A.search(A.apply(moving, T), fixed)
        it += 1
        m, _ = moments(moving, T, fixed, normals, idx, d2, max_dist, c)
        if m[0] == 0:
            raise ValueError("no usable pair within max_dist")
        last = (math.sqrt(m[30] / m[0]), math.sqrt(m[29] / m[0]))
        first = last if first is None else first
        T_new, _ = solve(m, T, c, length)
        shift = A.corner_shift(corners, T, T_new)
        T = T_new
        if shift <= min_delta:
            converged = "min_delta"
            break
    return dict(T=T, iterations=it, converged=converged, inliers=int(m[0]), skipped=int(m[1]), rms_before=first[0], rms_after=last[0],
                plane_rms_before=first[1], plane_rms_after=last[1], idx=idx, d2=d2, m=m)
