"""NumPy restatement of the label index and the per-label reductions behind seggroup_amd/boxes.py, one statement per
operation.  It never calls the library.  Products and sums are written out so that NumPy rounds as the contract says: double arithmetic on
the widened fp32 inputs, dot(a, b) = (a0*b0 + a1*b1) + a2*b2, nothing contracted."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
CHUNK = 1024


def label_index(labels):
    """-> (order int32 [M], values int32 [L], start int32 [L+1], ignored): the labelled points (labels >= 0) by label, ascending index
    within a label"""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    raw = np.flatnonzero(labels >= 0)
    order = raw[np.argsort(labels[raw], kind="stable")]
    values, counts = np.unique(labels[raw], return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)])
    return order.astype(np.int32), values.astype(np.int32), start.astype(np.int32), int(labels.size - raw.size)


def _per_label(fn, terms, start):
    """fn.reduceat over the rows of each label; [L, ...]"""
    if start.size == 1:
        return np.zeros((0,) + terms.shape[1:], terms.dtype)
    return fn.reduceat(terms, start[:-1].astype(np.int64), axis=0)


def moment_terms(xyz, order, start):
    """float64 [M,10]: 1 | q | q q^T (xx xy xz yy yz zz) per labelled point in the index's order, q = p - the label's first point"""
    p = np.asarray(xyz)[:, :3].astype(F64)[order]
    counts = np.diff(start)
    first = np.repeat(p[start[:-1]], counts, axis=0) if counts.size else np.zeros((0, 3))
    q = p - first
    cols = [np.ones(q.shape[0]), q[:, 0], q[:, 1], q[:, 2]]
    for r in range(3):
        for c in range(r, 3):
            cols.append(q[:, r] * q[:, c])
    return np.stack(cols, 1) if q.shape[0] else np.zeros((0, 10))


def moments(xyz, order, start):
    """-> (m float64 [L,10] by np.add over each label's terms, mag [L,10] the sums of the terms' magnitudes, lo, hi float32 [L,3])"""
    t = moment_terms(xyz, order, start)
    p32 = np.asarray(xyz)[:, :3].astype(F32)[order]
    return _per_label(np.add, t, start), _per_label(np.add, np.abs(t), start), _per_label(np.minimum, p32, start), _per_label(np.maximum, p32, start)


def angle_table(angles):
    theta = np.arange(angles, dtype=F64) * ((math.pi / 2.0) / angles)
    return np.stack([np.cos(theta), np.sin(theta)], 1)


def yaw_boxes(xyz, order, start, cs):
    """-> (best int32 [L], ext float64 [L,4], every float64 [L,A,4]): umin umax vmin vmax of u = c*x + s*y, v = c*y - s*x per angle, the
    angle of least (umax - umin) * (vmax - vmin), the lowest among equals"""
    p = np.asarray(xyz)[:, :3].astype(F64)[order]
    x, y = p[:, 0:1], p[:, 1:2]
    c, s = cs[None, :, 0], cs[None, :, 1]
    cx, sy, cy, sx = c * x, s * y, c * y, s * x
    u = cx + sy
    v = cy - sx
    every = np.stack([_per_label(np.minimum, u, start), _per_label(np.maximum, u, start), _per_label(np.minimum, v, start),
                      _per_label(np.maximum, v, start)], 2)
    du = every[:, :, 1] - every[:, :, 0]
    dv = every[:, :, 3] - every[:, :, 2]
    area = du * dv
    best = np.argmin(area, axis=1).astype(np.int32) if area.shape[0] else np.zeros(0, np.int32)       # the first among equals
    ext = every[np.arange(best.size), best] if best.size else np.zeros((0, 4))
    return best, ext, every


def frame_extents(xyz, order, start, frames):
    """-> float64 [L,6]: min, max of dot(row_k, p), k = 0, 1, 2, in the label's own frame"""
    p = np.asarray(xyz)[:, :3].astype(F64)[order]
    counts = np.diff(start)
    f = np.repeat(np.asarray(frames, F64).reshape(-1, 3, 3), counts, axis=0)                          # [M,3,3]
    out = []
    for k in range(3):
        d = (f[:, k, 0] * p[:, 0] + f[:, k, 1] * p[:, 1]) + f[:, k, 2] * p[:, 2]
        out += [_per_label(np.minimum, d, start), _per_label(np.maximum, d, start)]
    return np.stack(out, 1) if counts.size else np.zeros((0, 6))


def covariance(m):
    """the 3 x 3 covariance of one row of ten sums"""
    n, s = m[0], m[1:4]
    at = ((4, 5, 6), (5, 7, 8), (6, 8, 9))
    return np.array([[(m[at[r][c]] - s[r] * s[c] / n) / n for c in range(3)] for r in range(3)])


def box_axes(m):
    """the contract's frame from numpy.linalg.eigh -> (R [3,3], eig [3] descending): rows 0 and 1 with their largest-magnitude component
    positive (the lowest axis among equals), row 2 their cross product; the identity when the largest eigenvalue is not positive"""
    w, v = np.linalg.eigh(covariance(np.asarray(m, F64)))
    w, v = w[::-1], v[:, ::-1]
    if not w[0] > 0.0:
        return np.eye(3), w
    rows = []
    for r in range(2):
        a = v[:, r].copy()
        if a[int(np.argmax(np.abs(a)))] < 0.0:
            a = -a
        rows.append(a)
    rows.append(np.cross(rows[0], rows[1]))
    return np.array(rows), w


def corners(center, size, R):
    """[L,8,3]: bit a of corner k set -> the positive side of axis a"""
    out = np.zeros((center.shape[0], 8, 3))
    for k in range(8):
        c = center.copy()
        for a in range(3):
            c = c + ((1.0 if k >> a & 1 else -1.0) * (0.5 * size[:, a]))[:, None] * R[:, a, :]
        out[:, k] = c
    return out


def label_boxes(xyz, labels, kind="yaw", angles=90, min_points=1, frames=None):
    """the module's label_boxes -> dict of its fields.  kind "pca" takes the frames [L,3,3] (the library's sg_box_axes is Jacobi, this
    file's box_axes is eigh: the two agree to rounding, so extents are compared in ONE frame)."""
    xyz = np.asarray(xyz)
    order, values, start, ignored = label_index(labels)
    m, _, lo, hi = moments(xyz, order, start)
    l = values.size
    first = order[start[:-1]]
    p_first = xyz[first, :3].astype(F64)
    count = m[:, 0].astype(np.int64)
    centroid = p_first + m[:, 1:4] / m[:, 0:1]
    cov = np.array([covariance(row)[np.triu_indices(3)] for row in m]).reshape(l, 6)
    lo64, hi64 = lo.astype(F64), hi.astype(F64)
    yaw = np.full(l, np.nan)
    if kind == "aabb":
        R = np.tile(np.eye(3), (l, 1, 1))
        mins, maxs = lo64, hi64
    elif kind == "yaw":
        best, ext, _ = yaw_boxes(xyz, order, start, angle_table(angles))
        theta = best.astype(F64) * ((math.pi / 2.0) / angles)
        c, s = np.cos(theta), np.sin(theta)
        R = np.zeros((l, 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, s, -s, c, 1.0
        mins = np.stack([ext[:, 0], ext[:, 2], lo64[:, 2]], 1)
        maxs = np.stack([ext[:, 1], ext[:, 3], hi64[:, 2]], 1)
        yaw = theta
    else:
        R = np.asarray(frames, F64).reshape(l, 3, 3)
        e = frame_extents(xyz, order, start, R)
        mins, maxs = e[:, 0::2], e[:, 1::2]
    mid = 0.5 * (mins + maxs)
    size = maxs - mins
    center = (mid[:, 0:1] * R[:, 0, :] + mid[:, 1:2] * R[:, 1, :]) + mid[:, 2:3] * R[:, 2, :]
    keep = count >= min_points
    return dict(values=values[keep], count=count[keep], first=first[keep].astype(np.int32), lo=lo[keep], hi=hi[keep], centroid=centroid[keep],
                cov=cov[keep], R=R[keep], center=center[keep], size=size[keep], yaw=yaw[keep], ignored=ignored)


def detector_rows(lo, hi, sem):
    lo, hi = lo.astype(F64), hi.astype(F64)
    return np.concatenate([0.5 * (lo + hi), hi - lo, np.asarray(sem, F64).reshape(-1, 1)], 1)


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
def lattice_cuboid(w=3.0, h=2.0, d=1.0, step=0.25, angle=0.0, origin=(0.0, 0.0, 0.0), noise=0.0, seed=0):
    """the points of a `step` lattice filling [0,w] x [0,h] x [0,d], turned by `angle` radians about z and moved to `origin` ->
    float32 [n,3] (the float32 rounding of the turned coordinates is part of the cloud)"""
    gx, gy, gz = (np.arange(0.0, e + step / 2, step) for e in (w, h, d))
    p = np.stack(np.meshgrid(gx, gy, gz, indexing="ij"), -1).reshape(-1, 3)
    if noise:
        p = p + np.random.RandomState(seed).normal(0.0, noise, p.shape)
    c, s = math.cos(angle), math.sin(angle)
    q = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2]], 1)
    return (q + np.asarray(origin, F64)).astype(F32)
