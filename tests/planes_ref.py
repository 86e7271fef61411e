"""Plane extraction (seggroup_amd/planes.py) restated in NumPy: the list of free points, splitmix64 triples over it, the
rejection rules, the unit normals and the counts of sg_plane_ransac in float64 with one NumPy call per operation, the 11 sums with np.sum,
the fit with numpy.linalg.eigh, the labelling, the loop of detect_planes and level_transform.  Nothing here calls the library.

What cannot be compared exactly is fenced off here, not in the tests: `Ransac.undecided` for a rejection compare within a relative 1e-9
of its threshold, `count_lo` / `count_hi` for a point on the distance (or on the normal cone), and `Detected.fenced` for a round of the
loop whose outcome one of those could change.
"""
import math

import numpy as np

import align_ref as A
import register_ref as G

F32, F64 = np.float32, np.float64
MARGIN = 1e-9
LINE_RATIO = 2.0 ** -40
dot, cross = G.dot, G.cross


def free_of(n, labels):
    """-> int64 [M]: the free points in ascending index"""
    return np.arange(n, dtype=np.int64) if labels is None else np.nonzero(np.asarray(labels) < 0)[0]


def inliers(p, plane, dist, normals=None, min_cos=0.0):
    """p float64 [M,3], plane [..,4] -> bool [..,M]: |n.p + d| <= dist, and with normals also min_cos <= |n.nrm| < inf"""
    pl = np.asarray(plane, F64)[..., None, :]
    with np.errstate(all="ignore"):
        r = ((pl[..., 0] * p[:, 0] + pl[..., 1] * p[:, 1]) + pl[..., 2] * p[:, 2]) + pl[..., 3]
        ok = np.abs(r) <= dist
        if normals is not None:
            a = np.abs((pl[..., 0] * normals[:, 0] + pl[..., 1] * normals[:, 1]) + pl[..., 2] * normals[:, 2])
            ok &= (a >= min_cos) & (a < np.inf)
    return ok


def _near(x, thr, rel=MARGIN):
    with np.errstate(invalid="ignore"):
        return (thr > 0) & (np.abs(x - thr) <= rel * thr)


def hypotheses_of(p, tri, min_edge, min_sine):
    """free points p float64 [M,3], triples [H,3] of positions in it -> (keep bool [H], undecided bool [H], plane float64 [H,4]: zeros
    where rejected)"""
    tri = np.asarray(tri, np.int64)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    p0, p1, p2 = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    with np.errstate(all="ignore"):
        u, v, w = p1 - p0, p2 - p0, p2 - p1
        c = cross(u, v)
        lu, lv, lw, lc = (np.sqrt(dot(x, x)) for x in (u, v, w, c))
        thr = (min_sine * lu) * lv
        keep &= (lu >= min_edge) & (lv >= min_edge) & (lw >= min_edge) & (lc >= thr) & (lc > 0)
        und = _near(lu, min_edge) | _near(lv, min_edge) | _near(lw, min_edge) | _near(lc, thr)
        n = c / lc[:, None]
        d = -dot(n, p0)
    plane = np.where(keep[:, None], np.concatenate([n, d[:, None]], 1), 0.0)
    return keep, und, plane


def counts(p, plane, dist, normals=None, min_cos=0.0, chunk=256):
    out = np.zeros(plane.shape[0], np.int64)
    for h0 in range(0, plane.shape[0], chunk):
        out[h0:h0 + chunk] = inliers(p, plane[h0:h0 + chunk], dist, normals, min_cos).sum(-1)
    return out


class Ransac:
    """what sg_plane_ransac is held to: `free` (indices), `triples`, `keep` / `undecided` [H], `plane` [H,4], `count` (-1 where rejected),
    `count_lo` / `count_hi` (at dist (1 -/+ 1e-9) and min_cos (1 +/- 1e-9)) and `best`"""


def ransac(xyz, dist, hypotheses, seed=0, labels=None, min_edge=None, min_sine=0.1, triples=None, normals=None, min_cos=0.0):
    x = np.asarray(xyz, F32)[:, :3].astype(F64)
    r = Ransac()
    r.free = free_of(x.shape[0], labels)
    p = x[r.free]
    nrm = None if normals is None else np.asarray(normals, F32)[:, :3].astype(F64)[r.free]
    m = p.shape[0]
    min_edge = 10.0 * float(dist) if min_edge is None else float(min_edge)
    h = int(hypotheses)
    if m < 3:
        r.triples = np.zeros((h, 3), np.int32)
        r.keep, r.undecided, r.plane = np.zeros(h, bool), np.zeros(h, bool), np.zeros((h, 4))
    else:
        r.triples = G.triples_of(seed, h, m) if triples is None else np.asarray(triples, np.int32).reshape(-1, 3)
        r.keep, r.undecided, r.plane = hypotheses_of(p, r.triples, min_edge, float(min_sine))
    k = r.keep
    r.count, r.count_lo, r.count_hi = (np.full(h, -1, np.int64) for _ in range(3))
    if k.any():
        r.count[k] = counts(p, r.plane[k], dist, nrm, min_cos)
        r.count_lo[k] = counts(p, r.plane[k], dist * (1.0 - MARGIN), nrm, min_cos * (1.0 + MARGIN))
        r.count_hi[k] = counts(p, r.plane[k], dist * (1.0 + MARGIN), nrm, min_cos * (1.0 - MARGIN))
    r.best = int(np.argmax(r.count)) if k.any() else -1                  # the highest count, the lowest h among equals
    return r


def moment_terms(xyz, plane, dist, origin, labels=None, normals=None, min_cos=0.0):
    """the terms of the 11 sums over the free inliers -> float64 [n, 11] (column 0 is all ones)"""
    x = np.asarray(xyz, F32)[:, :3].astype(F64)
    free = free_of(x.shape[0], labels)
    p = x[free]
    nrm = None if normals is None else np.asarray(normals, F32)[:, :3].astype(F64)[free]
    sel = inliers(p, np.asarray(plane, F64), dist, nrm, min_cos)
    p = p[sel]
    pl = np.asarray(plane, F64)
    res = ((pl[0] * p[:, 0] + pl[1] * p[:, 1]) + pl[2] * p[:, 2]) + pl[3]
    q = p - np.asarray(origin, F64)
    qq = np.stack([q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]], 1)
    return np.concatenate([np.ones((p.shape[0], 1)), q, qq, (res * res)[:, None]], 1)


def moments(xyz, plane, dist, origin, labels=None, normals=None, min_cos=0.0):
    """-> (the 11 sums, the sums of the terms' absolute values: what bounds the distance between two summation orders)"""
    t = moment_terms(xyz, plane, dist, origin, labels, normals, min_cos)
    return t.sum(0), np.abs(t).sum(0)


class Degenerate(ValueError):
    pass


def fit(m, origin=(0, 0, 0)):
    """the 11 moments -> (plane [4], centroid [3], rms) with LAPACK's eigh; fewer than 3 points or points on a line raise Degenerate"""
    m = np.asarray(m, F64)
    n, sq = m[0], m[1:4]
    if n < 3:
        raise Degenerate("fewer than 3 points")
    S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    w, V = np.linalg.eigh(S - np.outer(sq, sq) / n)
    if not (w[2] > 0 and w[1] > LINE_RATIO * w[2]):
        raise Degenerate("points on a line")
    nrm = V[:, 0] / np.linalg.norm(V[:, 0])
    if nrm[int(np.argmax(np.abs(nrm)))] < 0:
        nrm = -nrm
    centroid = np.asarray(origin, F64) + sq / n
    return np.concatenate([nrm, [-float(nrm @ centroid)]]), centroid, math.sqrt(max(w[0], 0.0) / n)


class Detected:
    """detect_planes' result: labels, planes [P,4], points, ransac_count, h, rms, centroid, and `fenced`: a round whose outcome a fenced
    compare could change (the best count not alone at its value up to the fences, an undecided hypothesis that could win, a count or a
    labelled number within the fences of min_points, a point of the refit on the distance)"""


def detect(xyz, dist, max_planes=16, min_points=None, hypotheses=4096, seed=0, min_edge=None, min_sine=0.1, normals=None, min_cos=0.0):
    x32 = np.asarray(xyz, F32)[:, :3]
    x = x32.astype(F64)
    nrm = None if normals is None else np.asarray(normals, F32)[:, :3].astype(F64)
    lo, hi = A.box_of(x32)
    origin = 0.5 * (lo + hi)
    labels = np.full(x.shape[0], -1, np.int32)
    out = Detected()
    out.fenced = False
    rows = []
    for p in range(max_planes):
        r = ransac(x32, dist, hypotheses, seed + p, labels, min_edge, min_sine, None, normals, min_cos)
        if r.best < 0:
            break
        votes = int(r.count[r.best])
        # the winner must win whatever the points on the fences do: no other hypothesis may reach its lowest count with its own highest
        # (a lower h wins a tie), no rejection compare may sit on its threshold, and min_points must not fall between the two counts
        hs = np.arange(hypotheses)
        rival = (hs != r.best) & ((r.count_hi > r.count_lo[r.best]) | ((r.count_hi == r.count_lo[r.best]) & (hs < r.best)))
        out.fenced = out.fenced or bool(rival.any()) or bool(r.undecided.any())
        out.fenced = out.fenced or (r.count_lo[r.best] < min_points) != (r.count_hi[r.best] < min_points)
        if votes < min_points:
            break
        m, _ = moments(x32, r.plane[r.best], dist, origin, labels, normals, min_cos)
        try:
            pl, centroid, rms = fit(m, origin)
        except Degenerate:
            break
        free = free_of(x.shape[0], labels)
        sel = inliers(x[free], pl, dist, None if nrm is None else nrm[free], min_cos)
        for sign in (-1.0, 1.0):                                          # 1e-6: the refit comes from another eigen-solver, not from the same operations
            other = inliers(x[free], pl, dist * (1.0 + sign * 1e-6), None if nrm is None else nrm[free], min_cos * (1.0 - sign * 1e-6))
            out.fenced = out.fenced or not np.array_equal(other, sel)
        if int(sel.sum()) < min_points:
            break
        labels[free[sel]] = p
        rows.append((pl, int(sel.sum()), votes, r.best, rms, centroid))
    out.labels = labels
    out.planes = np.array([r[0] for r in rows], F64).reshape(-1, 4)
    out.points, out.ransac_count, out.h = (np.array([r[i] for r in rows], np.int64) for i in (1, 2, 3))
    out.rms = np.array([r[4] for r in rows], F64)
    out.centroid = np.array([r[5] for r in rows], F64).reshape(-1, 3)
    return out


def level_transform(planes, centroid, points, xyz, which="largest"):
    """-> T [4,4]: the chosen plane's normal, turned towards the cloud's mean, onto +z by the smallest rotation about the plane's centroid,
    which lands at z = 0"""
    i = int(np.argmax(points)) if which == "largest" else int(which)
    n = planes[i, :3] / np.linalg.norm(planes[i, :3])
    c = centroid[i]
    mean = np.asarray(xyz, F64)[:, :3].mean(0)
    if n @ (mean - c) < 0:
        n = -n
    z = np.array([0.0, 0.0, 1.0])
    axis = np.cross(n, z)
    s = np.linalg.norm(axis)
    if s < 1e-15:
        R = np.eye(3) if n[2] > 0 else np.diag([1.0, -1.0, -1.0])
    else:
        k = axis / s
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
        a = math.atan2(s, n[2])
        R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.array([c[0], c[1], 0.0]) - R @ c
    return T


# ---- the acceptance fixture -------------------------------------------------------------------------------------------------------------
PARAMS = dict(dist=0.005, min_points=40, hypotheses=1024, seed=0)
_cache = {}


def fixture():
    """register_ref.jittered_room(1, 3000, 1e-3) moved by align_ref.pose(37.0, 0.5) -> (float32 [3000,3], the pose)"""
    P = A.pose(37.0, 0.5)
    return A.apply(G.jittered_room(1, 3000, 1e-3), P), P


def fixture_reference():
    """detect() on the fixture, once per process"""
    if "d" not in _cache:
        _cache["d"] = detect(fixture()[0], **PARAMS)
    return _cache["d"]


def face_corners(P):
    """the four corners of each face of align_ref._FACES under the pose P -> float64 [6,4,3]"""
    out = []
    for o, u, v in A._FACES:
        o, u, v = (np.asarray(t, F64) for t in (o, u, v))
        c = np.array([o, o + u, o + v, o + u + v])
        out.append(c @ P[:3, :3].T + P[:3, 3])
    return np.array(out)
