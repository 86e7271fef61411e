"""The point-cloud over-segmenter over the RADIUS graph: the statement of DESIGN.md 8l in NumPy float32 -- the reference that
sg_radius_neighbours_grid, sg_pointcloud_normals_csr and sg_pcseg_edges_radius are held to bit for bit (tests/test_pcseg_radius_ref.py,
tests/test_gpu_pcseg_radius.py, tools/capture_pcseg_radius.py).

The pairs are radius_ref's (8k's predicate, unchanged); the lists are their CSR form with every row in ascending index; the neighbourhood
of a point is the point itself, then its row; mean, covariance, Jacobi, orientation, weights, order and the merge chain are pcseg_ref's
(8f), one NumPy call per float32 operation.  Nothing here calls the library.
"""
import numpy as np

import pcseg_ref as P
import radius_ref as RR

F32 = P.F32


# ---- 1-2. pairs and lists -----------------------------------------------------------------------------------------------------------
def lists(xyz, radius):
    """-> (off int64 [N+1], idx int32 [T]): off = the exclusive sum of radius_ref.count, the row of i = its neighbours in ascending index"""
    n = np.asarray(xyz).shape[0]
    cnt = np.zeros(n, np.int64)
    cols = []
    for i0, ok in RR.blocks(xyz, radius):
        cnt[i0:i0 + ok.shape[0]] = ok.sum(1)
        cols.append(np.nonzero(ok)[1])                          # row-major: ascending column within a row
    off = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    idx = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    assert idx.shape[0] == off[n]
    return off, idx


# ---- 3. neighbourhoods of variable length ---------------------------------------------------------------------------------------------
def _walk(off, idx):
    """yields (rows, j): step t = 0 is every point with itself, step t >= 1 the rows longer than t - 1 with their (t - 1)-th entry"""
    n = off.shape[0] - 1
    length = np.diff(off)
    yield np.arange(n), np.arange(n)
    for t in range(int(length.max()) if n else 0):
        rows = np.nonzero(length > t)[0]
        yield rows, idx[off[rows] + t].astype(np.int64)


def covariance(xyz, off, idx):
    """-> mean [N,3] and the six sums over the neighbourhood (i, then its row in stored order) from +0, not normalised"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    n = x.shape[0]
    s = np.zeros((n, 3), F32)
    for rows, j in _walk(off, idx):
        s[rows] = s[rows] + x[j]
    m = (np.diff(off) + 1).astype(F32)
    mean = (s / m[:, None]).astype(F32)
    a = [np.zeros(n, F32) for _ in range(6)]
    for rows, j in _walk(off, idx):
        q = x[j] - mean[rows]
        for c, (u, v) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            a[c][rows] = a[c][rows] + q[:, u] * q[:, v]
    return mean, a


def normals(xyz, off, idx, viewpoint=None, sweeps=P.SWEEPS, want_offdiag=False):
    """8f steps 4-5 over 8l's neighbourhoods -> [N,3] f32 (and the three off-diagonals after the last sweep)"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    _, a = covariance(x, off, idx)
    d, offd, V = P.jacobi(a, sweeps)
    b1 = d[1] < d[0]
    dm = np.where(b1, d[1], d[0])
    b2 = d[2] < dm
    n = np.stack([np.where(b2, V[r][2], np.where(b1, V[r][1], V[r][0])) for r in range(3)], 1).astype(F32)
    c = P.default_viewpoint(x) if viewpoint is None else np.asarray(viewpoint, F32).reshape(3)
    dd = c[None, :] - x
    with np.errstate(all="ignore"):
        s = (n[:, 0] * dd[:, 0] + n[:, 1] * dd[:, 1]) + n[:, 2] * dd[:, 2]
    out = np.where((s < 0)[:, None], -n, n).astype(F32)
    return (out, offd) if want_offdiag else out


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------
def edges_of(off, idx):
    """the pairs a < b in lexicographic order: the upper halves of the rows -> [E,2] int32"""
    n = off.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    up = idx > rows
    return np.stack([rows[up], idx[up].astype(np.int64)], 1).astype(np.int32)


def sorted_edges(xyz, radius, viewpoint=None):
    """-> dict(off, idx, normals, lex_edges, lex_w, edges, w): every stage of the statement"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    off, idx = lists(x, radius)
    nrm = normals(x, off, idx, viewpoint)
    edges = edges_of(off, idx)
    w = P.edge_weights(x, nrm, edges)
    order = np.argsort(w, kind="stable")                        # the list is lexicographic: a stable sort by w gives (w, a, b)
    return dict(off=off, idx=idx, normals=nrm, lex_edges=edges, lex_w=w, edges=np.ascontiguousarray(edges[order]),
                w=np.ascontiguousarray(w[order]))


def segment_pointcloud(xyz, radius, k_thresh=0.01, seg_min_verts=20, viewpoint=None):
    r = sorted_edges(xyz, radius, viewpoint)
    return P.merge(r["edges"], r["w"], np.asarray(xyz).shape[0], k_thresh, seg_min_verts)


def stage_digests(r, seg):
    """what tests/golden/pcseg_radius_expected.json holds of one case"""
    d = P.array_digest
    return {"T": int(r["off"][-1]), "off": d(r["off"], "<i8"), "idx": d(r["idx"], "<i4"), "normals": d(r["normals"], "<f4"),
            "lex_edges": d(r["lex_edges"], "<i4"), "lex_w": d(r["lex_w"], "<f4"), "edges_sorted": d(r["edges"], "<i4"),
            "w_sorted": d(r["w"], "<f4"), "ids": d(seg, "<i4")}


def eigh_check(xyz, off, idx, nrm):
    """pcseg_ref.eigh_check over 8l's neighbourhoods: float64 eigh of every point's covariance -> (largest angle in rad over the points
    whose relative gap (l1 - l0) / l2 is at least 0.05, share of the points with that gap)"""
    x = np.asarray(xyz, np.float64)[:, :3]
    n = x.shape[0]
    m = (np.diff(off) + 1).astype(np.float64)
    s = np.zeros((n, 3))
    for rows, j in _walk(off, idx):
        np.add.at(s, rows, x[j])
    mean = s / m[:, None]
    cov = np.zeros((n, 3, 3))
    for rows, j in _walk(off, idx):
        q = x[j] - mean[rows]
        np.add.at(cov, rows, q[:, :, None] * q[:, None, :])
    lam, vec = np.linalg.eigh(cov)
    with np.errstate(all="ignore"):
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    ok = gap >= 0.05
    nn = np.asarray(nrm, np.float64)
    cosang = np.abs((nn * vec[:, :, 0]).sum(1)) / np.linalg.norm(nn, axis=1)
    ang = np.arccos(np.clip(cosang, -1.0, 1.0))
    return (float(ang[ok].max()) if ok.any() else 0.0), float(ok.mean())


# ---- the generated cases the two test files and the capture share -------------------------------------------------------------------------
ROOM_RADIUS = 0.08
CLUMPED_RADIUS = 0.06
BALL_RADIUS = 0.01


def clumped_room(copies=12, jitter=1e-4, seed=17):
    """pcseg_ref.make_room_cloud(20, 0.05, 0.0, seed=3) with every point `copies` times, jittered by at most `jitter` per axis and
    shuffled -> (xyz f32 [15792,3], plane ids): where the kNN graph at k = 10 has no edge out of a clump"""
    xyz, plane = P.make_room_cloud(20, 0.05, 0.0, seed=3)
    rng = np.random.RandomState(seed)
    big = np.repeat(xyz.astype(np.float64), copies, axis=0) + rng.uniform(-jitter, jitter, (xyz.shape[0] * copies, 3))
    lab = np.repeat(plane, copies)
    perm = rng.permutation(big.shape[0])
    return np.ascontiguousarray(big[perm], dtype=F32), np.ascontiguousarray(lab[perm])


def ball(n=300, seed=29):
    """n points within 1e-3 of one centre: at radius 0.01 every row is n - 1 long, longer than a tile of 256 candidates"""
    rng = np.random.RandomState(seed)
    v = rng.standard_normal((n, 3))
    v *= (rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) * 0.9e-3 / np.linalg.norm(v, axis=1))[:, None]
    return np.ascontiguousarray(v + np.array([0.4, -1.2, 0.9]), dtype=F32)


def fixture_cases():
    """name -> (xyz, radius): every case of tests/golden/pcseg_radius_expected.json"""
    out = {}
    for n in RR.SIZES:
        for tag, r in RR.LINE_RADII.items():
            out["line_%d_%s" % (n, tag)] = (RR.jittered_line(n), r)
    out["two_clumps"] = (RR.two_clumps(), RR.CLUMP_RADIUS)
    clouds = P.case_clouds(include_large=True)
    for name, _ in P.ROOMS:
        out[name] = (clouds[name][0], ROOM_RADIUS)
    out["room_dup"] = (clouds["room_dup"][0], ROOM_RADIUS)
    out["all_equal"] = (clouds["all_equal"][0], 0.01)
    out["ball_300"] = (ball(), BALL_RADIUS)
    out["room_20k"] = (clouds["room_20k"][0], 0.04)
    out["clumped_room"] = (clumped_room()[0], CLUMPED_RADIUS)
    return out


_cases = {}


def case(name):
    """(xyz, radius, stages, ids) of one fixture case at the default parameters, computed once per process"""
    if "clouds" not in _cases:
        _cases["clouds"] = fixture_cases()
    if name not in _cases:
        xyz, radius = _cases["clouds"][name]
        r = sorted_edges(xyz, radius)
        _cases[name] = (xyz, radius, r, P.merge(r["edges"], r["w"], xyz.shape[0], 0.01, 20))
    return _cases[name]
