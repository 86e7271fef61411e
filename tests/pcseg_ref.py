"""The point-cloud over-segmenter's specification restated in NumPy float32 -- the reference that the library's device
stages are held to bit for bit (tests/test_pcseg_ref.py, tests/test_gpu_pcseg.py, tools/capture_pcseg.py).

Every array is float32 and every operation is one NumPy call on float32 operands, so each is rounded once, in the order the
specification writes it; NumPy's float32 sqrt and division are correctly rounded.  The one exception is the pair score's K = 3 dot
product, whose two fused multiply-adds are formed exactly (see _fma).  The merge chain is tests/overseg_ref.py's: steps 5-8 of 8d are
unchanged.  Nothing here calls the library.
"""
import concurrent.futures
import hashlib

import numpy as np

import overseg_ref

F32 = np.float32
SWEEPS = 5
merge = overseg_ref.merge
digest = overseg_ref.digest
PARAM_SWEEP = overseg_ref.PARAM_SWEEP


# ---- 1. the lists ----------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c of float32 arrays, rounded ONCE to float32.  The product of two float32 is exact in float64; the float64 sum is rounded to
    53 bits, and rounding that again to 24 bits differs from the single rounding only where the float64 sum sits exactly half way between
    two float32 neighbours although the exact sum does not.  Those entries are decided by the sum's exact rounding error (TwoSum)."""
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    r = s.astype(F32)
    tie = (np.ascontiguousarray(s).view(np.int64) & 0x1fffffff) == 0x10000000
    if tie.any():
        aa, bb, cc = (np.broadcast_to(x, s.shape)[tie].astype(np.float64) for x in (a, b, c))
        p = aa * bb
        st = p + cc
        v = st - p
        err = (p - (st - v)) + (cc - v)                         # TwoSum: the exact sum is st + err
        rt = r[tie]
        lo = np.where(rt.astype(np.float64) <= st, rt, np.nextafter(rt, F32(-np.inf)))
        hi = np.nextafter(lo, F32(np.inf))
        r[tie] = np.where(err > 0, hi, np.where(err < 0, lo, rt))
    return r


def _sq(p):
    return (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]


def pair_scores(q, c):
    """s[i, j] = ((-qq_i) - (-2 * t_ij)) - cc_j with t = fma(qz, cz, fma(qy, cy, qx * cx)): the library's pair_score"""
    t = q[:, 0:1] * c[None, :, 0]
    t = _fma(q[:, 1:2], c[None, :, 1], t)
    t = _fma(q[:, 2:3], c[None, :, 2], t)
    inner = F32(-2.0) * t
    return ((-_sq(q))[:, None] - inner) - _sq(c)[None, :]


def _top(s, kk):
    """per row the kk best columns: descending score, the lower index first among equal scores"""
    m, n = s.shape
    kth = np.partition(s, n - kk, axis=1)[:, n - kk]
    rows, cols = np.nonzero(s >= kth[:, None])
    order = np.lexsort((cols, -s[rows, cols], rows))
    rows, cols = rows[order], cols[order]
    start = np.searchsorted(rows, np.arange(m))
    return cols[start[:, None] + np.arange(kk)[None, :]]


def knn_table(xyz, k=10, chunk=512, threads=4):
    """-> int32 [N, k+1]: the complete top-(k+1) list of every point against the whole cloud; entry 0 is kept"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    n = x.shape[0]
    if n <= k:
        raise ValueError("%d points for k = %d" % (n, k))
    out = np.empty((n, k + 1), np.int32)

    def one(i):
        out[i:i + chunk] = _top(pair_scores(x[i:i + chunk], x), k + 1)
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(0, n, chunk)))
    return out


# ---- 2-5. normals ------------------------------------------------------------------------------------------------------------------
def default_viewpoint(xyz):
    x = np.asarray(xyz, F32)
    return ((x.min(0) + x.max(0)) * F32(0.5)).astype(F32)


def covariance(xyz, table):
    """-> mean [N,3] and the six sums a00, a01, a02, a11, a12, a22 over the list points in list order from +0, not normalised"""
    x = np.asarray(xyz, F32)
    kk = table.shape[1]
    s = np.zeros((x.shape[0], 3), F32)
    for t in range(kk):
        s = s + x[table[:, t]]
    mean = s / F32(kk)
    a = [np.zeros(x.shape[0], F32) for _ in range(6)]
    for t in range(kk):
        q = x[table[:, t]] - mean
        for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            a[n] = a[n] + q[:, i] * q[:, j]
    return mean, a


def jacobi(a, sweeps=SWEEPS):
    """cyclic Jacobi on the symmetric 3 x 3 matrices a = [a00, a01, a02, a11, a12, a22] (arrays over the points) -> diagonal [3][N],
    off-diagonals [3][N] after the last sweep, accumulated rotation v[r][c]"""
    n = a[0].shape[0]
    A = {(0, 0): a[0].copy(), (0, 1): a[1].copy(), (0, 2): a[2].copy(), (1, 1): a[3].copy(), (1, 2): a[4].copy(), (2, 2): a[5].copy()}
    V = [[np.full(n, F32(1.0 if r == c else 0.0)) for c in range(3)] for r in range(3)]
    one = F32(1.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
                apq = A[(p, q)]
                on = apq != 0
                theta = (A[(q, q)] - A[(p, p)]) / (F32(2.0) * apq)
                sgn = np.where(theta >= 0, one, -one).astype(F32)
                t = sgn / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                h = t * apq
                new = {(p, p): A[(p, p)] - h, (q, q): A[(q, q)] + h, (p, q): np.zeros(n, F32),
                       rp: c * A[rp] - s * A[rq], rq: s * A[rp] + c * A[rq]}
                for key, val in new.items():
                    A[key] = np.where(on, val, A[key]).astype(F32)
                for row in range(3):
                    x, y = V[row][p], V[row][q]
                    V[row][p] = np.where(on, c * x - s * y, x).astype(F32)
                    V[row][q] = np.where(on, s * x + c * y, y).astype(F32)
    return [A[(0, 0)], A[(1, 1)], A[(2, 2)]], [A[(0, 1)], A[(0, 2)], A[(1, 2)]], V


def normals(xyz, table, viewpoint=None, sweeps=SWEEPS):
    """-> [N,3] f32: the column of the accumulated rotation whose diagonal entry is smallest (the lowest index among equal entries), not
    re-normalised, turned towards the viewpoint (default: the centre of the bounding box)"""
    x = np.asarray(xyz, F32)
    _, a = covariance(x, table)
    d, _, V = jacobi(a, sweeps)
    b1 = d[1] < d[0]
    dm = np.where(b1, d[1], d[0])
    b2 = d[2] < dm
    n = np.stack([np.where(b2, V[r][2], np.where(b1, V[r][1], V[r][0])) for r in range(3)], 1).astype(F32)
    c = default_viewpoint(x) if viewpoint is None else np.asarray(viewpoint, F32).reshape(3)
    dd = c[None, :] - x
    with np.errstate(all="ignore"):
        s = (n[:, 0] * dd[:, 0] + n[:, 1] * dd[:, 1]) + n[:, 2] * dd[:, 2]
    return np.where((s < 0)[:, None], -n, n).astype(F32)


# ---- 6-7. edges and weights --------------------------------------------------------------------------------------------------------
def pairs_of(table, keep_self):
    """the rows (i, L[i][t]), t = 1..k, each sorted, lexicographically unique -> [*,2] int64"""
    n, kk = table.shape
    i = np.repeat(np.arange(n, dtype=np.int64), kk - 1)
    j = table[:, 1:].astype(np.int64).reshape(-1)
    if not keep_self:
        i, j = i[i != j], j[i != j]
    key = np.unique(np.minimum(i, j) * n + np.maximum(i, j))
    return np.stack([key // n, key % n], 1)


def cloud_edges(table):
    """the unique undirected pairs a < b in lexicographic order -> [E,2] int32"""
    return pairs_of(table, keep_self=False).astype(np.int32)


def edge_weights(xyz, nrm, edges):
    x, nrm = np.asarray(xyz, F32), np.asarray(nrm, F32)
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    na, nb = nrm[a], nrm[b]
    with np.errstate(all="ignore"):
        d = (na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]
        dx = x[b] - x[a]
        c = (nb[:, 0] * dx[:, 0] + nb[:, 1] * dx[:, 1]) + nb[:, 2] * dx[:, 2]
        flip = d < 0
        d, c = np.where(flip, -d, d), np.where(flip, -c, c)
        w = F32(1.0) - d
        return np.where(c > 0, w * w, w).astype(F32)


def sorted_edges(xyz, k=10, viewpoint=None, table=None):
    """-> dict(knn [N,k+1] i32, normals [N,3] f32, edges [E,2] i32 and w [E] f32 in ascending (w, a, b), lex_edges / lex_w: the same edges
    in lexicographic order)"""
    x = np.ascontiguousarray(np.asarray(xyz, F32))
    table = knn_table(x, k) if table is None else table
    nrm = normals(x, table, viewpoint)
    edges = cloud_edges(table)
    w = edge_weights(x, nrm, edges)
    order = np.argsort(w, kind="stable")                       # the list is lexicographic: a stable sort by w gives (w, a, b)
    return dict(knn=table, normals=nrm, edges=np.ascontiguousarray(edges[order]), w=np.ascontiguousarray(w[order]), lex_edges=edges, lex_w=w)


def segment_pointcloud(xyz, k=10, k_thresh=0.01, seg_min_verts=20, viewpoint=None):
    r = sorted_edges(xyz, k, viewpoint)
    return merge(r["edges"], r["w"], np.asarray(xyz).shape[0], k_thresh, seg_min_verts)


def array_digest(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def stage_digests(r, seg):
    """what tests/golden/pcseg_expected.json holds of one run: the sha256 of every stage of sorted_edges and of the ids"""
    return {"knn": array_digest(r["knn"], "<i4"), "normals": array_digest(r["normals"], "<f4"), "edges_sorted": array_digest(r["edges"], "<i4"),
            "w_sorted": array_digest(r["w"], "<f4"), "sha256": digest(seg)}


# ---- the generated clouds ----------------------------------------------------------------------------------------------------------
def make_room_cloud(side=40, spacing=0.05, jitter=0.0, seed=0):
    """Three side x side planes (floor z = 0, walls x = 0 and y = 0) and a box standing on the floor with its five visible faces, no
    point twice, in a seeded random order -> (xyz f32 [N,3], plane id [N] of the 8 planes)."""
    h = F32(spacing)
    g = np.arange(side, dtype=np.float64)
    u, v = np.meshgrid(g, g, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    z0 = np.zeros_like(u)
    parts = [np.stack([u, v, z0], 1), np.stack([z0 - 1, v, u + 1], 1), np.stack([u, z0 - 1, v + 1], 1)]       # lattice units
    b = max(side // 4, 2)                                       # the box spans b steps each way and is b steps high
    o = side // 2 - b // 2
    e = np.arange(b + 1, dtype=np.float64)
    a, c = np.meshgrid(e, e, indexing="ij")
    parts.append(np.stack([o + a.reshape(-1), o + c.reshape(-1), np.full(a.size, float(b))], 1))             # top
    r = np.arange(1, b, dtype=np.float64)                       # side rows between the floor and the top edge
    a, c = np.meshgrid(e, r, indexing="ij")
    for x0 in (o, o + b):
        parts.append(np.stack([np.full(a.size, float(x0)), o + a.reshape(-1), c.reshape(-1)], 1))
    a, c = np.meshgrid(e[1:-1], r, indexing="ij")
    for y0 in (o, o + b):
        parts.append(np.stack([o + a.reshape(-1), np.full(a.size, float(y0)), c.reshape(-1)], 1))
    xyz = (np.concatenate(parts, 0) * float(h)).astype(F32)
    plane = np.concatenate([np.full(p.shape[0], i, np.int32) for i, p in enumerate(parts)])
    rng = np.random.RandomState(seed)
    perm = rng.permutation(xyz.shape[0])
    xyz, plane = xyz[perm], plane[perm]
    if jitter:
        xyz = (xyz + (rng.standard_normal(xyz.shape) * jitter).astype(F32)).astype(F32)
    return np.ascontiguousarray(xyz), plane


ROOMS = (("room_j0", 0.0), ("room_j5e-4", 5e-4), ("room_j2e-3", 2e-3))
DEGENERATE = ("line", "all_equal")


def case_clouds(include_large=False):
    """name -> (xyz f32 [N,3], plane ids or None); k = 10 unless the test says otherwise"""
    out = {}
    for tag, jit in ROOMS:
        out[tag] = make_room_cloud(40, 0.05, jit, seed=3)
    xyz, plane = out["room_j5e-4"]
    rng = np.random.RandomState(7)
    src = rng.choice(xyz.shape[0], 200, replace=False)
    at = np.sort(rng.choice(xyz.shape[0], 200, replace=False))
    out["room_dup"] = (np.insert(xyz, at, xyz[src], axis=0), np.insert(plane, at, plane[src]))     # 200 points twice
    slab = lambda n, s: (np.random.RandomState(s).uniform(-1, 1, (n, 3)) * np.array([1.0, 0.7, 0.05])).astype(F32)     # noqa: E731
    out["n_k_plus_1"] = (slab(11, 11), None)
    for n in (255, 256, 257):                                   # the tile edge of the kNN and of every 256-thread launch
        out["n%d" % n] = (slab(n, n), None)
    t = np.arange(64, dtype=np.float64)
    out["line"] = ((t[:, None] * np.array([0.125, 0.25, -0.0625])[None, :] + np.array([1.0, -2.0, 0.5])).astype(F32), None)
    out["all_equal"] = (np.tile(np.array([[0.75, -1.5, 2.25]], F32), (32, 1)), None)
    if include_large:
        out["room_20k"] = make_room_cloud(80, 0.025, 2.5e-4, seed=5)
    return out


def write_vertex_only_ply(path, xyz, rgb, empty_face_element=False):
    """a binary PLY with a vertex element only (or with an empty face element): what a laser scanner or a depth fusion writes"""
    v = np.zeros(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    v["x"], v["y"], v["z"], v["red"], v["green"], v["blue"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb[:, 0], rgb[:, 1], rgb[:, 2]
    hdr = "ply\nformat binary_little_endian 1.0\ncomment a laser scan\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" \
          "property uchar red\nproperty uchar green\nproperty uchar blue\n" % xyz.shape[0]
    if empty_face_element:
        hdr += "element face 0\nproperty list uchar int vertex_indices\n"
    with open(path, "wb") as f:
        f.write((hdr + "end_header\n").encode())
        f.write(v.tobytes())


def purity(seg, plane):
    """share of the points whose plane is the most frequent one of their segment"""
    _, inv = np.unique(seg, return_inverse=True)
    table = np.zeros((inv.max() + 1, int(plane.max()) + 1), np.int64)
    np.add.at(table, (inv, plane), 1)
    return float(table.max(1).sum()) / seg.shape[0]


def eigh_check(xyz, table, nrm):
    """-> (largest angle in rad between the fp32 normal and float64 eigh's smallest eigenvector over the points whose relative gap
    (l1 - l0) / l2 is at least 0.05, share of the points with that gap)"""
    x = np.asarray(xyz, np.float64)
    pts = x[table]
    q = pts - pts.mean(1, keepdims=True)
    cov = np.einsum("nti,ntj->nij", q, q)
    lam, vec = np.linalg.eigh(cov)
    with np.errstate(all="ignore"):
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    ok = gap >= 0.05
    n = np.asarray(nrm, np.float64)
    cosang = np.abs((n * vec[:, :, 0]).sum(1)) / np.linalg.norm(n, axis=1)
    ang = np.arccos(np.clip(cosang, -1.0, 1.0))
    return (float(ang[ok].max()) if ok.any() else 0.0), float(ok.mean())
