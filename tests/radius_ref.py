"""The radius graph of a point cloud: the statement of DESIGN.md 8k in NumPy -- the reference that sg_radius_count_grid and
sg_components_radius are held to bit for bit (tests/test_radius_ref.py, tests/test_gpu_radius.py, tools/capture_radius.py).

The pair predicate is 8j's, over ALL pairs: d = p_j - p_i, d2 = (d0*d0 + d1*d1) + d2*d2 in float32 with one NumPy call per operation,
r2 = radius * radius rounded once; the pair counts when j != i and d2 <= r2.  The pairs are evaluated in chunked all-pairs blocks; there
is no grid here.  count[i] is the number of j that pass for i; the components are components_ref's union-find in which the lowest index
wins.  Nothing here calls the library.
"""
import numpy as np

import components_ref as CR

F32 = np.float32
CHUNK = 512


def _points(xyz):
    pts = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    if pts.ndim != 2 or pts.shape[0] < 1:
        raise ValueError("radius: at least one point [N, >= 3] is needed")
    if not np.isfinite(pts).all():
        raise ValueError("radius: a coordinate is not finite")
    return pts


def r2_of(radius):
    r = F32(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError("radius: the radius must be finite and positive")
    with np.errstate(over="ignore", under="ignore"):
        r2 = F32(r * r)
    if not (np.isfinite(r2) and r2 >= F32(2.0) ** -100):
        raise ValueError("radius: the square of the radius must be finite and at least 2^-100")
    return r2


def blocks(xyz, radius, chunk=CHUNK, threads=4):
    """yields (i0, passing [rows, N] bool) over chunks of rows, in order: the predicate exactly as 8k writes it (the chunks are evaluated
    on a few threads; NumPy releases the lock)"""
    import concurrent.futures
    pts = _points(xyz)
    r2 = r2_of(radius)
    n = pts.shape[0]
    cols = np.arange(n)

    def one(i0):
        q = pts[i0:i0 + chunk]
        with np.errstate(over="ignore", under="ignore"):
            d0 = pts[None, :, 0] - q[:, None, 0]
            d1 = pts[None, :, 1] - q[:, None, 1]
            d2 = pts[None, :, 2] - q[:, None, 2]
            dd = (d0 * d0 + d1 * d1) + d2 * d2
        assert dd.dtype == F32
        return i0, (dd <= r2) & (cols[None, :] != (i0 + np.arange(q.shape[0]))[:, None])

    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        starts = list(range(0, n, chunk))
        for at in range(0, len(starts), 2 * threads):           # a bounded number of chunks in memory
            yield from pool.map(one, starts[at:at + 2 * threads])


def count(xyz, radius):
    """-> int32 [N]: the number of j != i with d2 <= r2"""
    out = [ok.sum(1) for _, ok in blocks(xyz, radius)]
    return np.concatenate(out).astype(np.int32)


def pairs(xyz, radius):
    """-> (a, b) int64 with a < b: every edge of the radius graph once, in row order"""
    a, b = [], []
    for i0, ok in blocks(xyz, radius):
        i, j = np.nonzero(ok)
        up = j > i + i0
        a.append(i[up] + i0)
        b.append(j[up])
    return np.concatenate(a).astype(np.int64), np.concatenate(b).astype(np.int64)


def solve(xyz, radius, labels=None):
    """-> (count int32 [N], comp int32 [N], size int32 [N], C).  The union-find is components_ref's; chunk by chunk the pairs whose ends
    are in one component already are left out first (vectorised on the flattened parents) and the loop runs on the component ids that
    are left, which cannot change a component, so that a radius with millions of pairs stays a matter of seconds."""
    pts = _points(xyz)
    n = pts.shape[0]
    lab = None if labels is None else np.asarray(labels).reshape(-1)
    if lab is not None and lab.shape[0] != n:
        raise ValueError("labels: one value per point is needed")
    comp = np.arange(n, dtype=np.int64)
    cnt = np.zeros(n, np.int32)
    for i0, ok in blocks(pts, radius):
        rows = ok.shape[0]
        cnt[i0:i0 + rows] = ok.sum(1)
        i, j = np.nonzero(ok & (comp[None, :] != comp[i0:i0 + rows, None]))
        i = i + i0
        if lab is not None:
            same = lab[i] == lab[j]
            i, j = i[same], j[same]
        if i.size == 0:
            continue
        ra, rb = comp[i], comp[j]
        links = np.unique(np.stack([np.minimum(ra, rb), np.maximum(ra, rb)], 1), axis=0)
        roots = np.unique(links)                                 # the union-find runs on the component ids in play; the lowest id wins
        at = np.searchsorted(roots, links)
        merged, _, _ = CR.components(roots.shape[0], at[:, 0], at[:, 1])
        to = np.arange(n, dtype=np.int64)
        to[roots] = roots[merged]
        comp = to[comp]
    comp = comp.astype(np.int32)
    size = np.bincount(comp, minlength=n)[comp].astype(np.int32)
    return cnt, comp, size, int((comp == np.arange(n)).sum())


def from_pairs(xyz, radius, labels=None):
    """the plain form: the explicit pair list through components_ref.components (small clouds)"""
    a, b = pairs(xyz, radius)
    return CR.components(np.asarray(xyz).shape[0], a, b, labels=labels)


# ---- the cross-check of the fixture: a kd-tree in float64 ---------------------------------------------------------------------------------
def kdtree(xyz, radius):
    """-> (count, comp, C, nearest: the smallest |d/r - 1| over all pairs, float64).  query_pairs + csgraph.connected_components on the
    float64 values of the float32 coordinates and the float64 value of the float32 radius."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    pts = _points(xyz).astype(np.float64)
    n = pts.shape[0]
    r = float(F32(radius))
    tree = cKDTree(pts)
    near = tree.query_pairs(r * (1.0 + 1e-5), output_type="ndarray")
    d = np.sqrt(((pts[near[:, 0]] - pts[near[:, 1]]) ** 2).sum(1)) if near.shape[0] else np.zeros(0)
    nearest = float(np.abs(d / r - 1.0).min()) if d.size else np.inf
    e = near[d <= r]
    cnt = (np.bincount(e[:, 0], minlength=n) + np.bincount(e[:, 1], minlength=n)).astype(np.int32)
    c, lab = connected_components(coo_matrix((np.ones(e.shape[0], np.int8), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    first = np.full(c, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return cnt, first[lab].astype(np.int32), int(c), nearest


# ---- the generated cases both test files and the capture share ------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
LINE_STEP = 0.1
LINE_RADII = {"none": 0.05, "path": 0.12, "all": 100.0}        # no edges | i -- i + 1 only | everything joined
SPECK_RADII = (0.04, 0.06)           # in the fixture: below the lattice spacing of 0.05 | just above it
# The third radius joins the nearest speck (15 points, 1.9107 from the room) and not the next (1.9956).  625,205 pairs of the cloud have a
# float64 distance between those two values, the widest gap between neighbouring distances there is 1.46e-6 relative, so NO radius in that
# range keeps every pair 1e-6 away and tools/capture_radius.py rightly refuses each of them.  This one sits in the middle of that widest
# gap (7.3e-7 to either side); the GPU test holds it to the NumPy statement directly, the fixture does not hold it.
SPECK_JOIN_RADIUS = 1.9590621
CLUMP_RADIUS, CLUMP_K = 0.02, 10
IMPORTED_RADIUS = {"room_j0": 0.06, "room_j5e-4": 0.06, "room_j2e-3": 0.06, "room_dup": 0.06, "n_k_plus_1": 0.3, "n255": 0.15, "n256": 0.15,
                   "n257": 0.15, "line": 0.3, "all_equal": 0.01, "room_20k": 0.03}


def jittered_line(n, seed=None):
    """n points 0.1 apart along a slanted direction, jittered by at most 0.005 per axis, in a seeded random order"""
    rng = np.random.RandomState(1000 + n if seed is None else seed)
    t = np.arange(n, dtype=np.float64) * LINE_STEP
    pts = t[:, None] * np.array([0.6, -0.64, 0.48])[None, :] + np.array([-3.0, 2.0, 0.25]) + rng.uniform(-0.005, 0.005, (n, 3))
    return np.ascontiguousarray(pts[rng.permutation(n)], dtype=F32)


def two_clumps():
    """two clumps of 12 points, each within 1e-4 of its centre, the centres 0.01 apart: the case the kNN graph at k = 10 gets wrong"""
    rng = np.random.RandomState(21)
    c = np.array([[0.5, 0.25, -0.75], [0.51, 0.25, -0.75]])
    off = rng.uniform(-1.0, 1.0, (2, 12, 3))
    off *= 0.9e-4 / np.sqrt(3.0)
    pts = (c[:, None, :] + off).reshape(24, 3)
    return np.ascontiguousarray(pts[rng.permutation(24)], dtype=F32)


def stripes(n):
    """labels in bands along x: the plane-stripe filter of the speck cloud"""
    xyz, _ = CR.speck_cloud()
    assert xyz.shape[0] == n
    return np.floor(xyz[:, 0] / F32(0.25)).astype(np.int32)


def digest(a):
    return CR.digest(a)


def entry(cnt, comp, c):
    return {"N": int(comp.shape[0]), "C": int(c), "sizes": CR.sizes_desc(comp)[:10], "comp_sha256": digest(comp), "count_sha256": digest(cnt),
            "pairs": int(cnt.astype(np.int64).sum() // 2)}


def fixture_cases():
    """name -> (xyz, radius): every (cloud, radius) the committed fixture holds"""
    import pcseg_ref
    out = {}
    for n in SIZES:
        for tag, r in LINE_RADII.items():
            out["line_%d_%s" % (n, tag)] = (jittered_line(n), r)
    out["two_clumps"] = (two_clumps(), CLUMP_RADIUS)
    xyz, _ = CR.speck_cloud()
    for r in SPECK_RADII:
        out["specks_%g" % r] = (xyz, r)
    for name, (cloud, _) in pcseg_ref.case_clouds(include_large=True).items():
        out["cloud_" + name] = (cloud, IMPORTED_RADIUS[name])
    return out
