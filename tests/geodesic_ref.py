"""Geodesic distances over a graph, restated (the rules are in include/seggroup_hip.h).  Never calls the library.

    dist  = heap Dijkstra in Python floats (doubles, every addition rounded once)
    owner = the lowest seed from which a vertex is reached over TIGHT arcs (D(u) + w == D(v), D(v) finite): a minimum propagated with
            np.minimum.at to a fixed point
Where SciPy imports, scipy.sparse.csgraph.dijkstra(..., min_only=True) over the min-deduplicated arcs is asserted equal to `dist`.
The generators of the tests' graphs live here too, so that the CPU and the GPU tests speak of the same graphs.
"""
import heapq

import numpy as np

try:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra as _scipy_dijkstra
except ImportError:                                                          # pragma: no cover
    _scipy_dijkstra = None

NONE = np.iinfo(np.int32).max


def face_sides(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]]), dtype=np.int32)      # row-major: an upload reads rows


def lengths(edges, xyz):
    """the length of every row in double: d = double(p_a) - double(p_b), sqrt((d0*d0 + d1*d1) + d2*d2), one statement per operation"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    p = np.asarray(xyz)[:, :3].astype(np.float64)
    d = p[e[:, 0]] - p[e[:, 1]]
    s = d[:, 0] * d[:, 0]
    s = s + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    return np.sqrt(s)


def arcs(edges, xyz=None, weights=None):
    """[E,2] rows -> (src, dst, w) of the 2E' directed arcs, self loops dropped; w from the coordinates, the weights, or 1.0"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    assert xyz is None or weights is None
    w = lengths(e, xyz) if xyz is not None else (np.asarray(weights, np.float64) if weights is not None else np.ones(e.shape[0]))
    live = e[:, 0] != e[:, 1]
    e, w = e[live], w[live]
    return np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([w, w])


def _csr(V, src):
    order = np.argsort(src, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))])
    return order, ptr


def dijkstra(V, src, dst, w, seeds):
    order, ptr = _csr(V, src)
    to, wt = dst[order].tolist(), w[order].tolist()
    ptr = ptr.tolist()
    dist = [float("inf")] * V
    heap = []
    for s in np.flatnonzero(np.asarray(seeds) >= 0).tolist():
        dist[s] = 0.0
        heap.append((0.0, s))
    heapq.heapify(heap)
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for i in range(ptr[u], ptr[u + 1]):
            c = d + wt[i]
            if c < dist[to[i]]:
                dist[to[i]] = c
                heapq.heappush(heap, (c, to[i]))
    return np.array(dist, np.float64)


def tight_arcs(src, dst, w, dist):
    with np.errstate(invalid="ignore"):
        return np.isfinite(dist[dst]) & (dist[src] + w == dist[dst])


def _propagate(V, src, dst, start):
    """the least fixed point of O(v) = min(start(v), min over arcs (u, v) of O(u)); np.minimum.at over the arcs out of what changed"""
    o = start.copy()
    order, ptr = _csr(V, src)
    to = dst[order]
    front = np.flatnonzero(start != NONE)
    while front.size:
        n = ptr[front + 1] - ptr[front]
        at = np.repeat(ptr[front] - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
        new = o.copy()
        np.minimum.at(new, to[at], np.repeat(o[front], n))
        front = np.flatnonzero(new < o)
        o = new
    return o


def owners(V, src, dst, w, dist, seeds):
    t = tight_arcs(src, dst, w, dist)
    start = np.where(np.asarray(seeds) >= 0, np.arange(V), NONE).astype(np.int64)
    o = _propagate(V, src[t], dst[t], start)
    return np.where(o == NONE, -1, o).astype(np.int32)


def highest_owners(V, src, dst, w, dist, seeds):
    """the HIGHEST seed from which a vertex is reached over tight arcs (-1 unreached): where it differs from the owner, seeds tie"""
    t = tight_arcs(src, dst, w, dist)
    start = np.where(np.asarray(seeds) >= 0, -np.arange(V), NONE).astype(np.int64)
    o = _propagate(V, src[t], dst[t], start)
    return np.where(o == NONE, -1, -o).astype(np.int32)


def scipy_dist(V, src, dst, w, seeds):
    """SciPy's answer over the min-deduplicated arcs, or None where SciPy is missing or there is no seed"""
    idx = np.flatnonzero(np.asarray(seeds) >= 0)
    if _scipy_dijkstra is None or idx.size == 0:
        return None
    if src.size == 0:
        return np.where(np.asarray(seeds) >= 0, 0.0, np.inf)
    key = src * V + dst
    order = np.lexsort((w, key))
    first = np.concatenate([[True], key[order][1:] != key[order][:-1]])
    s, d, ww = src[order][first], dst[order][first], w[order][first]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=V))])
    g = csr_matrix((ww, d, ptr), shape=(V, V))                               # explicit zeros stay: arcs of weight 0
    return _scipy_dijkstra(g, directed=True, indices=idx, min_only=True)


def mask(dist, owner, max_dist):
    """the rule of max_dist: the unlimited result with every D > max_dist replaced by +inf / -1"""
    if max_dist is None:
        return dist, owner
    far = dist > max_dist
    return np.where(far, np.inf, dist), np.where(far, -1, owner).astype(np.int32)


def geodesic(V, seeds, edges, xyz=None, weights=None, max_dist=None, check_scipy=True):
    """-> (dist float64 [V], owner int32 [V]) by the two rules"""
    seeds = np.asarray(seeds)
    src, dst, w = arcs(edges, xyz, weights)
    dist = dijkstra(V, src, dst, w, seeds)
    if check_scipy:
        other = scipy_dist(V, src, dst, w, seeds)
        assert other is None or other.tobytes() == dist.tobytes(), "SciPy's dijkstra and the heap disagree"
    return mask(dist, owners(V, src, dst, w, dist, seeds), max_dist)


def relax_shuffled(V, src, dst, w, seeds, rng, share=0.3):
    """the in-place relaxation over random arc subsets in random order, to the fixed point (a full sweep that changes nothing ends it)"""
    dist = np.where(np.asarray(seeds) >= 0, 0.0, np.inf)
    n = src.shape[0]
    while True:
        for _ in range(4):
            pick = rng.permutation(n)[:max(1, int(share * n))]
            for i in pick.tolist():
                c = dist[src[i]] + w[i]
                if c < dist[dst[i]]:
                    dist[dst[i]] = c
        before = dist.copy()
        np.minimum.at(dist, dst, before[src] + w)
        if dist.tobytes() == before.tobytes():
            return dist


def stats(V, seeds, edges, xyz=None, weights=None, max_dist=None):
    """what sg_graph_geodesic_stats must say of the call, launches aside: (arcs kept, tight arcs, reached)"""
    src, dst, w = arcs(edges, xyz, weights)
    dist, owner = geodesic(V, seeds, edges, xyz, weights, max_dist, check_scipy=False)
    return int(src.shape[0]), int(tight_arcs(src, dst, w, dist).sum()), int((owner >= 0).sum())


# ---- the graphs of the tests --------------------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny, seed=0, jitter=0.3, step=0.05):
    """a triangulated nx x ny sheet with jittered float32 coordinates -> (xyz float32 [nx*ny,3], faces int32 [2(nx-1)(ny-1),3])"""
    rng = np.random.RandomState(seed)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    xyz = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3).astype(np.float64) * step
    xyz += rng.uniform(-jitter * step, jitter * step, xyz.shape)
    v = (gx * ny + gy)[:-1, :-1].reshape(-1)
    faces = np.concatenate([np.stack([v, v + ny, v + 1], 1), np.stack([v + 1, v + ny, v + ny + 1], 1)])
    return xyz.astype(np.float32), faces.astype(np.int32)


def unit_grid(n):
    """the n x n grid graph -> edges int32 [2n(n-1),2]; vertex (i, j) is i*n + j"""
    v = np.arange(n * n).reshape(n, n)
    return np.concatenate([np.stack([v[:-1].ravel(), v[1:].ravel()], 1), np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], 1)]).astype(np.int32)


def path(n, perm=None):
    """the path 0-1-..-(n-1); with `perm` vertex k of the path is perm[k]"""
    e = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    return (e if perm is None else np.asarray(perm)[e]).astype(np.int32)


def star(degree):
    """vertex 0 joined to 1..degree"""
    return np.stack([np.zeros(degree, np.int64), np.arange(1, degree + 1)], 1).astype(np.int32)


def random_graph(V, E, seed, isolated=0):
    """E rows with duplicates (of differing weights), both orientations and self loops -> (edges int32 [E,2], weights float64 [E]);
    quantised weights, so that equal sums -- ties -- occur; the last `isolated` vertices have no row"""
    rng = np.random.RandomState(seed)
    e = rng.randint(0, V - isolated, (E, 2))
    dup = rng.randint(0, E, E // 10)
    e[:E // 10] = e[dup][:, ::-1]                                            # a tenth are other rows turned round
    e[E // 10:E // 10 + E // 50, 1] = e[E // 10:E // 10 + E // 50, 0]          # self loops
    w = rng.randint(0, 8, E) / 4.0                                           # zero weights among them
    return e.astype(np.int32), w.astype(np.float64)
