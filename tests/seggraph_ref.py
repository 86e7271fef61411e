"""NumPy statement of sg_segment_graph and the seeded cases tests/test_seggraph_ref.py (CPU) and
tests/test_gpu_seggraph.py (GPU) share.  Nothing here imports the package."""
import numpy as np

E_SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 12289)      # the sort's tile is 4,096 keys, the scans' 2,048
S_SIZES = (1, 2, 3, 1024, 2049, 1 << 20)                                # 0, 2, 4, 20, 24 and 40 key bits
SHAPES = ("inside", "one_pair", "distinct", "negative", "loops", "mirrored", "mesh", "shuffled")


def segment_graph(adj, seg, S=None):
    """For every row (u, v): a = seg[u], b = seg[v]; the row counts when a >= 0, b >= 0 and a != b.  -> (pairs int32 [P,2]: the distinct
    (min, max) ascending, cross int32 [P]: the rows behind each pair).  Vertex indices must lie inside the scan and segment numbers
    below S: the library refuses the rest, the statement asserts it."""
    adj = np.asarray(adj, np.int64).reshape(-1, 2)
    seg = np.asarray(seg, np.int64).reshape(-1)
    assert adj.size == 0 or (adj.min() >= 0 and adj.max() < seg.shape[0])
    assert S is None or seg.size == 0 or seg.max() < S
    a, b = seg[adj[:, 0]], seg[adj[:, 1]]
    keep = (a >= 0) & (b >= 0) & (a != b)
    rows = np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], axis=1)
    if rows.shape[0] == 0:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    pairs, cross = np.unique(rows, axis=0, return_counts=True)
    return pairs.astype(np.int32), cross.astype(np.int32)


def bits_for(n):
    """bits that hold 0..n-1: a key is lo << bits_for(S) | hi"""
    b = 0
    while (1 << b) < n:
        b += 1
    return b


def size_case(E, S, seed=0):
    """-> adj int64 [E,2], seg int32 [V]: random rows over V = 3000 vertices whose segments are drawn from all of 0..S-1 with the two ends
    of the range always present (the highest key bits are in use), one vertex in fifty without a segment; a tenth of the rows (u, u), a
    tenth copies of other rows, half of those turned round."""
    rng = np.random.default_rng([47, E, S % 9973, seed])
    V = 3000
    seg = rng.integers(0, S, V).astype(np.int32)
    seg[:2] = (0, S - 1)
    seg[rng.choice(np.arange(2, V), V // 50, replace=False)] = -1
    adj = rng.integers(0, V, (E, 2)).astype(np.int64)
    if E >= 10:
        k = E // 10
        adj[:k, 1] = adj[:k, 0]
        adj[k:2 * k] = adj[2 * k:3 * k]
        adj[k:k + k // 2] = adj[k:k + k // 2, ::-1]
    if E >= 1:
        adj[-1] = (0, 1)                                            # the pair (0, S-1) when S > 1
    return adj, seg


def lattice(w, h, cell):
    """a w x h vertex lattice in cell x cell segments -> (mesh-ordered edges int64 [E,2]: right, down and diagonal of every vertex, seg
    int32 [w*h])"""
    col, row = np.meshgrid(np.arange(w), np.arange(h))
    col, row = col.reshape(-1), row.reshape(-1)
    v = row * w + col
    seg = ((row // cell) * -(-w // cell) + col // cell).astype(np.int32)
    right, down = col + 1 < w, row + 1 < h
    adj = np.concatenate([np.stack([v[right], v[right] + 1], 1), np.stack([v[down], v[down] + w], 1),
                          np.stack([v[right & down], v[right & down] + w + 1], 1)]).astype(np.int64)
    return adj, seg


def shape_case(shape, seed=0):
    """-> adj, seg, S for one of SHAPES"""
    rng = np.random.default_rng([53, SHAPES.index(shape), seed])
    if shape == "inside":                                           # every row inside one segment: P = 0
        seg = np.repeat(np.arange(40, dtype=np.int32), 50)
        u = rng.integers(0, 2000, 5000)
        adj = np.stack([u, (u // 50) * 50 + rng.integers(0, 50, 5000)], 1).astype(np.int64)
        return adj, seg, 40
    if shape == "one_pair":                                         # every row on one pair: cross = E
        seg = np.array([5] * 100 + [9] * 100, np.int32)
        adj = np.stack([rng.integers(0, 100, 5000), rng.integers(100, 200, 5000)], 1).astype(np.int64)
        adj[::3] = adj[::3, ::-1]
        return adj, seg, 10
    if shape == "distinct":                                         # every row a distinct pair: vertex s is segment s
        S = 120
        a, b = np.triu_indices(S, 1)
        adj = np.stack([a, b], 1).astype(np.int64)
        adj = adj[rng.permutation(adj.shape[0])]
        return adj, np.arange(S, dtype=np.int32), S
    if shape == "negative":                                         # a third of the vertices without a segment (-1, and lower)
        seg = rng.integers(0, 30, 3000).astype(np.int32)
        seg[rng.choice(3000, 1000, replace=False)] = rng.choice([-1, -7, -2 ** 31], 1000)
        return rng.integers(0, 3000, (6000, 2)).astype(np.int64), seg, 30
    if shape == "loops":                                            # rows (u, u) among the others
        seg = rng.integers(0, 30, 3000).astype(np.int32)
        adj = rng.integers(0, 3000, (6000, 2)).astype(np.int64)
        adj[::2, 1] = adj[::2, 0]
        return adj, seg, 30
    if shape == "mirrored":                                         # both orientations and duplicates: every row four times
        seg = rng.integers(0, 30, 3000).astype(np.int32)
        adj = rng.integers(0, 3000, (1500, 2)).astype(np.int64)
        adj = np.concatenate([adj, adj[:, ::-1], adj, adj[:, ::-1]])
        return adj, seg, 30
    adj, seg = lattice(90, 70, 8)                                   # a mesh: nine rows in ten inside one segment
    if shape == "shuffled":
        adj = adj[rng.permutation(adj.shape[0])]
        adj[::2] = adj[::2, ::-1]
    return adj, seg, int(seg.max()) + 1


def dense_matrix(pairs, S):
    """the reference's [S,S] 0/1 matrix of a pair list"""
    m = np.zeros((S, S))
    p = np.asarray(pairs).reshape(-1, 2)
    m[p[:, 0], p[:, 1]] = 1
    m[p[:, 1], p[:, 0]] = 1
    return m


def cluster_lists(off, members):
    return [members[off[c]:off[c + 1]].tolist() for c in range(len(off) - 1)]
