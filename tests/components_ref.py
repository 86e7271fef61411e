"""Connected components of a scan's graph: the statement of DESIGN.md 8j in NumPy -- the reference that the library's kernels are held to
bit for bit (tests/test_components_ref.py, tests/test_gpu_components.py, tools/capture_components.py).

The pairs come from an edge list, from the three sides of every face, or from a kNN table cut at a length; the cut is float32, one NumPy
call per operation, in the order 8j writes it.  The union-find is a plain Python loop whose ids are "the lowest index wins".  Nothing here
calls the library.
"""
import hashlib

import numpy as np

F32 = np.float32


def _check(idx, num_vertices, what):
    idx = np.asarray(idx, np.int64)
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= num_vertices):
        raise ValueError("%s: a vertex index outside 0..%d" % (what, num_vertices - 1))
    return idx


def pairs_from_edges(edges, num_vertices):
    e = _check(np.asarray(edges).reshape(-1, 2), num_vertices, "edges")
    return e[:, 0], e[:, 1]


def pairs_from_faces(faces, num_vertices):
    f = _check(np.asarray(faces).reshape(-1, 3), num_vertices, "faces")
    return np.concatenate([f[:, 0], f[:, 1], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2], f[:, 2]])


def pairs_from_knn(xyz, table, max_edge=np.inf):
    """(i, L[i][t]), t = 1.., with j != i and d2 <= r2; entry 0 is skipped whatever it holds"""
    pts = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    table = np.asarray(table)
    n, row = table.shape
    if pts.shape[0] != n or row < 2:
        raise ValueError("knn: a table [N, >= 2] and N points are needed")
    r = F32(max_edge)
    if not r > 0:
        raise ValueError("knn: max_edge must be +inf or finite and positive")
    if not np.isfinite(pts).all():
        raise ValueError("knn: a coordinate is not finite")
    i = np.repeat(np.arange(n, dtype=np.int64), row - 1)
    j = _check(table[:, 1:].reshape(-1), n, "knn")
    with np.errstate(over="ignore"):
        r2 = F32(r * r)
        d = pts[j] - pts[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == F32
    keep = (j != i) & (d2 <= r2)
    return i[keep], j[keep]


def components(num_vertices, a, b, labels=None):
    """-> comp int32 [V] (the lowest index of the component), size int32 [V], C"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if labels is not None:
        lab = np.asarray(labels).reshape(-1)
        if lab.shape[0] != num_vertices:
            raise ValueError("labels: one value per vertex is needed")
        same = lab[a] == lab[b]
        a, b = a[same], b[same]
    parent = list(range(num_vertices))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)                  # the lowest index wins: a component's root is its minimum
    comp = np.fromiter((find(v) for v in range(num_vertices)), np.int32, num_vertices)
    size = np.bincount(comp, minlength=num_vertices)[comp].astype(np.int32)
    return comp, size, int((comp == np.arange(num_vertices)).sum())


def from_edges(num_vertices, edges, labels=None):
    return components(num_vertices, *pairs_from_edges(edges, num_vertices), labels=labels)


def from_faces(num_vertices, faces, labels=None):
    return components(num_vertices, *pairs_from_faces(faces, num_vertices), labels=labels)


def from_knn(xyz, table, max_edge=np.inf, labels=None):
    return components(np.asarray(table).shape[0], *pairs_from_knn(xyz, table, max_edge), labels=labels)


def sizes_desc(comp):
    """the component sizes, largest first"""
    return sorted(np.bincount(comp)[np.unique(comp)].tolist(), reverse=True)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


# ---- what `clean` does with the components ---------------------------------------------------------------------------
def keep_mask(comp, size, min_verts=None, largest=False):
    comp, size = np.asarray(comp), np.asarray(size)
    if largest:
        big = size == size.max()
        return comp == comp[big].min()
    return size >= min_verts


def clean_arrays(keep, faces):
    """-> kept int32 [M] ascending, new_of_old int32 [V] (-1 where dropped), the faces whose three vertices are kept, renumbered, in order"""
    keep = np.asarray(keep, bool)
    kept = np.flatnonzero(keep).astype(np.int32)
    new_of_old = np.full(keep.shape[0], -1, np.int32)
    new_of_old[kept] = np.arange(kept.shape[0], dtype=np.int32)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    whole = keep[faces].all(1) if faces.shape[0] else np.zeros(0, bool)
    return kept, new_of_old, new_of_old[faces[whole]].reshape(-1, 3)


# ---- the generated cases both test files share ---------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257)
CHAIN = 4097
STAR_LEAVES = 5000
CLIQUE = 64
RANDOM_V, RANDOM_E, RANDOM_SEED = 20000, 15000, 17
ISLAND_PATCHES = ((3, (1, 3), 100, (3.0, 3.0, 3.0)), (12, (3, 4), 500, (-2.0, 1.0, 0.5)), (60, (6, 10), 900, (1.0, -2.0, 2.5)))
SPECKS = ((8, (3.0, 3.0, 3.0), 1000), (15, (-2.0, 1.0, 0.5), 3000), (3, (1.0, -2.0, 2.5), None))
CUTS = (np.inf, 0.1, 0.06)


def path_edges(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int32)


def _grid_patch(rows, cols, origin, step=0.04):
    """rows x cols vertices on a plane, triangulated; a single row of three is one triangle"""
    u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    xyz = (np.stack([u.reshape(-1), v.reshape(-1), np.zeros(u.size)], 1) * step + np.asarray(origin)).astype(F32)
    if rows == 1:
        return xyz, np.array([[0, 1, 2]], np.int32)
    idx = np.arange(rows * cols).reshape(rows, cols)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, :-1].reshape(-1), idx[1:, 1:].reshape(-1)
    return xyz, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)], 0).astype(np.int32)


def island_mesh():
    """a room of 1,200 vertices and three floating patches of 3, 12 and 60 vertices, their vertex blocks interleaved with the room's
    -> dict(xyz, rgb, faces, seg_indices, patch int32 [V]: 0 = room, else the patch's vertex count)"""
    from seggroup_amd import synthetic
    s = synthetic.make_room_scan(40, 30, 5, jitter=1e-3)
    blocks, cut = [], 0                                         # (xyz, rgb, seg, faces in block-local ids, tag)
    room_new = np.empty(s.xyz.shape[0], np.int64)
    pos, order = 0, []
    for n, (rows, cols), at, origin in ISLAND_PATCHES:
        order.append(("room", cut, at))
        order.append(("patch", n, (rows, cols, origin)))
        cut = at
    order.append(("room", cut, s.xyz.shape[0]))
    xyz, rgb, seg, patch, faces = [], [], [], [], []
    for kind, p, q in order:
        if kind == "room":
            room_new[p:q] = np.arange(pos, pos + q - p)
            xyz.append(s.xyz[p:q]); rgb.append(s.rgb[p:q]); seg.append(s.seg_indices[p:q]); patch.append(np.zeros(q - p, np.int32))
            pos += q - p
        else:
            pxyz, pf = _grid_patch(q[0], q[1], q[2])
            assert pxyz.shape[0] == p
            xyz.append(pxyz); rgb.append(np.full((p, 3), 40 + p, np.uint8)); seg.append(np.full(p, 100000 + p, np.int32))
            patch.append(np.full(p, p, np.int32))
            faces.append(pf + pos)
            pos += p
    faces.insert(0, room_new[s.faces.astype(np.int64)])
    return dict(xyz=np.ascontiguousarray(np.concatenate(xyz, 0), dtype=F32), rgb=np.ascontiguousarray(np.concatenate(rgb, 0)),
                faces=np.ascontiguousarray(np.concatenate(faces, 0), dtype=np.int32), seg_indices=np.concatenate(seg).astype(np.int32),
                patch=np.concatenate(patch))


def speck_cloud():
    """pcseg_ref's jittered room cloud with three specks of 8, 15 and 3 points -> (xyz f32 [5307,3], speck int32 [N]: 0 = room)"""
    import pcseg_ref
    room, _ = pcseg_ref.make_room_cloud(40, 0.05, 5e-4, seed=3)
    rng = np.random.RandomState(11)
    specks = [(np.asarray(o) + rng.uniform(0, 0.04, (n, 3))).astype(F32) for n, o, _ in SPECKS]
    parts, tags, cut = [], [], 0
    for (n, _, at), pts in zip(SPECKS, specks):
        at = room.shape[0] if at is None else at
        parts += [room[cut:at], pts]
        tags += [np.zeros(at - cut, np.int32), np.full(n, n, np.int32)]
        cut = at
    parts.append(room[cut:]); tags.append(np.zeros(room.shape[0] - cut, np.int32))
    return np.ascontiguousarray(np.concatenate(parts, 0), dtype=F32), np.concatenate(tags)


def case_graphs():
    """name -> dict(V, edges=[E,2] | faces=[F,3], labels=None | [V]): every case that needs no kNN table"""
    import overseg_ref
    out = {}
    for n in SIZES:
        out["empty_%d" % n] = dict(V=n, edges=np.zeros((0, 2), np.int32))
        out["path_%d" % n] = dict(V=n, edges=path_edges(n))
    chain = path_edges(CHAIN)
    rng = np.random.RandomState(5)
    out["chain_ascending"] = dict(V=CHAIN, edges=chain)
    out["chain_descending"] = dict(V=CHAIN, edges=np.ascontiguousarray(chain[::-1]))
    out["chain_shuffled"] = dict(V=CHAIN, edges=np.ascontiguousarray(chain[rng.permutation(CHAIN - 1)]))
    perm = rng.permutation(CHAIN).astype(np.int32)            # vertex ids permuted: the minimum sits mid-chain
    out["chain_permuted"] = dict(V=CHAIN, edges=np.ascontiguousarray(perm[chain]))
    out["chain_permuted_shuffled"] = dict(V=CHAIN, edges=np.ascontiguousarray(perm[chain][rng.permutation(CHAIN - 1)]))
    hub = STAR_LEAVES
    out["star_hub_highest"] = dict(V=STAR_LEAVES + 1, edges=np.stack([np.arange(STAR_LEAVES), np.full(STAR_LEAVES, hub)], 1).astype(np.int32))
    a, b = np.triu_indices(CLIQUE, 1)
    clique = np.stack([a, b], 1)
    out["two_cliques_bridge_last"] = dict(V=2 * CLIQUE, edges=np.concatenate([clique, clique + CLIQUE, [[CLIQUE - 1, CLIQUE]]], 0).astype(np.int32))
    rng = np.random.RandomState(RANDOM_SEED)
    rnd = rng.randint(0, RANDOM_V, (RANDOM_E, 2)).astype(np.int32)
    out["random"] = dict(V=RANDOM_V, edges=rnd)
    loops = np.repeat(rng.randint(0, RANDOM_V, 500), 2).reshape(-1, 2)
    noisy = np.concatenate([rnd, rnd[:, ::-1], rnd, loops, rnd, rnd[:, ::-1]], 0).astype(np.int32)
    out["random_noisy"] = dict(V=RANDOM_V, edges=np.ascontiguousarray(noisy[rng.permutation(noisy.shape[0])]), same_as="random")
    for name, (xyz, faces) in overseg_ref.case_meshes().items():
        out["mesh_" + name] = dict(V=xyz.shape[0], faces=faces)
        out["mesh_edges_" + name] = dict(V=xyz.shape[0], edges=overseg_ref.mesh_edges(faces, xyz.shape[0]), same_as="mesh_" + name)
    isl = island_mesh()
    out["island"] = dict(V=isl["xyz"].shape[0], faces=isl["faces"])
    from seggroup_amd import synthetic
    s = synthetic.make_room_scan(40, 30, 5, jitter=1e-3)
    v = s.xyz.shape[0]
    out["filter_stripes"] = dict(V=v, faces=s.faces, labels=s.seg_indices.astype(np.int32))
    out["filter_all_equal"] = dict(V=v, faces=s.faces, labels=np.full(v, -7, np.int32), same_as="filter_none")
    out["filter_none"] = dict(V=v, faces=s.faces)
    out["filter_all_distinct"] = dict(V=v, faces=s.faces, labels=(np.arange(v) - v // 2).astype(np.int32))
    return out


def solve(case):
    """the statement on one entry of case_graphs()"""
    if "faces" in case:
        return from_faces(case["V"], case["faces"], case.get("labels"))
    return from_edges(case["V"], case["edges"], case.get("labels"))


# counts measured on the CPU (8j): name -> (C, the sizes largest first, or None)
MESH_COUNTS = {"mesh_room_j0": (1, None), "mesh_room_j5e-4": (1, None), "mesh_room_j2e-3": (1, None), "mesh_raw_scan": (1, None),
               "mesh_isolated": (4, [1200, 1, 1, 1]), "mesh_one_vertex": (1, [1]), "mesh_no_edges": (50, [1] * 50),
               "island": (4, [1200, 60, 12, 3])}
