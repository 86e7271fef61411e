"""The mesh over-segmenter's specification restated in NumPy float32 -- the reference that the library's device stages
and host chain are held to bit for bit (tests/test_overseg_host.py, tests/test_gpu_overseg.py, tools/capture_overseg.py).

Every array is float32 and every operation is one NumPy call on float32 operands, so each is rounded once, in the order the
specification writes it; NumPy's float32 sqrt and division are correctly rounded.  The ordered sums are np.add.at over the (vertex,
face) pairs in face-major order; the merge chain is a plain Python loop.  Nothing here calls the library.
"""
import hashlib

import numpy as np

F32 = np.float32


def _normalise(n):
    """n / sqrt((x*x + y*y) + z*z) per row; exact zeros where the length is not positive."""
    n = np.ascontiguousarray(n, dtype=F32)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    out = np.zeros_like(n)
    ok = length > 0
    with np.errstate(all="ignore"):
        out[ok] = n[ok] / length[ok, None]
    return out


def face_normals(xyz, faces):
    xyz, faces = np.asarray(xyz, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    p0 = xyz[faces[:, 0]]
    e1, e2 = xyz[faces[:, 1]] - p0, xyz[faces[:, 2]] - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
    return _normalise(n)


def vertex_normals(xyz, faces):
    xyz, faces = np.asarray(xyz, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    fn = face_normals(xyz, faces)
    acc = np.zeros((xyz.shape[0], 3), F32)
    # pair 3f + c adds face f's normal to vertex faces[f, c]: per vertex that is ascending face index, twice for a face that names it twice
    np.add.at(acc, faces.reshape(-1), np.repeat(fn, 3, axis=0))
    return _normalise(acc)


def mesh_edges(faces, num_vertices):
    """unique undirected a < b over the three sides of every face, a != b, in lexicographic order -> [E,2] int32"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    pairs = np.concatenate([faces[:, [0, 1]], faces[:, [0, 2]], faces[:, [1, 2]]], 0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    lo, hi = pairs.min(1), pairs.max(1)
    key = np.unique(lo * np.int64(num_vertices) + hi)
    return np.stack([key // num_vertices, key % num_vertices], 1).astype(np.int32)


def edge_weights(xyz, normals, edges):
    xyz, nrm = np.asarray(xyz, F32), np.asarray(normals, F32)
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    na, nb = nrm[a], nrm[b]
    d = (na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]
    w = F32(1.0) - d
    dx = xyz[b] - xyz[a]
    c = (nb[:, 0] * dx[:, 0] + nb[:, 1] * dx[:, 1]) + nb[:, 2] * dx[:, 2]
    w = np.where(c > 0, w * w, w).astype(F32)
    return w


def sorted_edges(xyz, faces):
    """-> normals [V,3] f32, edges [E,2] i32 and w [E] f32 in ascending (w, a, b)"""
    xyz = np.asarray(xyz, F32)
    nrm = vertex_normals(xyz, faces)
    edges = mesh_edges(faces, xyz.shape[0])
    w = edge_weights(xyz, nrm, edges)
    order = np.argsort(w, kind="stable")                       # the list is lexicographic: a stable sort by w gives (w, a, b)
    return nrm, np.ascontiguousarray(edges[order]), np.ascontiguousarray(w[order])


def merge(edges, w, num_vertices, k_thresh=0.01, seg_min_verts=20):
    """the two ordered passes and the ids -> int32 [V]"""
    k = F32(k_thresh)
    parent = list(range(num_vertices))
    size = [1] * num_vertices
    thr = [k] * num_vertices

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    ea, eb = edges[:, 0].tolist(), edges[:, 1].tolist()
    ws = [F32(x) for x in np.asarray(w, F32)]
    for a, b, x in zip(ea, eb, ws):
        ra, rb = find(a), find(b)
        if ra != rb and x <= thr[ra] and x <= thr[rb]:
            parent[rb] = ra                                    # which root survives does not matter: the ids below do not depend on it
            size[ra] += size[rb]
            thr[ra] = F32(x + F32(k / F32(size[ra])))
    for a, b in zip(ea, eb):
        ra, rb = find(a), find(b)
        if ra != rb and (size[ra] < seg_min_verts or size[rb] < seg_min_verts):
            parent[rb] = ra
            size[ra] += size[rb]
    lowest, out = {}, np.empty(num_vertices, np.int32)
    for v in range(num_vertices):
        out[v] = lowest.setdefault(find(v), v)
    return out


def segment_mesh(xyz, faces, k_thresh=0.01, seg_min_verts=20):
    xyz = np.asarray(xyz, F32)
    _, edges, w = sorted_edges(xyz, faces)
    return merge(edges, w, xyz.shape[0], k_thresh, seg_min_verts)


def digest(seg):
    return hashlib.sha256(np.ascontiguousarray(seg, dtype="<i4").tobytes()).hexdigest()


# ---- the generated cases both test files and the capture tool share --------------------------------------------------------------
def case_meshes(include_large=False):
    """name -> (xyz f32 [V,3], faces i32 [F,3])"""
    from seggroup_amd import synthetic
    out = {}
    for tag, jit in (("room_j0", 0.0), ("room_j5e-4", 5e-4), ("room_j2e-3", 2e-3)):
        s = synthetic.make_room_scan(120, 100, 3, jitter=jit)
        out[tag] = (s.xyz, s.faces)
    s = synthetic.make_raw_scan(160, 120, 7)                   # duplicated vertices and degenerate faces
    out["raw_scan"] = (s.xyz, s.faces)
    s = synthetic.make_room_scan(40, 30, 5, jitter=1e-3)
    iso = np.array([[9.0, 9.0, 9.0], [-1.0, 2.0, 0.5], [0.0, 0.0, 0.0]], F32)
    out["isolated"] = (np.concatenate([s.xyz[:600], iso, s.xyz[600:]], 0),
                       np.where(s.faces >= 600, s.faces + 3, s.faces).astype(np.int32))      # three vertices that no face names
    out["one_vertex"] = (np.array([[1.0, 2.0, 3.0]], F32), np.zeros((0, 3), np.int32))
    out["no_edges"] = (s.xyz[:50].copy(), np.array([[4, 4, 4], [7, 7, 7]], np.int32))         # only degenerate faces: E = 0
    if include_large:
        s = synthetic.make_room_scan(400, 375, 11, jitter=5e-4)                              # 150,000 vertices
        out["room_150k"] = (s.xyz, s.faces)
    return out


PARAM_SWEEP = [(k, m) for k in (0.001, 0.01, 0.1) for m in (1, 20, 200)]
