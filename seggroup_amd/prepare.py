"""Raw ScanNet scan -> the hot path's input files.

Host-side mirror of the parts of the reference's offline pre-processing that produce what `SegModel.forward` reads
(`seggroup/dataset/scannet/util.py`, driven by `prepare_data.py:36-71` and `prepare_weak_label.py`): same function
names, same files, same bytes -- the compute runs on the GPU through the C ABI (`sg_prep_sample_points`,
`sg_nearest_point`, `sg_mesh_adjacency`, `sg_segment_lists`), there is no CPU path.

    generate_pointcloud_pth          util.py:633-693   data/resampled/<s>/<s>.{pcl,info,map,unmap}.pth
    generate_seg_labels_and_ds_set   util.py:174-220   label/real/raw/<s>/<s>.seg.txt, label/real/resampled/<s>/<s>.seg.json
    generate_mesh_adjcency_pth       util.py:795-811   adj/mesh/{raw,resampled}/<s>/<s>.adj.pth
    get_unmapper / get_adj_from_mesh util.py:538-550 / 771-792

Paths are relative to `root` (the reference uses the working directory).  `plydata` may be a `plyfile.PlyData`
(not installed here) or the `PlyMesh` of `read_ply` below: only `['vertex'][name]`, `['face']['vertex_indices']`
and `.count` are used.  Ground-truth / weak-label generation (util.py:129-170, 268-427, 697-768) lives in labels.py and
needs ScanNet's annotation files.  The over-segmentation (`<scene>_vh_clean_2.0.010000.segs.json`) that these producers
start from is read from the scan directory; `prepare_scene(..., oversegment=True)` makes a missing one from the mesh
first (oversegment.py), and rekey.py carries a scan's annotation files over to such a segmentation.  Only annotating a scan -- making
the aggregation and click files in the first place -- stays out of scope.

    python -m seggroup_amd.prepare --data_root D [--scenes FILE] [--root OUT] [--num_points 150000]
           [--label_style manual|maxseg|mainseg|rand] [--manual_label_path P] [--main_num M] [--anno_num A]
           [--seg-graph scan|dense] [--seed N] [--oversegment] [--knn K | --radius R] [--index brute|grid] [--workers W]

runs `prepare_scene` over <D>/scans/<scene>: the reference's prepare_data.py and prepare_weak_label.py in one pass.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

import numpy as np

from . import hip, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace
# the annotation-derived label producers of the same reference file (util.py:76-170, 224-427, 697-768) live in labels.py
from .labels import (generate_real_label_pth, generate_real_labels, generate_seg_adjacency_matrix, generate_weak_label_pth,  # noqa: F401
                     generate_weak_labels, group_adjacency_segs, load_aggregation, load_labels, load_seg_labels, read_label_mapper, weak_style_dir)


# ---- minimal PLY (binary little endian; ScanNet's `_vh_clean_2.ply`) ---------------------------------------------
_PLY_TYPES = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4", "double": "<f8",
              "int8": "i1", "uint8": "u1", "int16": "<i2", "uint16": "<u2", "int32": "<i4", "uint32": "<u4", "float32": "<f4", "float64": "<f8"}


class _Element:
    def __init__(self, count, cols):
        self.count, self._cols = count, cols

    def __getitem__(self, name):
        return self._cols[name]


class PlyMesh:
    """`mesh['vertex']['x']`, `mesh['face']['vertex_indices']` ([F,3] int32), `.count` -- the subset of plyfile used."""

    def __init__(self, elements):
        self._e = elements

    def __getitem__(self, name):
        return self._e[name]


def read_ply(path: str) -> PlyMesh:
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] == "comment" or tok[0] == "obj_info":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elements[-1][2].append(tok[1:])
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: only binary_little_endian PLY is supported (ScanNet's format), got {fmt}")
        out = {}
        for name, count, props in elements:
            if any(p[0] == "list" for p in props):
                if len(props) != 1:
                    raise ValueError(f"{path}: element {name}: a list property next to other properties is not supported")
                _, ctype, itype, pname = props[0]
                rec = np.dtype([("n", _PLY_TYPES[ctype]), ("v", _PLY_TYPES[itype], (3,))])
                raw = np.frombuffer(f.read(rec.itemsize * count), dtype=rec, count=count)
                if count and not (raw["n"] == 3).all():
                    raise ValueError(f"{path}: element {name}: only triangle faces are supported")
                out[name] = _Element(count, {pname: np.ascontiguousarray(raw["v"]).astype(np.int32)})
            else:
                rec = np.dtype([(p[1], _PLY_TYPES[p[0]]) for p in props])
                raw = np.frombuffer(f.read(rec.itemsize * count), dtype=rec, count=count)
                out[name] = _Element(count, {p[1]: np.ascontiguousarray(raw[p[1]]) for p in props})
    return PlyMesh(out)


def write_ply(path: str, xyz, rgb, faces) -> None:
    """ScanNet-shaped binary PLY (vertex: float xyz + uchar rgba; face: uchar count + int ids) -- for tests and tools."""
    xyz, rgb, faces = np.asarray(xyz, np.float32), np.asarray(rgb, np.uint8), np.asarray(faces, np.int32)
    v = np.zeros(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
    v["x"], v["y"], v["z"], v["red"], v["green"], v["blue"], v["alpha"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb[:, 0], rgb[:, 1], rgb[:, 2], 255
    fc = np.zeros(faces.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    fc["n"], fc["v"] = 3, faces
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\n"
           "property list uchar int vertex_indices\nend_header\n" % (xyz.shape[0], faces.shape[0]))
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(v.tobytes())
        f.write(fc.tobytes())


def has_faces(plydata) -> bool:
    """False for a point cloud: a PLY without a face element, or with an empty one."""
    try:
        return plydata["face"].count > 0
    except KeyError:
        return False


def mesh_arrays(plydata):
    """-> xyz f32 [V,3], rgb u8 [V,3], faces i32 [F,3] from a PlyMesh / plyfile.PlyData.  A PLY without a face element, or with an
    empty one (a point cloud), gives faces of shape [0,3]."""
    vtx = plydata["vertex"]
    xyz = np.stack([np.asarray(vtx[k], dtype=np.float32) for k in ("x", "y", "z")], 1)
    rgb = np.stack([np.asarray(vtx[k], dtype=np.uint8) for k in ("red", "green", "blue")], 1)
    if not has_faces(plydata):
        return np.ascontiguousarray(xyz), np.ascontiguousarray(rgb), np.zeros((0, 3), np.int32)
    vi = plydata["face"]["vertex_indices"]
    faces = np.asarray(vi, dtype=np.int32) if isinstance(vi, np.ndarray) and vi.ndim == 2 else \
        np.stack([np.asarray(x, dtype=np.int32) for x in vi]) if len(vi) else np.zeros((0, 3), np.int32)
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("only triangle meshes are supported")
    return np.ascontiguousarray(xyz), np.ascontiguousarray(rgb), np.ascontiguousarray(faces)


# ---- device calls -----------------------------------------------------------------------------------------------
def _two_cloud_grid(name, entry, x, y, ks, dtype, cell, device, stream, want_d2):
    """One call of a two-cloud grid search `entry(x, xs, U, y, ys, N, *ks, cell, out, d2, ws, bytes, stream)`: the shape check, the
    workspace, the tensors (rows of `ks` entries, or one value a row) and the sync -> (out, d2 or None)."""
    import torch
    edge = hip.knn_cell(cell)
    dev = torch_device(device)
    lib = hip.lib()
    call = getattr(lib, entry)
    with torch.cuda.device(dev), on_stream(stream):
        dx, dy = device_tensor(x, torch.float32, dev), device_tensor(y, torch.float32, dev)
        if dx.dim() != 2 or dy.dim() != 2 or dx.shape[1] < 3 or dy.shape[1] < 3:
            raise ValueError(f"{name}: x and y must be [*, >= 3]")
        u, n = int(dx.shape[0]), int(dy.shape[0])
        sp = stream_ptr(stream)
        need = getattr(lib, entry + "_ws_bytes")(u, n, *ks)
        if need == 0:                                               # outside the envelope: the library says why, nothing is allocated
            hip.check(call(None, int(dx.shape[1]), u, None, int(dy.shape[1]), n, *ks, edge, None, None, None, 0, sp))
        out = torch.empty((u,) + ks, dtype=getattr(torch, dtype), device=dev)
        d2 = torch.empty((u,) + ks, dtype=torch.float32, device=dev) if want_d2 else None
        ws = workspace(need, dev)
        hip.check(call(dx.data_ptr(), int(dx.shape[1]), u, dy.data_ptr(), int(dy.shape[1]), n, *ks, edge, out.data_ptr(),
                       d2.data_ptr() if want_d2 else None, ws.data_ptr(), ws.numel(), sp))
        sync(stream)
    return out, d2


def nearest_grid_stats() -> dict:
    """What the calling thread's last grid-indexed nearest-point search did: cells per axis, occupied cells and the largest
    cell of the candidates' index, the cell edge used, the largest ring count of a query the rings settled, the queries finished against
    every candidate, and the pair scores evaluated (counted in timed calls only)."""
    return hip.grid_stats("nearest_point_grid", ("max_ring", "fallback", "scores"))


def nearest_point_grid(x, y, cell=None, device=None, stream=None, want_d2=True):
    """sg_nearest_point_grid: for every row of x [U, >= 3] the index of its best-scoring row of y [N, >= 3], exactly
    get_unmapper's, from the exact grid index -> (idx int64 [U], d2 float32 [U] or None), device tensors.  `cell` forces the cell edge
    (a performance knob: the result does not depend on it)."""
    return _two_cloud_grid("nearest_point_grid", "sg_nearest_point_grid", x, y, (), "int64", cell, device, stream, want_d2)


def knn_cross_stats() -> dict:
    """nearest_grid_stats for the calling thread's last knn_cross_grid: the same record."""
    return hip.grid_stats("cloud_knn_cross_grid", ("max_ring", "fallback", "scores"))


def knn_cross_grid(x, y, k, cell=None, device=None, stream=None, want_d2=False):
    """sg_cloud_knn_cross_grid: for every row of x [U, >= 3] its k best-scoring rows of y [N, >= 3], k in {5, 10, 20} --
    descending score, the lower index first among equal scores, so column 0 is nearest_point_grid's index -- from the exact grid index
    -> (knn int32 [U, k], d2 float32 [U, k] or None), device tensors.  `cell` forces the cell edge (a performance knob: the result does
    not depend on it)."""
    return _two_cloud_grid("knn_cross_grid", "sg_cloud_knn_cross_grid", x, y, (int(k),), "int32", cell, device, stream, want_d2)


def get_unmapper(x, y, device=None, index="brute", cell=None):
    """util.py:538-550: for every row of x [U,3] the index of its nearest row of y [N,3] (LongTensor on the device).
    `index="grid"`: the same indices from the exact grid index (`cell` forces its cell edge)."""
    import torch
    which, edge = hip.knn_index(index), hip.knn_cell(cell)
    if which == hip.KNN_GRID:
        return nearest_point_grid(x, y, cell=edge, device=device, want_d2=False)[0]
    dev = torch_device(device)
    lib = hip.lib()
    dx, dy = device_tensor(x, torch.float32, dev), device_tensor(y, torch.float32, dev)
    out = torch.empty(dx.shape[0], dtype=torch.int64, device=dev)
    ws = workspace(lib.sg_nearest_point_ws_bytes(dy.shape[0]), dev)
    with torch.cuda.device(dev):
        hip.check(lib.sg_nearest_point(dx.data_ptr(), dx.shape[0], dy.data_ptr(), dy.shape[1], dy.shape[0], out.data_ptr(), ws.data_ptr(),
                                       ws.numel(), None))
        sync(None)
    return out


def sample_points(xyz, rgb, mapper, device=None, index="brute"):
    """The compute of generate_pointcloud_pth: -> (pointcloud_sampled [Np,6] f32, unmapper [V] i64, #unsampled vertices).
    `index="grid"`: the unsampled vertices find their nearest sampled point through the exact grid index -- the same
    unmapper."""
    import torch
    which = hip.knn_index(index)
    dev = torch_device(device)
    lib = hip.lib()
    d_xyz, d_rgb, d_map = device_tensor(xyz, torch.float32, dev), device_tensor(rgb, torch.uint8, dev), device_tensor(mapper, torch.int64, dev)
    v, n = d_xyz.shape[0], d_map.shape[0]
    if which == hip.KNN_GRID:
        # the gather and the unmapper of the sampled vertices are index work (the last occurrence of a vertex in the mapper wins);
        # the search of the compacted `missing` list is the library's
        pcl = torch.cat([d_xyz[d_map], (d_rgb[d_map].to(torch.float64) / 127.5 - 1.0).to(torch.float32)], 1).contiguous()
        unmap = torch.full((v,), -1, dtype=torch.int64, device=dev)
        unmap.scatter_reduce_(0, d_map, torch.arange(n, dtype=torch.int64, device=dev), "amax", include_self=True)
        missing = torch.nonzero(unmap < 0).reshape(-1)
        if missing.numel():
            unmap[missing] = nearest_point_grid(d_xyz[missing].contiguous(), pcl, device=dev, want_d2=False)[0]
        return pcl, unmap, int(missing.numel())
    pcl = torch.empty((n, 6), dtype=torch.float32, device=dev)
    unmap = torch.empty(v, dtype=torch.int64, device=dev)
    ws = workspace(lib.sg_prep_sample_ws_bytes(v, n), dev)
    miss = C.c_int(0)
    with torch.cuda.device(dev):
        hip.check(lib.sg_prep_sample_points(d_xyz.data_ptr(), d_rgb.data_ptr(), v, d_map.data_ptr(), n, pcl.data_ptr(), unmap.data_ptr(),
                                            C.byref(miss), ws.data_ptr(), ws.numel(), None))
        sync(None)
    return pcl, unmap, miss.value


def mesh_adjacency(faces, unmapper=None, num_vertices: Optional[int] = None, device=None):
    """The compute of get_adj_from_mesh: -> (adj [E,2] i64, adj_resampled [E',2] i64 or None), device tensors."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    d_f = device_tensor(faces, torch.int32, dev)
    f = d_f.shape[0]
    d_un = device_tensor(unmapper, torch.int64, dev) if unmapper is not None else None
    v = int(num_vertices if num_vertices is not None else (d_un.shape[0] if d_un is not None else int(d_f.max().item()) + 1 if f else 1))
    raw = torch.empty((max(3 * f, 1), 2), dtype=torch.int64, device=dev)
    res = torch.empty((max(3 * f, 1), 2), dtype=torch.int64, device=dev) if d_un is not None else None
    ws = workspace(lib.sg_mesh_adjacency_ws_bytes(f), dev)
    n_raw, n_res = C.c_int(0), C.c_int(0)
    with torch.cuda.device(dev):
        hip.check(lib.sg_mesh_adjacency(d_f.data_ptr(), f, d_un.data_ptr() if d_un is not None else None, v, raw.data_ptr(), C.byref(n_raw),
                                        res.data_ptr() if res is not None else None, C.byref(n_res) if res is not None else None,
                                        ws.data_ptr(), ws.numel(), None))
        sync(None)
    return raw[:n_raw.value], (res[:n_res.value] if res is not None else None)


def segment_lists(seg_indices, mapper, device=None):
    """The compute of generate_seg_labels_and_ds_set: -> (raw_label [V] i32, seg_points [Np] i32, seg_off [G+1] i32) device
    tensors: groups in ascending compacted-id order, members ascending."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    d_seg, d_map = device_tensor(seg_indices, torch.int32, dev), device_tensor(mapper, torch.int64, dev)
    v, n = d_seg.shape[0], d_map.shape[0]
    raw = torch.empty(v, dtype=torch.int32, device=dev)
    pts = torch.empty(n, dtype=torch.int32, device=dev)
    off = torch.empty(min(v, n) + 1, dtype=torch.int32, device=dev)
    ws = workspace(lib.sg_segment_lists_ws_bytes(v, n), dev)
    counts = (C.c_int * 2)()
    with torch.cuda.device(dev):
        hip.check(lib.sg_segment_lists(d_seg.data_ptr(), v, d_map.data_ptr(), n, raw.data_ptr(), pts.data_ptr(), off.data_ptr(), counts,
                                       ws.data_ptr(), ws.numel(), None))
        sync(None)
    return raw, pts, off[:counts[1] + 1]


def get_adj_from_mesh(plydata, unmapper=None, device=None):
    """util.py:771-792 -> (adj, adj_resampled) LongTensors (CPU, like the reference's)."""
    _, _, faces = mesh_arrays(plydata)
    raw, res = mesh_adjacency(faces, unmapper, num_vertices=plydata["vertex"].count, device=device)
    return raw.cpu(), (res.cpu() if res is not None else None)


def get_adj_from_pointcloud(pointcloud, k=10, device=None):
    """util.py:814-834 (optional in the reference: nothing calls it): the kNN graph of the cloud as a per-row sorted, unique
    [*, 2] LongTensor (CPU, like the reference's).  Equal scores rank by ascending index (torch.topk leaves that open)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    pts = device_tensor(pointcloud, torch.float32, dev)
    n, stride = int(pts.shape[0]), int(pts.shape[1])
    out = torch.empty((n * int(k), 2), dtype=torch.int64, device=dev)
    ws = workspace(lib.sg_pointcloud_adjacency_ws_bytes(n, int(k)), dev)
    cnt = C.c_int(0)
    with torch.cuda.device(dev):
        hip.check(lib.sg_pointcloud_adjacency(pts.data_ptr(), stride, n, int(k), out.data_ptr(), C.byref(cnt), ws.data_ptr(), ws.numel(), None))
        sync(None)
    return out[:cnt.value].cpu()


def pointcloud_knn(pointcloud, k=10, device=None, index="brute", cell=None):
    """-> int32 [N, k+1] device tensor: the complete top-(k + 1) list of every point against the whole cloud, in the scores and the tie
    rule of get_adj_from_pointcloud (descending score, the lower index first); entry 0, normally the point itself, is kept.
    `index="grid"`: the same table from the exact grid index, up to 2^24 points; `cell` forces its cell edge (a
    performance knob: the table does not depend on it)."""
    import torch
    which, edge = hip.knn_index(index), hip.knn_cell(cell)
    dev = torch_device(device)
    lib = hip.lib()
    pts = device_tensor(pointcloud, torch.float32, dev)
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("pointcloud_knn: the cloud must be [N, >= 3]")
    n, stride = int(pts.shape[0]), int(pts.shape[1])
    if which == hip.KNN_GRID:
        if n > hip.MAX_GRID_POINTS:                                 # refused before anything is allocated
            hip.check(lib.sg_pointcloud_knn_grid(None, stride, n, int(k), edge, None, None, 0, None))
        out = torch.empty((n, int(k) + 1), dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_pointcloud_knn_grid_ws_bytes(n, int(k)), dev)
        with torch.cuda.device(dev):
            hip.check(lib.sg_pointcloud_knn_grid(pts.data_ptr(), stride, n, int(k), edge, out.data_ptr(), ws.data_ptr(), ws.numel(), None))
            sync(None)
        return out
    out = torch.empty((n, int(k) + 1), dtype=torch.int32, device=dev)
    ws = workspace(lib.sg_pointcloud_knn_ws_bytes(n), dev)
    with torch.cuda.device(dev):
        hip.check(lib.sg_pointcloud_knn(pts.data_ptr(), stride, n, int(k), out.data_ptr(), ws.data_ptr(), ws.numel(), None))
        sync(None)
    return out


def get_adj_from_radius(xyz, radius, device=None):
    """The radius graph of a cloud as the pairs a < b in lexicographic order -> [E, 2] LongTensor (CPU): the upper halves
    of the rows of `components.radius_neighbours`."""
    import torch
    from .components import radius_neighbours
    indptr, indices = radius_neighbours(xyz, radius, device=device)
    n = indptr.shape[0] - 1
    rows = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
    cols = indices.long()
    up = cols > rows
    return torch.stack([rows[up], cols[up]], dim=1).cpu()


def get_adj_from_cloud_scan(xyz, unmapper=None, k=10, device=None, radius=None):
    """A scan without faces: the point graph stands in for the mesh edges.  -> (adj, adj_resampled): get_adj_from_pointcloud(xyz, k), and
    those rows mapped through the unmapper, per-row sorted and unique, rows with i == j dropped like get_adj_from_mesh drops them.
    `radius`: the raw list is the radius graph's (`get_adj_from_radius`) instead."""
    import torch
    raw = get_adj_from_pointcloud(xyz, k, device=device) if radius is None else get_adj_from_radius(xyz, radius, device=device)
    if unmapper is None:
        return raw, None
    un = torch.as_tensor(unmapper, dtype=torch.long).cpu()
    raw_ne = raw[raw[:, 0] != raw[:, 1]]
    res = torch.sort(un[raw_ne], dim=1)[0]
    res = torch.unique(res, dim=0) if res.shape[0] else res.reshape(0, 2)
    return raw, res


# ---- the reference's file-producing functions -------------------------------------------------------------------------
def make_mapper(num_vertices: int, num_points: int, perm=None):
    """util.py:664-676.  `perm` replaces the `torch.randperm(V)` draw (pass one for reproducible output)."""
    import torch
    rep, rem = num_points // num_vertices, num_points % num_vertices
    if rem > 0:
        p = torch.as_tensor(np.asarray(perm), dtype=torch.long) if perm is not None else torch.randperm(num_vertices)
        index_remainder = p[:rem]
    else:
        index_remainder = torch.LongTensor([])
    if rep != 0:
        return torch.cat([torch.arange(num_vertices).repeat(rep), index_remainder], dim=0)
    return index_remainder


def generate_pointcloud_pth(scene_path, item, num_points, plydata=None, root: str = ".", perm=None, device=None, index: str = "brute"):
    """util.py:633-693: `.pcl.pth` f32 [num_points,6], `.info.pth`, `.map.pth`, `.unmap.pth` under data/resampled/<scene>/."""
    import torch
    scene_name = scans.scene_name(scene_path)
    if plydata is None:
        plydata = read_ply(os.path.join(scene_path, scene_name + "_vh_clean_2.ply"))
    xyz, rgb, _ = mesh_arrays(plydata)
    mapper = make_mapper(xyz.shape[0], num_points, perm)
    pcl, unmap, _ = sample_points(xyz, rgb, mapper, device=device, index=index)
    out = os.path.join(root, "data", "resampled", scene_name)
    os.makedirs(out, exist_ok=True)
    torch.save(pcl.cpu(), os.path.join(out, scene_name + ".pcl.pth"))
    torch.save(torch.LongTensor([item]), os.path.join(out, scene_name + ".info.pth"))
    torch.save(mapper, os.path.join(out, scene_name + ".map.pth"))
    torch.save(unmap.cpu(), os.path.join(out, scene_name + ".unmap.pth"))


def generate_seg_labels_and_ds_set(scene_path, root: str = ".", device=None):
    """util.py:174-220: label/real/raw/<s>/<s>.seg.txt and label/real/resampled/<s>/<s>.seg.json."""
    import torch
    scene_name = scans.scene_name(scene_path)
    seg = np.asarray(load_seg_labels(os.path.join(scene_path, scene_name + "_vh_clean_2.0.010000.segs.json")), dtype=np.int64)
    if seg.size and seg.min() < 0:
        raise ValueError("segIndices must be non-negative")
    mapper = torch.load(os.path.join(root, "data", "resampled", scene_name, scene_name + ".map.pth"))
    raw, pts, off = segment_lists(seg.astype(np.int32), mapper, device=device)
    lib = hip.lib()
    d1 = os.path.join(root, "label", "real", "raw", scene_name)
    os.makedirs(d1, exist_ok=True)
    h_raw = np.ascontiguousarray(raw.cpu().numpy())
    hip.check(lib.sg_write_label_txt(os.path.join(d1, scene_name + ".seg.txt").encode(), h_raw.ctypes.data, h_raw.shape[0]))
    d2 = os.path.join(root, "label", "real", "resampled", scene_name)
    os.makedirs(d2, exist_ok=True)
    h_pts, h_off = np.ascontiguousarray(pts.cpu().numpy()), np.ascontiguousarray(off.cpu().numpy())
    hip.check(lib.sg_write_seg_json(os.path.join(d2, scene_name + ".seg.json").encode(), h_pts.ctypes.data, h_off.ctypes.data,
                                    h_off.shape[0] - 1, h_pts.shape[0]))


def generate_mesh_adjcency_pth(scene_name, plydata=None, root: str = ".", scene_path: Optional[str] = None, device=None, knn: int = 10,
                               radius=None):
    """util.py:795-811: adj/mesh/raw/<s>/<s>.adj.pth and adj/mesh/resampled/<s>/<s>.adj.pth (skipped when both exist).  A scan without
    faces gets the kNN graph of its points (`knn` neighbours) under the same names, or with `radius` the radius graph."""
    import torch
    if radius is not None and int(knn) != 10:
        raise ValueError("generate_mesh_adjcency_pth: radius and knn = %d are two different graphs; give one" % int(knn))
    p1 = os.path.join(root, "adj", "mesh", "raw", scene_name, scene_name + ".adj.pth")
    p2 = os.path.join(root, "adj", "mesh", "resampled", scene_name, scene_name + ".adj.pth")
    if os.path.exists(p1) and os.path.exists(p2):
        return
    if plydata is None:
        if scene_path is None:
            raise ValueError("generate_mesh_adjcency_pth: pass plydata or scene_path")
        plydata = read_ply(os.path.join(scene_path, scene_name + "_vh_clean_2.ply"))
    unmapper = torch.load(os.path.join(root, "data", "resampled", scene_name, scene_name + ".unmap.pth"))
    if not has_faces(plydata):
        adj, adj_resampled = get_adj_from_cloud_scan(mesh_arrays(plydata)[0], unmapper, knn, device=device, radius=radius)
    elif radius is not None:
        raise ValueError(f"{scene_name}: the radius graph belongs to a scan without faces; this scan is a mesh and uses its faces")
    else:
        adj, adj_resampled = get_adj_from_mesh(plydata, unmapper, device=device)
    for p, t in ((p1, adj), (p2, adj_resampled)):
        os.makedirs(os.path.dirname(p), exist_ok=True)
        torch.save(t, p)


def prepare_scene(scene_path, item, num_points: int = 150000, root: str = ".", perm=None, device=None, label_style: Optional[str] = None,
                  manual_label_path: Optional[str] = None, oversegment: bool = False, knn: int = 10, index: str = "brute", radius=None,
                  main_num: int = -1, anno_num: int = 1, seg_graph="dense", rng=None):
    """What prepare_data.py:36-71 + prepare_weak_label.py:60-90 do for one scan: point cloud, mapper / unmapper, segment lists,
    mesh adjacency and -- with `label_style` and ScanNet's annotation files next to the mesh -- the ground-truth and weak-label
    files, i.e. every input of SegModel.forward.  `oversegment=True`: a scan without a segs.json gets one from its mesh first
    (oversegment.py, default parameters); an existing file is never overwritten.  A scan without faces (a point cloud) is segmented
    over the kNN graph of its points (`knn` neighbours), and that graph stands in for the mesh adjacency.  `index="grid"`: the
    unsampled vertices' nearest sampled point comes from the exact grid index; the files are the same.  `radius` (a scan
    without faces): the over-segmentation and the adjacency files come from the radius graph instead of the kNN graph.
    `main_num`, `anno_num`, `seg_graph` and `rng` go to `generate_weak_labels`.  -> what it returned (labeled vertices,
    vertices, clicked segments, segments, instances), or None without `label_style`."""
    hip.knn_index(index)
    if radius is not None and int(knn) != 10:
        raise ValueError("prepare_scene: radius and knn = %d are two different graphs; give one" % int(knn))
    scene_name = scans.scene_name(scene_path)
    ply = read_ply(os.path.join(scene_path, scene_name + "_vh_clean_2.ply"))
    if radius is not None and has_faces(ply):
        raise ValueError(f"{scene_name}: the radius graph belongs to a scan without faces; this scan is a mesh and uses its faces")
    if oversegment:
        from .oversegment import oversegment_scan
        oversegment_scan(scene_path, device=device, plydata=ply, knn=knn, radius=radius)
    elif not has_faces(ply) and not os.path.exists(os.path.join(scene_path, scene_name + "_vh_clean_2.0.010000.segs.json")):
        raise ValueError(f"{scene_name}: a scan without faces and without a segs.json: pass oversegment=True to make one from the points")
    generate_pointcloud_pth(scene_path, item, num_points, ply, root=root, perm=perm, device=device, index=index)
    generate_seg_labels_and_ds_set(scene_path, root=root, device=device)
    generate_mesh_adjcency_pth(scene_name, ply, root=root, device=device, knn=knn, radius=radius)
    if label_style is None:
        return None
    generate_real_labels(scene_path, root=root)
    generate_real_label_pth(scene_path, root=root)
    ret = generate_weak_labels(scene_path, ply, label_style=label_style, manual_label_path=manual_label_path, main_num=main_num,
                               anno_num=anno_num, root=root, seg_graph=seg_graph, rng=rng, device=device)
    generate_weak_label_pth(scene_name, weak_style_dir(label_style, main_num, anno_num), root=root)
    return ret


# ---- the dataset-level command: the reference's prepare_data.py and prepare_weak_label.py over a tree of scans -----------------------
REPORT_NAME = "prepare_report.json"
LABEL_STYLES = ("manual", "maxseg", "mainseg", "rand")


def scene_rng(seed: int, scene: str):
    """the RandomState a scene's mapper permutation and clicks are drawn from: a function of the seed and the scene's name alone, so the
    tree depends neither on --workers nor on the order of the scenes"""
    import zlib
    return np.random.RandomState(zlib.crc32(("%d/%s" % (int(seed), scene)).encode()))


def summary_lines(rets, scenes: int):
    """prepare_weak_label.py:116-132 over the per-scene return values; the two per-scene averages are over `scenes`"""
    lp, ap_, ls, as_, ins = (sum(int(r[i]) for r in rets) for i in range(5))
    return ["Average labeled points of weak label in all points: %.2f%%" % (lp / ap_ * 100),
            "Average labeled segments of weak label in all segments: %.2f%%" % (ls / as_ * 100),
            "Average real labeled points in all points: %.4f%%" % (ls / ap_ * 100),
            "Average instance number per scene: %.2f" % (ins / scenes),
            "Average labeled segment number per scene: %.2f" % (ls / scenes)]


def prepare_scans(data_root: str, scenes=None, root: str = ".", num_points: int = 150000, label_style: Optional[str] = None,
                  manual_label_path: Optional[str] = None, main_num: int = -1, anno_num: int = 1, seg_graph: str = "scan", seed: int = 0,
                  oversegment: bool = False, knn: int = 10, radius=None, index: str = "brute", workers: int = 4, device=None):
    """`prepare_scene` over <data_root>/scans/<scene> for every named scene (default: every scan directory) on threads ->
    [(scene, return value of generate_weak_labels or None)] in the scenes' order; writes <root>/prepare_report.json.  `item` is a
    scene's position in the list; its permutation and its clicks come from `scene_rng(seed, scene)`."""
    dev = torch_device(device)
    scans_dir = os.path.join(data_root, "scans")
    if scenes is None:
        scenes = scans.scan_names(scans_dir)
    item_of = {scene: i for i, scene in enumerate(scenes)}

    def say(line):                                                   # one write per line: the threads' lines do not interleave
        sys.stdout.write(line + "\n")
        sys.stdout.flush()

    def one(scene, stream):
        item = item_of[scene]
        say("[%04d/%d] Dealing with %s..." % (item, len(scenes), scene))
        rng = scene_rng(seed, scene)
        scene_path = os.path.join(scans_dir, scene)
        perm = rng.permutation(scans.declared_count(os.path.join(scene_path, scene + scans.PLY_SUFFIX), b"vertex"))
        ret = prepare_scene(scene_path, item, num_points, root=root, perm=perm, device=dev, label_style=label_style,
                            manual_label_path=manual_label_path, oversegment=oversegment, knn=knn, index=index, radius=radius,
                            main_num=main_num, anno_num=anno_num, seg_graph=seg_graph, rng=rng)
        say("[%04d/%d] Finish %s!" % (item, len(scenes), scene))
        return ret

    done = scans.map_scans(list(scenes), workers, dev, one)
    os.makedirs(root, exist_ok=True)
    doc = {"num_points": int(num_points), "label_style": label_style, "main_num": int(main_num), "anno_num": int(anno_num),
           "seg_graph": seg_graph if label_style not in (None, "manual") else None, "seed": int(seed),
           "scenes": {scene: (None if ret is None else dict(zip(("labeled_points", "points", "labeled_segments", "segments", "instances"),
                                                               (int(x) for x in ret)))) for scene, ret in done}}
    scans.write_report(os.path.join(root, REPORT_NAME), doc)
    return done


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.prepare",
                                 description="Every input of SegModel.forward for a tree of ScanNet scans: what the reference's "
                                             "prepare_data.py and prepare_weak_label.py write, in one pass.")
    ap.add_argument("--data_root", required=True, help="the dataset's root: scans are <data_root>/scans/<scene>")
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line (default: every scan directory)")
    ap.add_argument("--root", default=".", help="where data/, label/ and adj/ go (default: CWD)")
    ap.add_argument("--num_points", type=int, default=150000, help="points to sample per scan")
    ap.add_argument("--label_style", default=None, choices=LABEL_STYLES, help="also write ground truth and weak labels of this style")
    ap.add_argument("--manual_label_path", default=None, help="directory of manual click files (only for manual)")
    ap.add_argument("--main_num", type=int, default=-1, help="main segments to consider (only for mainseg)")
    ap.add_argument("--anno_num", type=int, default=1, help="annotations per instance (only for maxseg and mainseg)")
    ap.add_argument("--seg-graph", dest="seg_graph", default="scan", choices=("scan", "dense"),
                    help="simulated clicks: the scan's own graph contracted on the GPU, or the reference's dense matrix over the faces")
    ap.add_argument("--seed", type=int, default=0, help="every scene draws from RandomState(crc32('<seed>/<scene>'))")
    ap.add_argument("--oversegment", action="store_true", help="make a missing segs.json from the scan first")
    graph = ap.add_mutually_exclusive_group()
    graph.add_argument("--knn", type=int, default=None, help="a scan without faces: neighbours of its point graph (default 10)")
    graph.add_argument("--radius", type=float, default=None, help="a scan without faces: the radius graph instead of the kNN graph")
    ap.add_argument("--index", default="brute", choices=tuple(hip.KNN_INDEX), help="nearest sampled point: brute force or the grid index")
    scans.add_workers_argument(ap)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    if a.label_style == "manual" and a.manual_label_path is None:
        ap.error("--label_style manual needs --manual_label_path")
    if a.label_style == "mainseg" and (a.main_num < 1 or a.anno_num > a.main_num):
        ap.error("--label_style mainseg needs --main_num >= 1 and --anno_num <= --main_num")
    if a.num_points < 1 or a.anno_num < 1:
        ap.error("--num_points and --anno_num must be at least 1")
    scans.check_workers(ap, a.workers)
    done = prepare_scans(a.data_root, scans.scene_list(a.scenes), a.root, a.num_points, a.label_style, a.manual_label_path, a.main_num,
                         a.anno_num, a.seg_graph, a.seed, a.oversegment, 10 if a.knn is None else a.knn, a.radius, a.index, a.workers,
                         a.device)
    if a.label_style is not None and done:
        print()
        for line in summary_lines([ret for _, ret in done], len(done)):
            print(line)
    print("\nFinish all!\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
