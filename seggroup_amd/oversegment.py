"""Over-segmentation: a scan's `_vh_clean_2.ply` -> `<scene>_vh_clean_2.<kThresh>.segs.json` (DESIGN.md 8d for a mesh, 8f for a cloud).

The over-segmentation is the one input of `prepare.py` / `labels.py` that used to come from outside (ScanNet ships it, made by its
Segmentator tool).  This is a graph-based segmenter of the same family -- Felzenszwalb-Huttenlocher merging over the mesh edges,
weighted by the difference of the vertex normals, with `kThresh` and `segMinVerts` -- so a mesh that is not a ScanNet download can go
through the whole project.  The contract is the specification in DESIGN.md 8d (the tie order is defined, the result is deterministic);
it is NOT byte equality with the files ScanNet ships.

Normals, edges, weights and the sort run on the GPU (`sg_overseg_edges`), the order-dependent merge chain on the host
(`sg_overseg_merge`, usable without a GPU); there is no other path.

A PLY without faces (a laser scan, a fused depth cloud) takes the point-cloud path on its own: the graph is the kNN graph of the cloud,
the normals come from the covariance of every point's k + 1 nearest points (`sg_pcseg_edges`), the order of the edges and the chain are
the mesh path's.  `--pointcloud` sends a mesh down that path too; its faces are ignored.

A cloud above 2^20 points is thinned on a voxel grid first (`voxel=H` / `--voxel H`): the segmenter sees one point per
occupied voxel, and every point takes the id of its voxel's representative.

`index="grid"` / `--index grid` takes the point-cloud path's neighbour lists from the exact grid index instead of scoring
every pair: the same lists bit for bit, hence the same segs.json, in a fraction of the time and up to 2^24 points.  With `--voxel` the
cloud is thinned first and the grid works on the representatives.

    python -m seggroup_amd.oversegment --scans DIR [--scenes LIST] [--k-thresh 0.01] [--seg-min-verts 20] [--force] [--workers 4]
                                       [--pointcloud] [--knn {5,10,20}] [--viewpoint X Y Z] [--voxel H] [--index {brute,grid}] [--radius R]

`radius=R` / `--radius R` (a scan without faces, or `--pointcloud`; instead of `--knn` and `--index`): the graph is the radius graph of
the points, every pair at most R apart, and the normals are taken over those neighbourhoods -- for clouds that hold more than
k points inside the neighbourhood scale, where the kNN graph has no edge out of a clump.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
from typing import Optional

import numpy as np

from . import hip, scans
from .components import radius_neighbours, radius_pairs
from .device import device_cloud, device_tensor, on_stream, stream_ptr, sync, torch_device, workspace
from .prepare import mesh_arrays, pointcloud_knn, read_ply
from .scans import segs_json_name  # noqa: F401  (the name is made here; every reader of a scan tree finds it in scans.py)
from .thin import thin_cloud


def _mesh_tensors(xyz, faces, dev):
    import torch
    d_xyz, d_f = device_tensor(xyz, torch.float32, dev), device_tensor(faces, torch.int32, dev)
    if d_xyz.dim() != 2 or d_xyz.shape[1] != 3 or d_f.dim() != 2 or d_f.shape[1] != 3:
        raise ValueError("oversegment: xyz must be [V,3] and faces [F,3]")
    if d_xyz.shape[0] < 1:
        raise ValueError("oversegment: a mesh needs at least one vertex")
    return d_xyz, d_f, int(d_xyz.shape[0]), int(d_f.shape[0])


def device_edges(xyz, faces, device=None, stream=None, want_face_normals: bool = False):
    """The device stages of one mesh -> dict(face_normals [F,3] | None, normals [V,3], edges [E,2] i32, w [E]) of device tensors:
    the unique undirected edges in ascending (w, a, b)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, d_f, v, f = _mesh_tensors(xyz, faces, dev)
        fn = torch.empty((f, 3), dtype=torch.float32, device=dev) if want_face_normals else None
        nrm = torch.empty((v, 3), dtype=torch.float32, device=dev)
        edges = torch.empty((max(3 * f, 1), 2), dtype=torch.int32, device=dev)
        w = torch.empty(max(3 * f, 1), dtype=torch.float32, device=dev)
        ws = workspace(lib.sg_overseg_ws_bytes(v, f), dev)
        n_e = C.c_int(0)
        hip.check(lib.sg_overseg_edges(d_xyz.data_ptr(), v, d_f.data_ptr() if f else None, f, fn.data_ptr() if fn is not None and f else None,
                                       nrm.data_ptr(), edges.data_ptr(), w.data_ptr(), C.byref(n_e), ws.data_ptr(), ws.numel(),
                                       stream_ptr(stream)))
        sync(stream)
    return dict(face_normals=fn, normals=nrm, edges=edges[:n_e.value], w=w[:n_e.value])


def vertex_normals(xyz, faces, device=None):
    """-> [V,3] f32 device tensor: the face normals summed per vertex in ascending face index, normalised."""
    return device_edges(xyz, faces, device=device)["normals"]


def edge_weights(xyz, faces, device=None):
    """-> (edges [E,2] i32, w [E] f32) device tensors in ascending (w, a, b)."""
    r = device_edges(xyz, faces, device=device)
    return r["edges"], r["w"]


def merge_edges(edges, w, num_vertices: int, k_thresh: float = 0.01, seg_min_verts: int = 20) -> np.ndarray:
    """The host chain over edges sorted by ascending (w, a, b) -> int32 [V].  Needs no GPU."""
    e = np.ascontiguousarray(np.asarray(edges), dtype=np.int32).reshape(-1, 2)
    ww = np.ascontiguousarray(np.asarray(w), dtype=np.float32).reshape(-1)
    if ww.shape[0] != e.shape[0]:
        raise ValueError("merge_edges: one weight per edge")
    out = np.empty(max(int(num_vertices), 0), dtype=np.int32)
    hip.check(hip.lib().sg_overseg_merge(e.ctypes.data if e.size else None, ww.ctypes.data if ww.size else None, e.shape[0], int(num_vertices),
                                         float(k_thresh), int(seg_min_verts), out.ctypes.data if out.size else None))
    return out


def segment_mesh(xyz, faces, k_thresh: float = 0.01, seg_min_verts: int = 20, device=None, stream=None) -> np.ndarray:
    """-> int32 [V]: seg_indices[v] = the lowest vertex index of v's segment (non-contiguous ids, like ScanNet's)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, d_f, v, f = _mesh_tensors(xyz, faces, dev)
        out = np.empty(v, dtype=np.int32)
        ws = workspace(lib.sg_overseg_ws_bytes(v, f), dev)
        hip.check(lib.sg_overseg_scan(d_xyz.data_ptr(), v, d_f.data_ptr() if f else None, f, float(k_thresh), int(seg_min_verts),
                                      out.ctypes.data if v else None, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
    return out


def _cloud_tensor(xyz, dev):
    return device_cloud(xyz, dev, "oversegment", exact=True)


def _viewpoint(viewpoint):
    """-> (ctypes float[3] or None); the host array the library reads"""
    if viewpoint is None:
        return None
    v = np.asarray(viewpoint, dtype=np.float32).reshape(-1)
    if v.shape[0] != 3:
        raise ValueError("oversegment: the viewpoint is three coordinates")
    return (C.c_float * 3)(*v.tolist())


def knn_grid_stats() -> dict:
    """What the calling thread's last grid-indexed kNN did: cells per axis, occupied cells, the largest cell, the cell edge
    used, the largest ring count of a query the rings settled, the queries finished against the whole cloud, and the pair scores
    evaluated (counted in timed calls only)."""
    return hip.grid_stats("pointcloud_knn_grid", ("max_ring", "fallback", "scores"))


def _radius_only(who, radius, k=10, index="brute", knn=None):
    """`radius` selects the radius graph in place of the kNN graph: it goes with neither a neighbour count, nor a kNN index,
    nor a caller's kNN table.  -> the radius as a float, or None"""
    if radius is None:
        return None
    if int(k) != 10:
        raise ValueError(f"{who}: radius and k = {int(k)} are two different graphs; give one")
    if index != "brute":
        raise ValueError(f"{who}: radius and index = {index!r} are two different graphs (the radius graph has its own grid); give one")
    if knn is not None:
        raise ValueError(f"{who}: radius and a kNN table are two different graphs; give one")
    import math
    r = float(radius)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"{who}: radius must be a finite length > 0, not {radius!r}")
    return r


def _graph_source(what, d_xyz, n, k, which, edge, r, dev, stream):
    """The three graphs a cloud is segmented over -- brute-force kNN, grid kNN, radius -- stated once for sg_pcseg_edges* and
    sg_pcseg_scan* (`what`: "edges" or "scan").  Every entry point reads (xyz, n, *head, viewpoint, *mid, its outputs, *tail, ws,
    ws_bytes, stream).  -> (the entry point, head, mid, tail, workspace bytes, T: the radius graph's pair count, 0 for kNN).  A cloud
    outside the grid's envelope is refused here, in the library's words, before anything is allocated."""
    lib = hip.lib()
    if r is not None:
        t = radius_pairs(d_xyz, n, r, edge, dev, stream)[0]
        return getattr(lib, f"sg_pcseg_{what}_radius"), (r, edge, t), (), (C.byref(C.c_int64(0)),), lib.sg_pcseg_ws_bytes_radius(n, t), t
    if which == hip.KNN_GRID:
        need = lib.sg_pcseg_ws_bytes_indexed(n, k, which) if n <= hip.MAX_GRID_POINTS else 0
        if need == 0:
            hip.check(lib.sg_pointcloud_knn_grid(None, 3, n, k, edge, None, None, 0, None))
        return getattr(lib, f"sg_pcseg_{what}_indexed"), (k,), (which, edge), (), need, 0
    return getattr(lib, f"sg_pcseg_{what}"), (k,), (), (), lib.sg_pcseg_ws_bytes(n, k), 0


def pointcloud_edges(xyz, k: int = 10, viewpoint=None, device=None, stream=None, index: str = "brute", cell=None, radius=None):
    """The device stages of one cloud -> dict(knn [N,k+1] i32, normals [N,3], edges [E,2] i32, w [E]) of device tensors:
    every point's k + 1 best-scoring points, the covariance normals turned towards the viewpoint (default: the centre of the bounding
    box), and the unique undirected kNN pairs a < b in ascending (w, a, b).  `index="grid"`: the lists come from the exact grid index
    (`cell` forces its cell edge) -- the same bytes, up to 2^24 points.

    `radius=R` (instead of `k` and `index`): the radius graph -> dict(indptr int64 [N+1], indices int32 [T], normals,
    edges, w): every point's neighbours within R in ascending index, the normals over those neighbourhoods, the pairs a < b of the
    graph in ascending (w, a, b).  `cell` forces the grid's cell edge and cannot change a byte."""
    import torch
    r = _radius_only("pointcloud_edges", radius, k, index)
    which, edge = hip.knn_index(index), hip.knn_cell(cell)
    dev = torch_device(device)
    k = int(k)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, n = _cloud_tensor(xyz, dev)
        call, head, mid, tail, need, t = _graph_source("edges", d_xyz, n, k, which, edge, r, dev, stream)
        if r is not None:                                           # the rows of the graph: CSR lists, or the kNN table
            rows = dict(indptr=torch.empty(n + 1, dtype=torch.int64, device=dev), indices=torch.empty(max(t, 1), dtype=torch.int32, device=dev))
            cap = max(t // 2, 1)
        else:
            rows = dict(knn=torch.empty((n, k + 1), dtype=torch.int32, device=dev))
            cap = max(n * k, 1)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
        edges = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        w = torch.empty(cap, dtype=torch.float32, device=dev)
        n_e = C.c_int(0)
        ws = workspace(need, dev)
        hip.check(call(d_xyz.data_ptr(), n, *head, _viewpoint(viewpoint), *mid, *[x.data_ptr() for x in rows.values()], nrm.data_ptr(),
                       edges.data_ptr(), w.data_ptr(), C.byref(n_e), *tail, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    if r is not None:
        rows["indices"] = rows["indices"][:t]
    return dict(rows, normals=nrm, edges=edges[:n_e.value], w=w[:n_e.value])


def pointcloud_normals(xyz, k: int = 10, viewpoint=None, knn=None, device=None, radius=None, lists=None):
    """-> [N,3] f32 device tensor: per point the eigenvector of the smallest eigenvalue of its k + 1 nearest points' covariance, not
    re-normalised, turned towards the viewpoint.  `knn`: a table of `prepare.pointcloud_knn` (made when not given).

    `radius=R` (instead of `k` and `knn`): the neighbourhood of a point is the point and every other point within R.
    `lists=(indptr, indices)`: a caller's rows in place of `components.radius_neighbours(xyz, R)`; they are checked on the device."""
    import torch
    r = _radius_only("pointcloud_normals", radius, k, "brute", knn)
    if lists is not None and r is None:
        raise ValueError("pointcloud_normals: lists belong to the radius form")
    dev = torch_device(device)
    lib = hip.lib()
    k = int(k)
    with torch.cuda.device(dev):
        d_xyz, n = _cloud_tensor(xyz, dev)
        if r is not None:
            if lists is None:
                lists = radius_neighbours(d_xyz, r, device=dev)
            indptr, indices = device_tensor(lists[0], torch.int64, dev), device_tensor(lists[1], torch.int32, dev)
            if indptr.dim() != 1 or indptr.shape[0] != n + 1 or indices.dim() != 1:
                raise ValueError("pointcloud_normals: lists are (indptr [N + 1], indices [T])")
            if int(indptr[-1]) != indices.shape[0]:
                raise ValueError("pointcloud_normals: indptr[N] = %d, and indices holds %d entries" % (int(indptr[-1]), indices.shape[0]))
            nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
            ws = workspace(lib.sg_pointcloud_knn_ws_bytes(n), dev)
            hip.check(lib.sg_pointcloud_normals_csr(d_xyz.data_ptr(), n, indptr.data_ptr(), indices.data_ptr() if indices.numel() else None,
                                                    _viewpoint(viewpoint), nrm.data_ptr(), ws.data_ptr(), ws.numel(), None))
            sync(None)
            return nrm
        table = pointcloud_knn(d_xyz, k, device=dev) if knn is None else device_tensor(knn, torch.int32, dev)
        if table.dim() != 2 or tuple(table.shape) != (n, k + 1):
            raise ValueError("pointcloud_normals: knn must be [N, k+1]")
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ws = workspace(lib.sg_pointcloud_knn_ws_bytes(n), dev)
        hip.check(lib.sg_pointcloud_normals(d_xyz.data_ptr(), n, table.data_ptr(), k, _viewpoint(viewpoint), nrm.data_ptr(), ws.data_ptr(),
                                            ws.numel(), None))
        sync(None)
    return nrm


def segment_pointcloud(xyz, k: int = 10, k_thresh: float = 0.01, seg_min_verts: int = 20, viewpoint=None, device=None,
                       stream=None, voxel: Optional[float] = None, index: str = "brute", cell=None, radius=None) -> np.ndarray:
    """-> int32 [N]: seg_indices[i] = the lowest point index of i's segment, for a cloud without faces.

    `voxel`: thin the cloud on a grid of that edge first and segment the representatives with the same parameters -- the
    segmenter sees only the thinned cloud (its default viewpoint is that cloud's box centre, `seg_min_verts` counts thinned points) --;
    every point then takes its representative's id, as a raw index: rep[seg_thin[thin_of_point]], the segment's lowest representative.
    That is how a cloud above 2^20 points is segmented; a grid that leaves every point alone gives the un-thinned ids.

    `index="grid"`: the neighbour lists come from the exact grid index (`cell` forces its cell edge): the same ids, and a
    cloud of up to 2^24 points is segmented at full resolution.  With `voxel` the grid works on the representatives.

    `radius=R` (instead of `k` and `index`): the graph is the radius graph -- every pair of points at most R apart, the
    normals over those neighbourhoods.  That is the graph for a cloud with more than k points inside the neighbourhood scale (near the
    scanner, overlapping sweeps, an unthinned cloud), where the kNN graph has no edge out of a clump.  `voxel` combines as with kNN."""
    import torch
    r = _radius_only("segment_pointcloud", radius, k, index)
    which, edge = hip.knn_index(index), hip.knn_cell(cell)
    dev = torch_device(device)
    k = int(k)
    if voxel is not None:
        with torch.cuda.device(dev), on_stream(stream):
            d_all = _cloud_tensor(xyz, dev)[0]
        rep, top, _ = thin_cloud(d_all, voxel, device=dev, stream=stream)
        with torch.cuda.device(dev), on_stream(stream):
            d_thin = d_all.index_select(0, rep.long())
        seg_thin = segment_pointcloud(d_thin, k, k_thresh, seg_min_verts, viewpoint=viewpoint, device=dev, stream=stream, index=index, cell=cell,
                                      radius=radius)
        rep_h = rep.cpu().numpy()
        return np.ascontiguousarray(rep_h[seg_thin[top.cpu().numpy()]], dtype=np.int32)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, n = _cloud_tensor(xyz, dev)
        out = np.empty(n, dtype=np.int32)
        call, head, mid, tail, need, _ = _graph_source("scan", d_xyz, n, k, which, edge, r, dev, stream)
        ws = workspace(need, dev)
        hip.check(call(d_xyz.data_ptr(), n, *head, _viewpoint(viewpoint), *mid, float(k_thresh), int(seg_min_verts), out.ctypes.data, *tail,
                       ws.data_ptr(), ws.numel(), stream_ptr(stream)))
    return out


def write_segs_json(path: str, seg_indices, scene_id: str, k_thresh: float = 0.01, seg_min_verts: int = 20) -> None:
    seg = np.ascontiguousarray(np.asarray(seg_indices), dtype=np.int32).reshape(-1)
    hip.check(hip.lib().sg_write_segs_json(os.fspath(path).encode(), scene_id.encode(), seg.ctypes.data if seg.size else None, seg.shape[0],
                                           float(k_thresh), int(seg_min_verts)))


def oversegment_scan(scene_path: str, k_thresh: float = 0.01, seg_min_verts: int = 20, force: bool = False, device=None, stream=None,
                     plydata=None, pointcloud: bool = False, knn: int = 10, viewpoint=None, voxel: Optional[float] = None,
                     index: str = "brute", radius=None) -> Optional[str]:
    """Writes the scan's segs.json next to its mesh; -> the path, or None when the file was there already (never overwritten without
    `force`).  A scan without faces is segmented as a point cloud (`knn` neighbours, normals towards `viewpoint`); `pointcloud=True`
    does the same to a mesh, ignoring its faces.  `voxel`: the point-cloud path thins on that grid first (`segment_pointcloud`); on the
    mesh path it is an error, not ignored.  `index`: "brute" or "grid", the point-cloud path's neighbour search; on
    the mesh path "grid" is an error as well.  `radius`: the point-cloud path's graph is the radius graph instead of the
    kNN graph; not with a non-default `knn` or `index`, and on the mesh path an error."""
    hip.knn_index(index)
    _radius_only("oversegment_scan", radius, knn, index)
    name = scans.scene_name(scene_path)
    out = os.path.join(scene_path, segs_json_name(name, k_thresh))
    if os.path.exists(out) and not force:
        return None
    if plydata is None:
        plydata = read_ply(os.path.join(scene_path, name + "_vh_clean_2.ply"))
    xyz, _, faces = mesh_arrays(plydata)
    if pointcloud or faces.shape[0] == 0:
        seg = segment_pointcloud(xyz, knn, k_thresh, seg_min_verts, viewpoint=viewpoint, device=device, stream=stream, voxel=voxel, index=index,
                                 radius=radius)
    elif radius is not None:
        raise ValueError(f"{name}: the radius graph belongs to the point-cloud path; this scan is a mesh (pass pointcloud=True to ignore its faces)")
    elif voxel is not None:
        raise ValueError(f"{name}: voxel thinning belongs to the point-cloud path; this scan is a mesh (pass pointcloud=True to ignore its faces)")
    elif index != "brute":
        raise ValueError(f"{name}: the grid index belongs to the point-cloud path; this scan is a mesh (pass pointcloud=True to ignore its faces)")
    else:
        seg = segment_mesh(xyz, faces, k_thresh, seg_min_verts, device=device, stream=stream)
    write_segs_json(out, seg, name, k_thresh, seg_min_verts)
    return out


def oversegment_scans(scans_dir: str, scenes=None, k_thresh: float = 0.01, seg_min_verts: int = 20, force: bool = False, workers: int = 4,
                      device=None, pointcloud: bool = False, knn: int = 10, viewpoint=None, voxel: Optional[float] = None, index: str = "brute",
                      radius=None):
    """Every scan directory under `scans_dir` (or the named ones) -> (written paths, skipped scene names).  Workers are threads, each
    with its own stream and workspace: the host chain of one scan overlaps the device work of the next."""
    hip.knn_index(index)
    _radius_only("oversegment_scans", radius, knn, index)
    dev = torch_device(device)
    if scenes is None:
        scenes = scans.scan_names(scans_dir)
    done = scans.map_scans(scenes, workers, dev, lambda scene, stream: oversegment_scan(
        os.path.join(scans_dir, scene), k_thresh, seg_min_verts, force, device=dev, stream=stream, pointcloud=pointcloud, knn=knn,
        viewpoint=viewpoint, voxel=voxel, index=index, radius=radius))
    return [path for _, path in done if path is not None], [scene for scene, path in done if path is None]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.oversegment", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line (default: every scan with a mesh)")
    ap.add_argument("--k-thresh", type=float, default=0.01)
    ap.add_argument("--seg-min-verts", type=int, default=20)
    ap.add_argument("--force", action="store_true", help="overwrite existing segs.json files")
    scans.add_workers_argument(ap)
    ap.add_argument("--device", default=None)
    ap.add_argument("--pointcloud", action="store_true", help="segment every scan as a point cloud (a scan without faces always is); faces are ignored")
    ap.add_argument("--knn", type=int, default=10, choices=(5, 10, 20), help="neighbours per point of the point-cloud path")
    ap.add_argument("--viewpoint", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="the point-cloud path turns its normals towards this point (default: the centre of the bounding box)")
    ap.add_argument("--voxel", type=float, default=None, metavar="H",
                    help="the point-cloud path thins the cloud on a voxel grid of this edge first (needed above 2^20 points)")
    ap.add_argument("--index", default="brute", choices=("brute", "grid"),
                    help="neighbour search of the point-cloud path: every pair, or the exact grid index (the same lists; up to 2^24 points)")
    ap.add_argument("--radius", type=float, default=None, metavar="R",
                    help="the point-cloud path segments over the radius graph (every pair of points at most R apart) instead of the kNN graph")
    a = ap.parse_args(argv)
    given = [t.split("=")[0] for t in (sys.argv[1:] if argv is None else argv)]
    if a.radius is not None:
        import math
        if not (a.radius > 0.0 and math.isfinite(a.radius)):
            ap.error("--radius must be a finite length > 0")
        if any(t in ("--kn", "--knn") for t in given):                      # given explicitly, the default value included
            ap.error("--radius and --knn are two different graphs: give one")
        if any(len(t) > 2 and "--index".startswith(t) for t in given):
            ap.error("--radius and --index are two different graphs (the radius graph has its own grid): give one")
    scenes = scans.scene_list(a.scenes)
    if (a.voxel is not None or a.index != "brute" or a.radius is not None) and not a.pointcloud:
        names = scenes if scenes is not None else scans.scan_names(a.scans)
        meshes = [s for s in names if scans.declared_faces(os.path.join(a.scans, s, s + "_vh_clean_2.ply")) > 0]
        if meshes and a.voxel is not None:
            ap.error("--voxel thins point clouds, and %s %s faces: add --pointcloud to ignore them" % (", ".join(meshes[:5]),
                                                                                                       "has" if len(meshes) == 1 else "have"))
        if meshes and a.radius is not None:
            ap.error("--radius is the graph of point clouds, and %s %s faces: add --pointcloud to ignore them" % (", ".join(meshes[:5]),
                                                                                                             "has" if len(meshes) == 1 else "have"))
        if meshes:
            ap.error("--index grid indexes point clouds, and %s %s faces: add --pointcloud to ignore them" % (", ".join(meshes[:5]),
                                                                                                              "has" if len(meshes) == 1 else "have"))
    written, skipped = oversegment_scans(a.scans, scenes, a.k_thresh, a.seg_min_verts, a.force, a.workers, a.device, pointcloud=a.pointcloud,
                                         knn=a.knn, viewpoint=a.viewpoint, voxel=a.voxel, index=a.index, radius=a.radius)
    for p in written:
        print("wrote", p)
    for s in skipped:
        print("skipped", s, "(segs.json exists; --force overwrites)")
    print(f"{len(written)} written, {len(skipped)} skipped")
    return 0


if __name__ == "__main__":
    sys.exit(main())
