"""Connected components of a scan on the GPU; scans without their floating pieces; pseudo instances that fall apart.

A laser scan or a fused depth cloud carries specks of a few points away from every surface, a reconstructed mesh small floating patches.
No click reaches them, so each goes down the unlabeled fallback and puts noise into some instance's pseudo label.  `components` labels
every vertex with the lowest vertex index of its component (`sg_components_edges` / `_faces` / `_knn`: one hooking pass over the pairs on
the GPU, integers only, the same bytes on every run; there is no other path).  The graph is an edge list, a mesh's faces, or a kNN table
cut at a length -- the kNN graph as it is, not a radius graph: a point with more than k neighbours inside the length links to its k
nearest only -- or the radius graph itself: every pair of points at most `radius` apart, searched on the grid index
(`sg_components_radius`), with the number of neighbours inside the radius per point as a by-product (`neighbour_counts`,
`sg_radius_count_grid`: the radius outlier filter).

    python -m seggroup_amd.components --scans DIR --out DIR (--min-verts M | --largest) [--pointcloud --knn {5,10,20} --max-edge R
                                      --index {grid,brute}] [--scenes FILE] [--force] [--workers W] [--device D] [--report-only]
                                      [--radius R [--min-neighbours M]]
        every scan directory of --scans -> a scan directory under --out without the small pieces, which every command of the project reads
        as it is: <scene>_vh_clean_2.ply (the kept vertices in ascending raw index with their colours, the faces whose vertices are kept),
        <scene>.clean.npz (kept, new_of_old, comp, the parameters), the segs.json taken at the kept vertices and the aggregation file when
        the source has them; clean_report.json for the run.  A mesh uses its faces; a scan without faces (or --pointcloud) uses its kNN
        graph and NEEDS --max-edge, in the scan's unit.  Results made on the cleaned scans go back to the raw ones with
        `python -m seggroup_amd.transfer --from-scans CLEAN --to-scans RAW ...`: a kept vertex is its own nearest vertex at distance 0.
        --radius R (a scan without faces, or --pointcloud; instead of --max-edge): the radius graph over all points.  --min-neighbours M
        (needs --radius; --min-verts / --largest are then optional): a vertex is kept only if at least M points lie within R of it AND,
        when a size rule is given too, its component in the radius graph over ALL points passes that rule -- one pass, nothing is
        recomputed on the survivors.  <scene>.clean.npz then holds `count`, clean_report.json the radius, R, the cell edge and the
        vertices dropped by each rule.
    python -m seggroup_amd.components --fragments --scans DIR -n EXP --stage S [--layer final] [--root .] [--json OUT] [--max-edge R | --radius R ...]
        per scene the pseudo instances of results/EXP/<scene>/<stage>/pseudo_labels.sgl that are in more than one piece of the scan's own
        graph, their piece sizes, and the share of the vertices outside their instance's largest piece; a report, no label file is touched
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import shutil
import sys
from typing import Optional

import numpy as np

from . import hip, pseudo_labels, scans
from .device import device_tensor, on_stream, stream_ptr, torch_device, workspace
from .prepare import mesh_arrays, pointcloud_knn, read_ply, write_ply

MAP_SUFFIX = ".clean.npz"
REPORT_NAME = "clean_report.json"
KNN_CHOICES = (5, 10, 20)


def _shape2(a, cols, what):
    shape = tuple(a.shape)
    if len(shape) != 2 or (shape[1] != cols if cols else shape[1] < 2):
        raise ValueError("components: %s must be [*, %s], not %r" % (what, cols or ">= 2", shape))
    return int(shape[0]), int(shape[1])


def _cut(max_edge) -> float:
    r = math.inf if max_edge is None else float(max_edge)
    if not r > 0.0:
        raise ValueError("components: max_edge must be a length > 0 (None or inf: no cut), not %r" % (max_edge,))
    return r


def _radius(radius) -> float:
    r = float(radius)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError("components: radius must be a finite length > 0, not %r" % (radius,))
    return r


def _cloud(xyz, what):
    shape = tuple(xyz.shape)
    if len(shape) != 2 or shape[1] < 3 or shape[0] < 1:
        raise ValueError("%s: xyz must be [N >= 1, >= 3], not %r" % (what, shape))
    if shape[0] > hip.MAX_GRID_POINTS:
        raise hip.SgError(hip.SG_EUNSUP, "%s: %d points; the grid path holds at most 2^24" % (what, shape[0]))
    return int(shape[0])


def radius_stats() -> dict:
    """the calling thread's last radius call (`components(radius=)`, `neighbour_counts`): cells per axis, occupied cells, the largest cell,
    the cell edge, the ring count R of the block a query reads; pair tests and pairs passed are counted in timed calls only"""
    stats = hip.grid_stats("radius_grid", ("R", "pair_tests", "pairs_passed"), slots=9)
    stats["cells"] = list(stats["cells"])
    return stats


def neighbour_counts(xyz, radius, cell=0.0, device=None, stream=None):
    """-> int32 [N] (a device tensor): per point the number of OTHER points whose fp32 d2 <= radius^2, coincident points
    included -- the radius outlier filter's figure.  `cell`: the grid's forced edge, 0 or None for the library's choice; it cannot change
    a result."""
    r, c = _radius(radius), hip.knn_cell(cell)
    n = _cloud(xyz, "neighbour_counts")
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_tensor(xyz, torch.float32, dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_radius_grid_ws_bytes(n), dev)
        hip.check(lib.sg_radius_count_grid(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, r, c, count.data_ptr(), ws.data_ptr(), ws.numel(),
                                           stream_ptr(stream)))
    return count


def radius_pairs(d_xyz, n, r, c, dev, stream):
    """The query form of sg_radius_neighbours_grid over a device cloud [n, >= 3] -> (T, the number of (ordered) pairs of the radius graph,
    which is not known before; the rows' offsets int64 [n + 1]).  The library answers SG_ENOMEM with T whenever there is a pair.  The
    caller holds the device and the stream (`on_stream`)."""
    import torch
    lib = hip.lib()
    indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    total = C.c_int64(0)
    ws = workspace(lib.sg_radius_neighbours_ws_bytes(n, 0), dev)
    rc = lib.sg_radius_neighbours_grid(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, r, c, 0, indptr.data_ptr(), None, C.byref(total), ws.data_ptr(),
                                       ws.numel(), stream_ptr(stream))
    if rc != hip.SG_ENOMEM or total.value <= 0:
        hip.check(rc)
    return int(total.value), indptr


def radius_neighbours(xyz, radius, cell=0.0, device=None, stream=None):
    """-> (indptr int64 [N + 1], indices int32 [T]) device tensors: the radius graph of `neighbour_counts` written down in CSR form
    (DESIGN.md 8l).  The row of i, indices[indptr[i]:indptr[i + 1]], holds every OTHER point whose fp32 d2 <= radius^2 in ascending
    index; `cell` cannot change a byte.  Two calls of the library: one that counts (T is not known before), one that fills."""
    r, c = _radius(radius), hip.knn_cell(cell)
    n = _cloud(xyz, "radius_neighbours")
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_tensor(xyz, torch.float32, dev)
        t, indptr = radius_pairs(d_xyz, n, r, c, dev, stream)
        indices = torch.empty(t, dtype=torch.int32, device=dev)
        if t:
            ws = workspace(lib.sg_radius_neighbours_ws_bytes(n, t), dev)
            hip.check(lib.sg_radius_neighbours_grid(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, r, c, t, indptr.data_ptr(), indices.data_ptr(),
                                                    C.byref(C.c_int64(0)), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
    return indptr, indices


def components(V: int, *, edges=None, faces=None, knn=None, radius=None, xyz=None, max_edge=None, labels=None, cell=0.0, device=None,
               stream=None):
    """-> (comp int32 [V], size int32 [V], C): comp[v] = the lowest vertex index of v's component, size[v] = its vertex count (device
    tensors), C = the number of components.  Exactly one of `edges` [E,2], `faces` [F,3], `knn` [V, k+1] (with `xyz` [V, >= 3]; a pair
    counts when its fp32 d2 <= max_edge^2; max_edge=None: every pair).  `labels` [V]: a pair counts only when both ends hold the same
    value.  NumPy arrays or tensors.  A fourth source, `radius` (with `xyz` [V, >= 3]; `cell`: the grid's forced edge, 0 for the
    library's choice): the radius graph, every pair of points whose fp32 d2 <= radius^2.  Anything else is a ValueError
    before a device call."""
    V = int(V)
    given = [n for n, a in (("edges", edges), ("faces", faces), ("knn", knn), ("radius", radius)) if a is not None]
    if len(given) != 1:
        raise ValueError("components: exactly one of edges, faces, knn and radius is needed, not %s" % (given or "none"))
    if V < 1:
        raise ValueError("components: a graph needs at least one vertex")
    if knn is None and radius is None and xyz is not None:
        raise ValueError("components: xyz belongs to the knn and radius forms")
    if knn is None and max_edge is not None:
        raise ValueError("components: max_edge belongs to the knn form")
    grid_cell = hip.knn_cell(cell)
    if radius is None and grid_cell != 0.0:
        raise ValueError("components: cell belongs to the radius form")
    if radius is not None:
        if xyz is None:
            raise ValueError("components: the radius form needs xyz")
        if _cloud(xyz, "components") != V:
            raise ValueError("components: the radius form needs xyz [V, >= 3] with V = %d" % V)
        reach = _radius(radius)
    elif edges is not None:
        count, _ = _shape2(edges, 2, "edges")
    elif faces is not None:
        count, _ = _shape2(faces, 3, "faces")
    else:
        if xyz is None:
            raise ValueError("components: the knn form needs xyz")
        count, row = _shape2(knn, 0, "knn")
        if len(tuple(xyz.shape)) != 2 or xyz.shape[1] < 3 or int(xyz.shape[0]) != V or count != V:
            raise ValueError("components: the knn form needs knn [V, k+1] and xyz [V, >= 3] with V = %d" % V)
        cut = _cut(max_edge)
    if labels is not None and tuple(labels.shape) != (V,):
        raise ValueError("components: labels must be [%d], not %r" % (V, tuple(labels.shape)))

    import torch
    dev = torch_device(device)
    lib = hip.lib()
    need = lib.sg_radius_grid_ws_bytes(V) if radius is not None else lib.sg_components_ws_bytes(V)
    if need == 0:
        raise hip.SgError(hip.SG_EUNSUP, "components: %d vertices; a graph holds at most 2^27" % V)
    with torch.cuda.device(dev), on_stream(stream):
        d_lab = None if labels is None else device_tensor(labels, torch.int32, dev)
        comp = torch.empty(V, dtype=torch.int32, device=dev)
        size = torch.empty(V, dtype=torch.int32, device=dev)
        ws = workspace(need, dev)
        c = C.c_int(0)
        tail = (hip.ptr(d_lab), comp.data_ptr(), size.data_ptr(), C.byref(c), ws.data_ptr(), ws.numel(), stream_ptr(stream))
        if radius is not None:
            d_xyz = device_tensor(xyz, torch.float32, dev)
            rc = lib.sg_components_radius(d_xyz.data_ptr(), int(d_xyz.shape[1]), V, reach, grid_cell, *tail)
        elif edges is not None:
            d_src = device_tensor(edges, torch.int32, dev)
            rc = lib.sg_components_edges(d_src.data_ptr() if count else None, count, V, *tail)
        elif faces is not None:
            d_src = device_tensor(faces, torch.int32, dev)
            rc = lib.sg_components_faces(d_src.data_ptr() if count else None, count, V, *tail)
        else:
            d_src, d_xyz = device_tensor(knn, torch.int32, dev), device_tensor(xyz, torch.float32, dev)
            rc = lib.sg_components_knn(d_xyz.data_ptr(), int(d_xyz.shape[1]), d_src.data_ptr(), V, row, cut, *tail)
        hip.check(rc)                                            # the call synchronised the stream
    return comp, size, c.value


def keep_mask(comp, size, min_verts: Optional[int] = None, largest: bool = False):
    """-> bool [V]: the vertices of the components with size >= min_verts, or (largest=True) of the largest component alone, the one with
    the lowest comp among equals.  Exactly one of the two; tensors give a tensor, arrays an array."""
    if (min_verts is None) == (not largest):
        raise ValueError("keep_mask: exactly one of min_verts and largest is needed")
    if largest:
        big = size == size.max()
        return comp == comp[big].min()
    if int(min_verts) < 1:
        raise ValueError("keep_mask: min_verts must be at least 1")
    return size >= int(min_verts)


def clean_arrays(keep, faces):
    """-> (kept int32 [M] ascending, new_of_old int32 [V], -1 where dropped, faces int32 [F',3]: the faces whose three vertices are kept,
    renumbered, in their original order) as tensors on keep's device"""
    import torch
    keep = keep.to(torch.bool)
    kept = torch.nonzero(keep).reshape(-1).to(torch.int32)
    rank = torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1
    new_of_old = torch.where(keep, rank, torch.full_like(rank, -1))
    f = faces.to(device=keep.device, dtype=torch.long).reshape(-1, 3)
    whole = keep[f].all(1)
    return kept, new_of_old, new_of_old[f[whole]].reshape(-1, 3).to(torch.int32)


def _scan_graph(xyz, faces, pointcloud, knn, max_edge, index, what, radius=None):
    """-> (source name, keyword arguments of `components`) for a scan's own graph; max_edge is read on the kNN path only, radius takes
    its place (the radius graph)"""
    if radius is not None:
        if max_edge is not None:
            raise ValueError(f"{what}: radius and max_edge are two different graphs; give one")
        if not (pointcloud or faces.shape[0] == 0):
            raise ValueError(f"{what}: radius belongs to a scan without faces (or pointcloud=True); a mesh uses its faces")
        return "radius", dict(radius=_radius(radius), xyz=xyz)
    if pointcloud or faces.shape[0] == 0:
        if max_edge is None:
            raise ValueError(f"{what}: a scan without faces (or pointcloud=True) needs max_edge, in the scan's unit; a default would be a guess")
        _cut(max_edge)
        return "knn", dict(knn=pointcloud_knn(xyz, int(knn), index=index), xyz=xyz, max_edge=max_edge)
    return "faces", dict(faces=faces)


def clean_scan(scene_path: str, out_dir: str, min_verts: Optional[int] = None, largest: bool = False, pointcloud: bool = False, knn: int = 10,
               max_edge: Optional[float] = None, index: str = "grid", force: bool = False, device=None, stream=None,
               report_only: bool = False, radius: Optional[float] = None, min_neighbours: Optional[int] = None) -> Optional[dict]:
    """One scan directory -> <out_dir>/<scene>/ without the small pieces (see the module's doc); -> its entry of clean_report.json, or
    None when the cleaned PLY was there already (never overwritten without `force`).  `report_only`: the entry alone, nothing written.
    `radius` (a scan without faces, or pointcloud=True): the radius graph in place of the kNN graph.  `min_neighbours` (needs `radius`;
    min_verts / largest are then optional): keep a vertex only if that many points lie within `radius` of it and its component in the
    radius graph over ALL points passes the size rule, when one is given."""
    import torch
    _check_rules("clean_scan", min_verts, largest, radius, min_neighbours)
    hip.knn_index(index)
    scene = scans.scene_name(scene_path)
    dst = os.path.join(out_dir, scene)
    ply_out = os.path.join(dst, scene + "_vh_clean_2.ply")
    if not report_only and os.path.exists(ply_out) and not force:
        return None
    xyz, rgb, faces = mesh_arrays(read_ply(os.path.join(scene_path, scene + "_vh_clean_2.ply")))
    source, graph = _scan_graph(xyz, faces, pointcloud, knn, max_edge, index, scene, radius)
    v = int(xyz.shape[0])
    d_comp, d_size, n_comp = components(v, device=device, stream=stream, **graph)
    stats = radius_stats() if source == "radius" else None
    d_count = None if min_neighbours is None else neighbour_counts(xyz, radius, device=d_comp.device, stream=stream)
    with torch.cuda.device(d_comp.device):                       # both calls synchronised their stream
        sized = min_verts is not None or largest
        d_keep = keep_mask(d_comp, d_size, min_verts, largest) if sized else torch.ones(v, dtype=torch.bool, device=d_comp.device)
        by_size = int((~d_keep).sum())
        if d_count is not None:
            d_dense = d_count >= int(min_neighbours)
            by_count = int((~d_dense).sum())
            d_keep = d_keep & d_dense
        d_kept, d_new, d_faces = clean_arrays(d_keep, torch.from_numpy(faces).to(d_comp.device))
        roots = d_comp == torch.arange(v, dtype=torch.int32, device=d_comp.device)
        sizes = torch.sort(d_size[roots], descending=True)[0]
        kept_components = int((roots & d_keep).sum()) if d_count is None else int(torch.unique(d_comp[d_keep]).numel())
        kept, new_of_old, new_faces, comp = d_kept.cpu().numpy(), d_new.cpu().numpy(), d_faces.cpu().numpy(), d_comp.cpu().numpy()
        largest_sizes = sizes[:10].cpu().tolist()
    entry = {"V": v, "M": int(kept.shape[0]), "components": int(n_comp), "kept_components": kept_components, "largest_sizes": largest_sizes,
             "source": source, "F": int(faces.shape[0]), "kept_F": int(new_faces.shape[0])}
    if stats is not None:
        entry.update(radius=float(radius), R=stats["R"], cell=stats["cell"], dropped={"size": by_size})
        if d_count is not None:
            entry["dropped"]["min_neighbours"] = by_count
    doc, ids = kept_segs(scene_path, scene, v, kept)
    if doc is not None:
        before, after = np.unique(ids), np.unique(ids[kept])
        entry.update(source_segments=int(before.shape[0]), kept_segments=int(after.shape[0]), lost_segments=np.setdiff1d(before, after).tolist())
    if report_only:
        return entry
    extra = {}
    if source == "radius":
        extra.update(radius=np.float32(radius), min_neighbours=np.int32(-1 if min_neighbours is None else min_neighbours))
    if d_count is not None:
        extra["count"] = d_count.cpu().numpy()
    write_kept_scan(scene_path, dst, scene, xyz, rgb, kept, new_of_old, new_faces, doc, comp=comp,
                    min_verts=np.int32(-1 if min_verts is None else min_verts), largest=np.bool_(largest), source=np.str_(source),
                    knn=np.int32(knn if source == "knn" else 0), max_edge=np.float32(np.inf if max_edge is None else max_edge), **extra)
    return entry


def kept_segs(scene_path: str, scene: str, v: int, kept):
    """the scan's segs.json taken at the kept vertices -> (its document with segIndices cut down, the raw scan's int64 [V] ids), or
    (None, None) for a scan without one"""
    segs = os.path.join(scene_path, scans.segs_json_name(scene))
    if not os.path.exists(segs):
        return None, None
    with open(segs) as f:
        doc = json.load(f)
    ids = np.asarray(doc["segIndices"], dtype=np.int64)
    if ids.shape[0] != v:
        raise ValueError(f"{segs}: {ids.shape[0]} segIndices for {v} vertices")
    doc["segIndices"] = ids[kept].tolist()
    return doc, ids


def write_kept_scan(scene_path: str, dst: str, scene: str, xyz, rgb, kept, new_of_old, new_faces, doc, **map_fields) -> None:
    """A scan directory `dst` that holds the kept vertices of <scene_path> only, for `clean_scan` and `planes --remove`: the PLY (kept
    vertices in ascending raw index with their colours, `new_faces`), <scene>.clean.npz (kept, new_of_old, then `map_fields` in the
    caller's order), `doc` (kept_segs') as the segs.json when there is one, and the aggregation file copied."""
    os.makedirs(dst, exist_ok=True)
    write_ply(os.path.join(dst, scene + scans.PLY_SUFFIX), xyz[kept], rgb[kept], new_faces)
    np.savez(os.path.join(dst, scene + MAP_SUFFIX), kept=kept, new_of_old=new_of_old, **map_fields)
    if doc is not None:
        with open(os.path.join(dst, scans.segs_json_name(scene)), "w") as f:
            json.dump(doc, f)
    agg = os.path.join(scene_path, scene + ".aggregation.json")
    if os.path.exists(agg):
        shutil.copyfile(agg, os.path.join(dst, scene + ".aggregation.json"))


def _check_rules(who, min_verts, largest, radius, min_neighbours):
    if min_neighbours is None:
        if (min_verts is None) == (not largest):
            raise ValueError(f"{who}: exactly one of min_verts and largest is needed")
        return
    if radius is None:
        raise ValueError(f"{who}: min_neighbours counts the points within radius; radius is needed")
    if int(min_neighbours) < 1:
        raise ValueError(f"{who}: min_neighbours must be at least 1")
    if min_verts is not None and largest:
        raise ValueError(f"{who}: at most one of min_verts and largest")


def clean_scans(scans_dir: str, out_dir: str, min_verts: Optional[int] = None, largest: bool = False, pointcloud: bool = False, knn: int = 10,
                max_edge: Optional[float] = None, index: str = "grid", scenes=None, force: bool = False, workers: int = 4, device=None,
                report_only: bool = False, radius: Optional[float] = None, min_neighbours: Optional[int] = None):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    <out_dir>/clean_report.json.  Workers are threads, each with its own stream."""
    _check_rules("clean_scans", min_verts, largest, radius, min_neighbours)
    dev = torch_device(device)
    head = {"min_verts": min_verts, "largest": bool(largest), "pointcloud": bool(pointcloud), "knn": int(knn),
            "max_edge": None if max_edge is None else float(max_edge), "index": index, "report_only": bool(report_only)}
    if radius is not None:
        head.update(radius=float(radius), min_neighbours=None if min_neighbours is None else int(min_neighbours))
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, head,
                           lambda path, stream: clean_scan(path, out_dir, min_verts, largest, pointcloud, knn, max_edge, index, force, device=dev,
                                                           stream=stream, report_only=report_only, radius=radius, min_neighbours=min_neighbours))


# ---- pseudo instances that fall apart -------------------------------------------------------------------------------------------------
def fragments(labels, V: int, **graph) -> dict:
    """The label-filtered components of a graph (`graph`: the source keywords of `components`) -> dict(instances, fragmented,
    outside_largest, outside_share, pieces {label: sizes, largest first} of the labels in more than one piece).  Every value of
    `labels` counts as an instance.  `radius=R, xyz=...` is the radius graph."""
    import torch
    comp, _, _ = components(V, labels=labels, **graph)
    with torch.cuda.device(comp.device):
        lab = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels).to(device=comp.device, dtype=torch.int64)
        key, count = torch.unique(torch.stack([lab, comp.to(torch.int64)], 1), dim=0, return_counts=True)
        key, count = key.cpu().numpy(), count.cpu().numpy()
    inst, first, pieces_per = np.unique(key[:, 0], return_index=True, return_counts=True)
    pieces, outside = {}, 0
    for lb, at, n in zip(inst.tolist(), first.tolist(), pieces_per.tolist()):
        if n > 1:
            sizes = sorted(count[at:at + n].tolist(), reverse=True)
            pieces[int(lb)] = sizes
            outside += sum(sizes[1:])
    return {"V": int(V), "instances": int(inst.shape[0]), "fragmented": len(pieces), "outside_largest": int(outside),
            "outside_share": outside / float(V), "pieces": pieces}


def fragments_scene(scene_path: str, exp: str, stage: str, layer: str = "final", root: str = ".", pointcloud: bool = False, knn: int = 10,
                    max_edge: Optional[float] = None, index: str = "grid", device=None, stream=None, radius: Optional[float] = None) -> dict:
    """`fragments` of one scene's `<layer>.ins` vector on the scan's own graph (its faces, its kNN graph cut at max_edge, or its radius
    graph)"""
    scene = scans.scene_name(scene_path)
    lab = pseudo_labels.load(os.path.join(root, "results", exp, scene, stage)).vector(layer + ".ins")
    xyz, _, faces = mesh_arrays(read_ply(os.path.join(scene_path, scene + "_vh_clean_2.ply")))
    if lab.shape[0] != xyz.shape[0]:
        raise ValueError(f"{scene}: {lab.shape[0]} labels for {xyz.shape[0]} vertices")
    source, graph = _scan_graph(xyz, faces, pointcloud, knn, max_edge, index, scene, radius)
    out = fragments(lab, int(xyz.shape[0]), device=device, stream=stream, **graph)
    out["source"] = source
    out["pieces"] = {str(k): v for k, v in out["pieces"].items()}
    return out


def fragments_scans(scans_dir: str, exp: str, stage: str, layer: str = "final", root: str = ".", scenes=None, workers: int = 4, device=None,
                    **graph) -> dict:
    dev = torch_device(device)
    if scenes is None:
        base = os.path.join(root, "results", exp)
        scenes = [s for s in scans.scan_names(scans_dir) if os.path.isdir(os.path.join(base, s, stage))]
    return dict(scans.map_scans(scenes, workers, dev, lambda scene, stream: fragments_scene(os.path.join(scans_dir, scene), exp, stage, layer, root,
                                                                                            device=dev, stream=stream, **graph)))


def _positive(text):
    r = float(text)
    if not (r > 0.0 and math.isfinite(r)):
        raise argparse.ArgumentTypeError("a finite length > 0 is needed, not %s" % text)
    return r


def _needs_max_edge(scans_dir, scenes, pointcloud):
    if pointcloud:
        return "--pointcloud"
    for s in scenes:
        if scans.declared_faces(os.path.join(scans_dir, s, s + "_vh_clean_2.ply")) == 0:
            return "%s has no faces and" % s
    return None


def _radius_needs_clouds(ap, scans_dir, scenes, pointcloud):
    """--radius is the graph of a scan without faces (or of --pointcloud): a mesh in the list is a parser error, not a silent switch"""
    if pointcloud:
        return
    for s in scenes:
        if scans.declared_faces(os.path.join(scans_dir, s, s + "_vh_clean_2.ply")) != 0:
            ap.error(f"--radius belongs to a scan without faces: {s} is a mesh (--pointcloud ignores the faces)")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.components", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--out", default=None, help="where the cleaned scan directories and clean_report.json go")
    ap.add_argument("--min-verts", type=int, default=None, help="keep the components with at least this many vertices")
    ap.add_argument("--largest", action="store_true", help="keep the largest component alone")
    ap.add_argument("--pointcloud", action="store_true", help="use the kNN graph even where the scan has faces")
    ap.add_argument("--knn", type=int, default=10, choices=KNN_CHOICES, help="neighbours per point of the kNN graph")
    ap.add_argument("--max-edge", type=_positive, default=None, help="kNN graph: the longest pair that counts, in the scan's unit (no default)")
    ap.add_argument("--index", default="grid", choices=sorted(hip.KNN_INDEX), help="kNN graph: the neighbour search")
    ap.add_argument("--radius", type=_positive, default=None,
                    help="the radius graph in place of the kNN graph: every pair of points at most this far apart, in the scan's unit")
    ap.add_argument("--min-neighbours", type=int, default=None, help="with --radius: keep the vertices with at least this many points within the radius")
    ap.add_argument("--report-only", action="store_true", help="write clean_report.json and no scan")
    scans.add_batch_arguments(ap, "overwrite existing cleaned scans")
    ap.add_argument("--fragments", action="store_true", help="report the pseudo instances that are in more than one piece")
    ap.add_argument("-n", "--exp_name", default=None, help="--fragments: name of the experiment")
    ap.add_argument("--stage", default="epoch_last", help="--fragments: the export directory's name")
    ap.add_argument("--layer", default="final", help="--fragments: final or layer_1 .. layer_4")
    ap.add_argument("--root", default=".", help="--fragments: directory holding results/ (default: CWD)")
    ap.add_argument("--json", default=None, help="--fragments: write the report here as well")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    scenes = scans.scene_list(a.scenes)
    if a.radius is not None and a.max_edge is not None:
        ap.error("--radius and --max-edge are two different graphs: give one")
    if a.min_neighbours is not None:
        if a.radius is None:
            ap.error("--min-neighbours counts the points within --radius R: --radius is needed")
        if a.min_neighbours < 1:
            ap.error("--min-neighbours must be at least 1")
    if a.fragments:
        if not a.exp_name:
            ap.error("--fragments needs -n EXP")
        if a.min_verts is not None or a.largest:
            ap.error("--fragments is a report: --min-verts / --largest belong to cleaning")
        if a.min_neighbours is not None:
            ap.error("--fragments is a report: --min-neighbours belongs to cleaning")
        names = scenes if scenes is not None else [s for s in scans.scan_names(a.scans)
                                                   if os.path.isdir(os.path.join(a.root, "results", a.exp_name, s, a.stage))]
        why = _needs_max_edge(a.scans, names, a.pointcloud)
        if a.radius is not None:
            _radius_needs_clouds(ap, a.scans, names, a.pointcloud)
        elif why and a.max_edge is None:
            ap.error(f"{why} needs --max-edge R (the scan's unit; there is no default)")
        if not why and a.max_edge is not None:
            ap.error("--max-edge belongs to the kNN graph: every scan here is a mesh (--pointcloud ignores the faces)")
        graph = dict(radius=a.radius) if a.radius is not None else {}
        rep = fragments_scans(a.scans, a.exp_name, a.stage, a.layer, a.root, names, a.workers, a.device, pointcloud=a.pointcloud, knn=a.knn,
                              max_edge=a.max_edge, index=a.index, **graph)
        for scene, e in rep.items():
            print("fragments", scene, e["instances"], "instances,", e["fragmented"], "in pieces,", "%.4f" % e["outside_share"], "outside")
        if a.json:
            scans.write_report(a.json, {"exp": a.exp_name, "stage": a.stage, "layer": a.layer, "scenes": rep})
        return 0
    if not a.out:
        ap.error("cleaning needs --out DIR")
    if a.min_neighbours is None and (a.min_verts is None) == (not a.largest):
        ap.error("exactly one of --min-verts M and --largest is needed")
    if a.min_verts is not None and a.largest:
        ap.error("at most one of --min-verts M and --largest")
    if a.min_verts is not None and a.min_verts < 1:
        ap.error("--min-verts must be at least 1")
    names = scenes if scenes is not None else scans.scan_names(a.scans)
    why = _needs_max_edge(a.scans, names, a.pointcloud)
    if a.radius is not None:
        _radius_needs_clouds(ap, a.scans, names, a.pointcloud)
    elif why and a.max_edge is None:
        ap.error(f"{why} needs --max-edge R (the scan's unit; there is no default)")
    if not why and a.max_edge is not None:
        ap.error("--max-edge belongs to the kNN graph: every scan here is a mesh (--pointcloud ignores the faces)")
    new = dict(radius=a.radius, min_neighbours=a.min_neighbours) if a.radius is not None else {}
    report, skipped = clean_scans(a.scans, a.out, a.min_verts, a.largest, a.pointcloud, a.knn, a.max_edge, a.index, names, a.force, a.workers,
                                  a.device, a.report_only, **new)
    scans.print_outcome(report, skipped, lambda scene, e: ("cleaned", scene, e["V"], "->", e["M"], "vertices,", e["components"], "->",
                                                           e["kept_components"], "components"),
                        "(cleaned scan exists; --force overwrites)", "reported" if a.report_only else "written")
    return 0


if __name__ == "__main__":
    sys.exit(main())
