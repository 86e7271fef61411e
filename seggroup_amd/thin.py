"""Voxel thinning of a large point cloud, and lifting results back to every point.

A laser scan, an S3DIS room or a fused depth cloud has millions of points at a density that varies with range; the point-cloud path
(`oversegment.segment_pointcloud`, `prepare.pointcloud_knn`) takes 2^20.  The front end is a voxel grid: keep ONE INPUT POINT per occupied
voxel -- the one nearest the cell centre, the lowest index among equals --, work on the thinned cloud, and carry every per-point result
back through the map.  The representatives are input points (colours and every other attribute stay real) and come out in ascending
raw index, so a grid fine enough to leave every point alone is the identity.  Keys, sort, selection and compaction run on the GPU
(`sg_cloud_thin`, up to 2^27 points); there is no other path.  Lifting is a gather.

    python -m seggroup_amd.thin --scans DIR --out DIR --voxel H [--scenes LIST] [--force] [--workers W] [--device D]
        every scan directory of --scans -> a thinned scan directory under --out that every command of the project reads as it is:
        <scene>_vh_clean_2.ply (vertices only: a mesh LOSES ITS FACES), <scene>.thin.npz (rep, thin_of_point, voxel, lo), the segs.json
        taken at the representatives and the aggregation file when the source has them; thin_report.json for the run
    python -m seggroup_amd.thin --lift -n EXP --stage S --maps THINNED_SCANS --out ROOT2 [--root .] [--scenes LIST]
        results/EXP/<scene>/<stage>/ of --root (made on the thinned scans) -> the same files for the raw scans under ROOT2/results/...:
        pseudo_labels.sgl and per-vector .npy files; .txt is not read (run `expand` on the lifted .sgl)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import sys
from typing import Optional

import numpy as np

from . import hip, pseudo_labels, scans
from .device import device_cloud, on_stream, stream_ptr, sync, torch_device, workspace
from .prepare import mesh_arrays, read_ply, write_ply

MAP_SUFFIX = ".thin.npz"
REPORT_NAME = "thin_report.json"


def thin_cloud(xyz, voxel: float, device=None, stream=None):
    """-> (rep int32 [M], thin_of_point int32 [N], lo float32 [3]) device tensors: rep = the representatives' indices, ascending;
    rep[thin_of_point[i]] stands for point i; lo = the corner of the grid.  xyz: [N, >= 3] rows, xyz first (NumPy or tensor)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, n = device_cloud(xyz, dev, "thin_cloud")
        stride = int(d_xyz.shape[1])
        need = lib.sg_cloud_thin_ws_bytes(n)
        if need == 0:
            raise hip.SgError(hip.SG_EUNSUP, "thin_cloud: %d points; a cloud holds at most 2^27" % n)
        rep = torch.empty(n, dtype=torch.int32, device=dev)
        top = torch.empty(n, dtype=torch.int32, device=dev)
        ws = workspace(need, dev)
        m, lo = C.c_int(0), (C.c_float * 3)()
        hip.check(lib.sg_cloud_thin(d_xyz.data_ptr(), stride, n, float(voxel), rep.data_ptr(), top.data_ptr(), C.byref(m), lo, ws.data_ptr(),
                                    ws.numel(), stream_ptr(stream)))
        rep = rep[:m.value].clone()
        d_lo = torch.tensor(list(lo), dtype=torch.float32, device=dev)
        sync(stream)
    return rep, top, d_lo


def lift(values, thin_of_point):
    """values[thin_of_point] on the leading axis: a result per thinned point -> the result per raw point.  NumPy arrays and tensors."""
    try:
        import torch
    except ImportError:                                          # pragma: no cover
        torch = None
    if torch is not None and isinstance(values, torch.Tensor):
        idx = thin_of_point if isinstance(thin_of_point, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(thin_of_point))
        return values.index_select(0, idx.to(device=values.device, dtype=torch.long))
    if torch is not None and isinstance(thin_of_point, torch.Tensor):
        thin_of_point = thin_of_point.cpu().numpy()
    return np.asarray(values)[np.asarray(thin_of_point)]


def lift_sgl(src: str, dst: str, thin_of_point) -> str:
    """A `pseudo_labels.sgl` made on a thinned scan -> one for the raw scan: the same tables, seg_of_vertex[thin_of_point], the raw V."""
    lab = pseudo_labels.load(src)
    top = np.asarray(thin_of_point.cpu() if hasattr(thin_of_point, "cpu") else thin_of_point).reshape(-1)
    if top.size and (int(top.min()) < 0 or int(top.max()) >= lab.V):
        raise ValueError("lift_sgl: the map names thinned points outside 0..%d" % (lab.V - 1))
    os.makedirs(os.path.dirname(os.path.abspath(pseudo_labels.sgl_path(dst))), exist_ok=True)
    return pseudo_labels.write(dst, lab.tables, lab.seg_of_vertex[top])


def load_map(maps_dir: str, scene: str):
    """-> the arrays of <maps_dir>/<scene>/<scene>.thin.npz"""
    with np.load(os.path.join(maps_dir, scene, scene + MAP_SUFFIX)) as z:
        return {k: z[k] for k in ("rep", "thin_of_point", "voxel", "lo")}


def thin_scan(scene_path: str, out_dir: str, voxel: float, force: bool = False, device=None, stream=None) -> Optional[dict]:
    """One scan directory -> <out_dir>/<scene>/ (see the module's doc); -> its entry of thin_report.json, or None when the thinned
    PLY was there already (never overwritten without `force`)."""
    scene = scans.scene_name(scene_path)
    dst = os.path.join(out_dir, scene)
    ply_out = os.path.join(dst, scene + "_vh_clean_2.ply")
    if os.path.exists(ply_out) and not force:
        return None
    xyz, rgb, _ = mesh_arrays(read_ply(os.path.join(scene_path, scene + "_vh_clean_2.ply")))
    d_rep, d_top, d_lo = thin_cloud(xyz, voxel, device=device, stream=stream)
    rep, top, lo = d_rep.cpu().numpy(), d_top.cpu().numpy(), d_lo.cpu().numpy()
    os.makedirs(dst, exist_ok=True)
    write_ply(ply_out, xyz[rep], rgb[rep], np.zeros((0, 3), np.int32))
    np.savez(os.path.join(dst, scene + MAP_SUFFIX), rep=rep, thin_of_point=top, voxel=np.float32(voxel), lo=lo)
    h = np.float32(voxel)
    entry = {"V": int(xyz.shape[0]), "M": int(rep.shape[0]), "voxel": float(h),
             "cells": [int(np.floor((xyz[:, a].max() - lo[a]) / h)) + 1 for a in range(3)],
             "largest_voxel": int(np.bincount(top, minlength=rep.shape[0]).max())}
    segs = os.path.join(scene_path, scans.segs_json_name(scene))
    if os.path.exists(segs):
        with open(segs) as f:
            doc = json.load(f)
        ids = np.asarray(doc["segIndices"], dtype=np.int64)
        if ids.shape[0] != xyz.shape[0]:
            raise ValueError(f"{segs}: {ids.shape[0]} segIndices for {xyz.shape[0]} vertices")
        doc["segIndices"] = ids[rep].tolist()
        with open(os.path.join(dst, scans.segs_json_name(scene)), "w") as f:
            json.dump(doc, f)
        before, after = np.unique(ids), np.unique(ids[rep])
        entry.update(source_segments=int(before.shape[0]), kept_segments=int(after.shape[0]),
                     lost_segments=np.setdiff1d(before, after).tolist())
    agg = os.path.join(scene_path, scene + ".aggregation.json")
    if os.path.exists(agg):
        shutil.copyfile(agg, os.path.join(dst, scene + ".aggregation.json"))
    return entry


def thin_scans(scans_dir: str, out_dir: str, voxel: float, scenes=None, force: bool = False, workers: int = 4, device=None):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    <out_dir>/thin_report.json.  Workers are threads, each with its own stream."""
    dev = torch_device(device)
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, {"voxel": float(np.float32(voxel))},
                           lambda path, stream: thin_scan(path, out_dir, voxel, force, device=dev, stream=stream))


def lift_stage(src: str, dst: str, index_map, n_src: int, verb: str = "lift", unit: str = "thinned points"):
    """The files of one export directory through a gather map: pseudo_labels.sgl and every .npy vector of `src`, each of `n_src` values
    on its leading axis, -> the same names under `dst` with index_map.shape[0] values; -> the files written.  `verb` and `unit` word the
    errors for the caller's map."""
    os.makedirs(dst, exist_ok=True)
    files = []
    if os.path.isfile(os.path.join(src, pseudo_labels.SGL_NAME)):
        files.append(lift_sgl(os.path.join(src, pseudo_labels.SGL_NAME), os.path.join(dst, pseudo_labels.SGL_NAME), index_map))
    for name in sorted(os.listdir(src)):
        if name.endswith(".npy"):
            vec = np.load(os.path.join(src, name))
            if vec.shape[0] != n_src:
                raise ValueError(f"{src}/{name}: {vec.shape[0]} values for {n_src} {unit}")
            np.save(os.path.join(dst, name), lift(vec, index_map))
            files.append(os.path.join(dst, name))
    if not files:
        raise FileNotFoundError(f"{src}: neither {pseudo_labels.SGL_NAME} nor .npy vectors (.txt is not read: {verb} the .sgl and run expand)")
    return files


def lift_results(exp: str, stage: str, maps_dir: str, out_root: str, root: str = ".", scenes=None):
    """results/<exp>/<scene>/<stage>/ under `root` -> the lifted files under <out_root>/results/<exp>/<scene>/<stage>/ for every scene
    (default: every scene of the experiment that has a map); -> [(scene, files written)].  Needs no GPU."""
    base = os.path.join(root, "results", exp)
    if scenes is None:
        scenes = sorted(s for s in os.listdir(base) if os.path.exists(os.path.join(maps_dir, s, s + MAP_SUFFIX)))
    done = []
    for scene in scenes:
        src = os.path.join(base, scene, stage)
        if not os.path.isdir(src):
            raise FileNotFoundError(f"{src}: no such export directory")
        top = load_map(maps_dir, scene)["thin_of_point"]
        done.append((scene, lift_stage(src, os.path.join(out_root, "results", exp, scene, stage), top, int(top.max()) + 1 if top.size else 0)))
    return done


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.thin", description=__doc__.split("\n\n")[0])
    ap.add_argument("--lift", action="store_true", help="lift results made on thinned scans back to the raw scans")
    ap.add_argument("--scans", default=None, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--out", required=True, help="where the thinned scan directories go; with --lift, the root that receives results/")
    ap.add_argument("--voxel", type=float, default=None, help="edge of the voxel grid, in the scan's unit")
    scans.add_batch_arguments(ap, "overwrite existing thinned scans")
    ap.add_argument("-n", "--exp_name", default=None, help="--lift: name of the experiment")
    ap.add_argument("--stage", default="epoch_last", help="--lift: the export directory's name")
    ap.add_argument("--maps", default=None, help="--lift: the thinned scans (their <scene>.thin.npz hold the maps)")
    ap.add_argument("--root", default=".", help="--lift: directory holding results/ (default: CWD)")
    a = ap.parse_args(argv)
    if a.lift:
        if not a.exp_name or not a.maps:
            ap.error("--lift needs -n EXP and --maps THINNED_SCANS")
        done = lift_results(a.exp_name, a.stage, a.maps, a.out, a.root, scans.scene_list(a.scenes))
        for scene, files in done:
            print("lifted", scene, len(files), "files")
        print(f"{len(done)} scenes lifted")
        return 0
    if not a.scans or a.voxel is None:
        ap.error("thinning needs --scans DIR and --voxel H")
    scans.check_workers(ap, a.workers)
    report, skipped = thin_scans(a.scans, a.out, a.voxel, scans.scene_list(a.scenes), a.force, a.workers, a.device)
    scans.print_outcome(report, skipped, lambda scene, e: ("thinned", scene, e["V"], "->", e["M"]), "(thinned scan exists; --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
