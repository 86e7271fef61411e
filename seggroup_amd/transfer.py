"""Labels onto another geometry of the same scene.

Pseudo labels live on the vertices they were made on.  Another geometry of the same room -- ScanNet's high-resolution `_vh_clean.ply`
beside `_vh_clean_2.ply`, the raw laser scan beside a cloud that somebody else's tool thinned, a second sensor's cloud, a thinned tree
whose `.thin.npz` was not kept -- gets them by nearest vertex: every target vertex takes the values of the source vertex that
`get_unmapper` would name for it (the best pair score, the lowest index among equals).  The search is `sg_nearest_point_grid`, the exact
grid index; `index="brute"` is `sg_nearest_point` itself, for at most 2^20 source vertices.  Carrying the values over is `thin.lift` /
`thin.lift_sgl`: a gather.

    python -m seggroup_amd.transfer --from-scans DIR --to-scans DIR -n EXP --stage S --out ROOT2 [--root .] [--scenes FILE]
                                    [--workers K] [--index {grid,brute}] [--device D]
        for every scene present in both trees: results/EXP/<scene>/<S>/ of --root (made on --from-scans) -> the same files at the
        target's V under ROOT2/results/EXP/<scene>/<S>/ (pseudo_labels.sgl and the per-vector .npy files, as `thin --lift` writes
        them), ROOT2/results/EXP/<scene>/<S>/<scene>.transfer.npz (nearest, d2) and one ROOT2/transfer_report.json

Not here: a distance cut-off that un-labels far vertices (a lifted .sgl has no "no segment" for a vertex: the report says how far the
vertices are, the decision is the user's), interpolation or voting over several neighbours, and segs.json or clicks (rekey.py and thin.py
own those).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import hip, scans
from .device import device_tensor, torch_device
from .prepare import get_unmapper, mesh_arrays, nearest_point_grid, read_ply
from .thin import lift_stage
from .thin import lift as transfer                                  # transfer(values, nearest): values[nearest] on the leading axis
from .thin import lift_sgl as transfer_sgl                           # transfer_sgl(src, dst, nearest): a .sgl for the target geometry

MAP_SUFFIX = ".transfer.npz"
REPORT_NAME = "transfer_report.json"
FAR = (0.05, 0.1, 0.5)                                               # the report counts the target vertices farther than these


def nearest_vertex(src_xyz, dst_xyz, index: str = "grid", cell=None, device=None, stream=None):
    """For every target vertex the source vertex nearest to it -> (nearest int64 [Vdst], d2 float32 [Vdst]) device tensors: nearest is
    get_unmapper(dst_xyz, src_xyz), d2 = (dx*dx + dy*dy) + dz*dz of the pair in fp32.  `index="brute"` scores every pair
    (sg_nearest_point: at most 2^20 source vertices); `cell` forces the grid's cell edge, which cannot change the result."""
    import torch
    which, edge = hip.knn_index(index), hip.knn_cell(cell)
    n_src = int(src_xyz.shape[0])
    if which == hip.KNN_BRUTE and n_src > hip.MAX_POINTS:
        raise ValueError("nearest_vertex: %d source vertices; index='brute' scores every pair and takes at most %d -- use --index grid "
                         "(index='grid')" % (n_src, hip.MAX_POINTS))
    if which == hip.KNN_GRID:
        return nearest_point_grid(dst_xyz, src_xyz, cell=edge, device=device, stream=stream)
    dev = torch_device(device)
    with torch.cuda.device(dev):
        d_src, d_dst = device_tensor(src_xyz, torch.float32, dev)[:, :3], device_tensor(dst_xyz, torch.float32, dev)[:, :3]
        nearest = get_unmapper(d_dst.contiguous(), d_src.contiguous(), device=dev)
        d = d_dst - d_src.index_select(0, nearest)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return nearest, d2


def _scan_xyz(scans_dir: str, scene: str):
    return mesh_arrays(read_ply(os.path.join(scans_dir, scene, scene + "_vh_clean_2.ply")))[0]


def transfer_scene(scene: str, from_scans: str, to_scans: str, exp: str, stage: str, out_root: str, root: str = ".", index: str = "grid",
                   device=None, stream=None):
    """One scene: results/<exp>/<scene>/<stage>/ under `root`, made on <from_scans>/<scene>, -> the same files for <to_scans>/<scene>
    under <out_root>/results/...; -> (its entry of transfer_report.json, the files written)."""
    src_dir = os.path.join(root, "results", exp, scene, stage)
    if not os.path.isdir(src_dir):
        raise FileNotFoundError(f"{src_dir}: no such export directory")
    src_xyz, dst_xyz = _scan_xyz(from_scans, scene), _scan_xyz(to_scans, scene)
    d_near, d_d2 = nearest_vertex(src_xyz, dst_xyz, index=index, device=device, stream=stream)
    nearest, d2 = d_near.cpu().numpy(), d_d2.cpu().numpy()
    dst_dir = os.path.join(out_root, "results", exp, scene, stage)
    files = lift_stage(src_dir, dst_dir, nearest, int(src_xyz.shape[0]), "transfer", "source vertices")
    np.savez(os.path.join(dst_dir, scene + MAP_SUFFIX), nearest=nearest, d2=d2)
    dist = np.sqrt(d2.astype(np.float64))
    entry = {"source_V": int(src_xyz.shape[0]), "target_V": int(dst_xyz.shape[0]), "max_distance": float(dist.max()) if dist.size else 0.0,
             "median_distance": float(np.median(dist)) if dist.size else 0.0,
             "farther_than": {"%g" % t: int((dist > t).sum()) for t in FAR}}
    return entry, files


def transfer_results(from_scans: str, to_scans: str, exp: str, stage: str, out_root: str, root: str = ".", scenes=None, workers: int = 4,
                     index: str = "grid", device=None):
    """Every scene of `from_scans` (or the named ones) that both trees hold -> (report {scene: entry}, missing {scene: why}); writes
    <out_root>/transfer_report.json.  Workers are threads, each with its own stream."""
    hip.knn_index(index)
    dev = torch_device(device)
    have_src, have_dst = set(scans.scan_names(from_scans)), set(scans.scan_names(to_scans))
    if scenes is None:
        scenes = sorted(have_src | have_dst)
    missing = {}
    todo = []
    for s in scenes:
        if s not in have_src:
            missing[s] = "no scan under --from-scans"
        elif s not in have_dst:
            missing[s] = "no scan under --to-scans"
        else:
            todo.append(s)
    report = dict(scans.map_scans(todo, workers, dev, lambda scene, stream: transfer_scene(scene, from_scans, to_scans, exp, stage, out_root, root,
                                                                                           index, device=dev, stream=stream)[0]))
    os.makedirs(out_root, exist_ok=True)
    scans.write_report(os.path.join(out_root, REPORT_NAME), {"experiment": exp, "stage": stage, "index": index, "scenes": report, "missing": missing})
    return report, missing


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.transfer", description=__doc__.split("\n\n")[0])
    ap.add_argument("--from-scans", required=True, help="the scans the results were made on (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--to-scans", required=True, help="the scans that receive them")
    ap.add_argument("-n", "--exp_name", required=True, help="name of the experiment")
    ap.add_argument("--stage", default="epoch_last", help="the export directory's name")
    ap.add_argument("--out", required=True, help="the root that receives results/ and transfer_report.json")
    ap.add_argument("--root", default=".", help="directory holding results/ (default: CWD)")
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line")
    scans.add_workers_argument(ap)
    ap.add_argument("--index", choices=sorted(hip.KNN_INDEX), default="grid", help="grid: the exact grid index; brute: every pair (at most 2^20 source vertices)")
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    try:
        report, missing = transfer_results(a.from_scans, a.to_scans, a.exp_name, a.stage, a.out, a.root, scans.scene_list(a.scenes), a.workers,
                                           a.index, a.device)
    except ValueError as e:
        if "--index grid" not in str(e):
            raise
        ap.error(str(e))
    for scene, e in report.items():
        print("transferred", scene, e["source_V"], "->", e["target_V"], "max distance %.4g" % e["max_distance"])
    for scene, why in sorted(missing.items()):
        print("skipped", scene, "(" + why + ")")
    print(f"{len(report)} scenes transferred, {len(missing)} skipped")
    return 0


if __name__ == "__main__":
    sys.exit(main())
