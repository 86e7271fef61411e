"""Labels onto another geometry of the same scene.

Pseudo labels live on the vertices they were made on.  Another geometry of the same room -- ScanNet's high-resolution `_vh_clean.ply`
beside `_vh_clean_2.ply`, the raw laser scan beside a cloud that somebody else's tool thinned, a second sensor's cloud, a thinned tree
whose `.thin.npz` was not kept -- gets them by nearest vertex: every target vertex takes the values of the source vertex that
`get_unmapper` would name for it (the best pair score, the lowest index among equals).  The search is `sg_nearest_point_grid`, the exact
grid index; `index="brute"` is `sg_nearest_point` itself, for at most 2^20 source vertices.  Carrying the values over is `thin.lift` /
`thin.lift_sgl`: a gather.

Where the source is the denser cloud, its labels are ragged at instance boundaries or the target is offset by a few millimetres, the
nearest vertex is an arbitrary member of a mixed neighbourhood.  `--vote K` takes the K nearest source vertices
(`sg_cloud_knn_cross_grid`), lets them vote on one label vector (`sg_knn_vote`: the most frequent value, the one met first among equally
frequent ones) and carries over ALL values of `rep`, the nearest source vertex that holds the winner -- so a target vertex's labels
still come from one source vertex, the .sgl stays consistent and every layer stays a function of the segment.

All of this assumes one frame.  Where the target is centimetres to decimetres off -- a photogrammetry cloud beside a laser scan, a
re-export in another pose, a rescan after a coarse manual registration -- `--align` first finds the rigid transform T that
maps the TARGET into the source's frame (`align.icp` with `--align-max-dist`, or a `<scene>.align.json` that `python -m seggroup_amd.align`
wrote), and the search runs on the moved target.  Everything after the search is unchanged: the files are written at the target's own
geometry, the distances in the report are those after alignment.

    python -m seggroup_amd.transfer --from-scans DIR --to-scans DIR -n EXP --stage S --out ROOT2 [--root .] [--scenes FILE]
                                    [--workers K] [--index {grid,brute}] [--vote {5,10,20} [--vote-on NAME]]
                                    [--align {icp,DIR} [--align-max-dist D] [--align-metric {point,plane}]
                                     [--align-init global --align-voxel H]] [--device D]
        for every scene present in both trees: results/EXP/<scene>/<S>/ of --root (made on --from-scans) -> the same files at the
        target's V under ROOT2/results/EXP/<scene>/<S>/ (pseudo_labels.sgl and the per-vector .npy files, as `thin --lift` writes
        them), ROOT2/results/EXP/<scene>/<S>/<scene>.transfer.npz (nearest, d2; with --vote also rep, votes, tied) and one
        ROOT2/transfer_report.json.  --vote-on: `seg` (the default: the .sgl's seg_of_vertex) or a vector name such as final.ins, taken
        from the .sgl's expansion or from the .npy file.  --align icp --align-max-dist D: point-to-point ICP of the target onto the source
        with the inlier radius D; --align DIR: T from DIR/<scene>.align.json.  With either the .transfer.npz also holds T (float64 [4,4],
        target -> source frame) and the scene's report entry an `align` record.  --align-metric plane (with --align icp): point-to-plane
        ICP on the SOURCE's normals -- its faces when its PLY has any, else its kNN-10 covariance --; the `align` record
        then also holds metric, normals, skipped, plane_rms_before and plane_rms_after.

Not here: a distance cut-off that un-labels far vertices (a lifted .sgl has no "no segment" for a vertex: the report says how far the
vertices are -- after the alignment, when there is one -- and the decision is the user's), interpolation or distance-weighted votes,
anything but a rigid transform between the two geometries (no scale, no deformation, no trimming or robust weights, no registration
without a starting pose: align.py says what its ICP is and is not), and segs.json or clicks (rekey.py and thin.py own those).  Every
search here is Euclidean: the nearest vertex THROUGH SPACE, which is right between two geometries of one room and wrong for spreading a
click over its own scan (a chair's label reaches the table top 5 cm away).  Distances ALONG the scan's graph, the click nearest along the
surface and the labels grown from clicks that way are seggroup_amd/geodesic.py.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import align as rigid
from . import hip, pseudo_labels, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device
from .prepare import get_unmapper, knn_cross_grid, mesh_arrays, nearest_point_grid, read_ply
from .thin import lift_stage
from .thin import lift as transfer                                  # transfer(values, nearest): values[nearest] on the leading axis
from .thin import lift_sgl as transfer_sgl                           # transfer_sgl(src, dst, nearest): a .sgl for the target geometry

MAP_SUFFIX = ".transfer.npz"
REPORT_NAME = "transfer_report.json"
FAR = (0.05, 0.1, 0.5)                                               # the report counts the target vertices farther than these
VOTE_K = (5, 10, 20)                                                 # the list lengths sg_cloud_knn_cross_grid is built for
VOTE_ON = ["seg"] + hip.LABEL_NAMES


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


def nearest_vertices(src_xyz, dst_xyz, k, cell=None, device=None, stream=None):
    """For every target vertex its k nearest source vertices, k in {5, 10, 20} -> (knn int32 [Vdst, k], d2 float32 [Vdst, k]) device
    tensors: descending pair score, the lower index first among equal scores, so knn[:, 0] is nearest_vertex's answer."""
    return knn_cross_grid(dst_xyz, src_xyz, k, cell=hip.knn_cell(cell), device=device, stream=stream, want_d2=True)


def vote(knn, labels, device=None, stream=None):
    """sg_knn_vote over the rows of knn [U, k <= 32] (indices into labels [N], any int32 values) -> (winner, rep, count, tied) int32 [U]
    device tensors: the most frequent label of the row -- the one met first among equally frequent ones --, the nearest neighbour that
    holds it, how many hold it, and whether another label is as frequent.  An index outside 0..N-1 is a ValueError."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_knn, d_lab = device_tensor(knn, torch.int32, dev), device_tensor(labels, torch.int32, dev)
        if d_knn.dim() != 2 or d_lab.dim() != 1:
            raise ValueError("vote: knn must be [U, k] and labels [N]")
        u, k = int(d_knn.shape[0]), int(d_knn.shape[1])
        out = torch.empty((4, u), dtype=torch.int32, device=dev)
        hip.check_arg(lib.sg_knn_vote(d_knn.data_ptr(), u, k, d_lab.data_ptr(), int(d_lab.shape[0]), *[out[i].data_ptr() for i in range(4)],
                                      stream_ptr(stream)))
        sync(stream)
    return out[0], out[1], out[2], out[3]


def vote_labels(src_dir: str, vote_on: str, n_src: int) -> np.ndarray:
    """The source labels the neighbours vote on -> int32 [n_src]: `seg` is the .sgl's seg_of_vertex, a vector name its expansion from the
    .sgl, or the .npy file of that name."""
    have_sgl = os.path.isfile(os.path.join(src_dir, pseudo_labels.SGL_NAME))
    if vote_on == "seg":
        if not have_sgl:
            raise ValueError(f"{src_dir}: no {pseudo_labels.SGL_NAME}, so there is no segment to vote on -- name a vector with --vote-on "
                             "(vote_on=), e.g. final.ins")
        labels = pseudo_labels.load(src_dir).seg_of_vertex
    elif vote_on not in hip.LABEL_NAMES:
        raise ValueError("--vote-on (vote_on=) must be 'seg' or one of %s, not %r" % (", ".join(hip.LABEL_NAMES), vote_on))
    else:
        lab = pseudo_labels.load(src_dir) if have_sgl else None
        if lab is not None and vote_on in lab.names:
            labels = lab.vector(vote_on)
        elif os.path.isfile(os.path.join(src_dir, vote_on + ".npy")):
            labels = np.load(os.path.join(src_dir, vote_on + ".npy"))
        else:
            raise ValueError(f"{src_dir}: --vote-on (vote_on=) {vote_on}: neither in {pseudo_labels.SGL_NAME} nor {vote_on}.npy")
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != n_src:
        raise ValueError(f"{src_dir}: --vote-on (vote_on=) {vote_on}: shape {labels.shape} for {n_src} source vertices")
    return np.ascontiguousarray(labels, dtype=np.int32)


def check_vote(vote_k, vote_on, index: str) -> None:
    """the combinations of vote, vote_on and index that are refused before anything runs (ValueError)"""
    if vote_k is None:
        if vote_on is not None:
            raise ValueError("--vote-on (vote_on=) needs --vote (vote=): without a vote there is nothing to vote on")
        return
    if vote_k not in VOTE_K:
        raise ValueError("--vote (vote=) must be one of %s, not %r" % (VOTE_K, vote_k))
    if index != "grid":
        raise ValueError("--vote (vote=) searches through the grid index only -- use --index grid (index='grid')")
    if vote_on is not None and vote_on not in VOTE_ON:
        raise ValueError("--vote-on (vote_on=) must be 'seg' or one of %s, not %r" % (", ".join(hip.LABEL_NAMES), vote_on))


ALIGN_INITS = ("global",)


def check_align(align, align_max_dist, index: str, align_metric=None, align_init=None, align_voxel=None) -> None:
    """the combinations of align, align_max_dist, align_metric, align_init, align_voxel and index that are refused before anything runs
    (ValueError)"""
    if align_init is not None:
        if align_init not in ALIGN_INITS:
            raise ValueError("--align-init (align_init=) must be 'global', not %r" % (align_init,))
        if align != "icp":
            raise ValueError("--align-init (align_init=) needs --align icp (align='icp'): a transform that is read needs no starting pose")
        if align_voxel is None or not float(align_voxel) > 0.0:
            raise ValueError("--align-init global needs --align-voxel (align_voxel=) > 0: the edge both scans are thinned at has no default")
    elif align_voxel is not None:
        raise ValueError("--align-voxel (align_voxel=) needs --align-init global (align_init='global')")
    if align_metric is not None:
        if align != "icp":
            raise ValueError("--align-metric (align_metric=) needs --align icp (align='icp'): without an ICP there is no metric to choose")
        if align_metric not in rigid.METRICS:
            raise ValueError("--align-metric (align_metric=) must be 'point' or 'plane', not %r" % (align_metric,))
    if align is None:
        if align_max_dist is not None:
            raise ValueError("--align-max-dist (align_max_dist=) needs --align icp (align='icp'): without an ICP there is no inlier radius")
        return
    if index != "grid":
        raise ValueError("--align (align=) searches through the grid index only -- use --index grid (index='grid')")
    if align == "icp":
        if align_max_dist is None or not float(align_max_dist) > 0.0:
            raise ValueError("--align icp (align='icp') needs --align-max-dist (align_max_dist=) > 0: the inlier radius has no default")
    else:
        if align_max_dist is not None:
            raise ValueError("--align-max-dist (align_max_dist=) goes with --align icp only: --align %s reads its transforms" % (align,))
        if not os.path.isdir(align):
            raise ValueError("--align (align=) must be 'icp' or a directory of <scene>%s files, not %r" % (rigid.ALIGN_SUFFIX, align))


def scene_alignment(scene: str, src_xyz, dst_xyz, align, align_max_dist, device=None, stream=None, align_metric=None, src_faces=None,
                    align_init=None, align_voxel=None):
    """-> (T float64 [4,4] mapping the target into the source's frame, the scene's `align` record of the report).  align_metric="plane":
    the source is the fixed cloud, so the normals are the source's (`src_faces`, else its kNN-10 covariance).  align_init="global": the
    ICP starts from register.global_registration of the two scans thinned at `align_voxel`; the record gains `global`."""
    init, coarse = None, {}
    if align == "icp" and align_init == "global":
        from .register import global_registration
        c = global_registration(dst_xyz, src_xyz, voxel=float(align_voxel), device=device, stream=stream)
        init, coarse = c.T, {"global": c.scalars()}
    if align == "icp" and align_metric == "plane":
        nrm, how = rigid.scan_normals(src_xyz, src_faces, device=device)
        al = rigid.icp(dst_xyz, src_xyz, align_max_dist, init=init, device=device, stream=stream, metric="plane", normals=nrm)
        return al.T, dict(al.scalars(), normals=how, source="icp", **coarse)
    if align == "icp":
        al = rigid.icp(dst_xyz, src_xyz, align_max_dist, init=init, device=device, stream=stream)
        return al.T, dict(al.scalars(), source="icp", **coarse)
    path = rigid.align_path(align, scene)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no alignment for this scene under --align (align=)")
    doc = rigid.read_align(path)
    return doc["T"], dict({k: doc.get(k) for k in rigid.SCALARS}, source=path)


def _scan_xyz(scans_dir: str, scene: str, faces: bool = False):
    xyz, _, tri = mesh_arrays(read_ply(os.path.join(scans_dir, scene, scene + "_vh_clean_2.ply")))
    return (xyz, tri) if faces else xyz


def transfer_scene(scene: str, from_scans: str, to_scans: str, exp: str, stage: str, out_root: str, root: str = ".", index: str = "grid",
                   device=None, stream=None, vote_k=None, vote_on=None, align=None, align_max_dist=None, align_metric=None, align_init=None,
                   align_voxel=None):
    """One scene: results/<exp>/<scene>/<stage>/ under `root`, made on <from_scans>/<scene>, -> the same files for <to_scans>/<scene>
    under <out_root>/results/...; -> (its entry of transfer_report.json, the files written).  With `vote_k` the files are gathered by
    `rep`, the nearest of the vote_k nearest source vertices that holds their most frequent `vote_on` label.  With `align`
    ("icp" with `align_max_dist`, or a directory of <scene>.align.json) the search runs on the target moved into the source's frame
    (DESIGN.md 8p); the files are still the target's.  `align_metric` ("point" | "plane", with align="icp"): the ICP's metric.
    `align_init="global"` with `align_voxel` (align="icp" only): the ICP starts from a global registration."""
    check_vote(vote_k, vote_on, index)
    check_align(align, align_max_dist, index, align_metric, align_init, align_voxel)
    src_dir = os.path.join(root, "results", exp, scene, stage)
    if not os.path.isdir(src_dir):
        raise FileNotFoundError(f"{src_dir}: no such export directory")
    (src_xyz, src_faces), dst_xyz = _scan_xyz(from_scans, scene, faces=True), _scan_xyz(to_scans, scene)
    dst_dir = os.path.join(out_root, "results", exp, scene, stage)
    voted, aligned, query = {}, {}, dst_xyz
    if align is not None:
        T, record = scene_alignment(scene, src_xyz, dst_xyz, align, align_max_dist, device=device, stream=stream, align_metric=align_metric,
                                    src_faces=src_faces, align_init=align_init, align_voxel=align_voxel)
        aligned, query = {"T": T}, rigid.apply(dst_xyz, T, device=device, stream=stream)
    if vote_k is None:
        d_near, d_d2 = nearest_vertex(src_xyz, query, index=index, device=device, stream=stream)
        nearest, d2 = d_near.cpu().numpy(), d_d2.cpu().numpy()
        gather = nearest
    else:
        vote_on = "seg" if vote_on is None else vote_on
        labels = vote_labels(src_dir, vote_on, int(src_xyz.shape[0]))
        d_knn, d_d2 = nearest_vertices(src_xyz, query, vote_k, device=device, stream=stream)
        _, d_rep, d_count, d_tied = vote(d_knn, labels, device=device, stream=stream)
        nearest, d2 = d_knn[:, 0].cpu().numpy().astype(np.int64), np.ascontiguousarray(d_d2[:, 0].cpu().numpy())
        gather = d_rep.cpu().numpy()
        voted = {"rep": gather, "votes": d_count.cpu().numpy(), "tied": d_tied.cpu().numpy()}
    files = lift_stage(src_dir, dst_dir, gather, int(src_xyz.shape[0]), "transfer", "source vertices")
    np.savez(os.path.join(dst_dir, scene + MAP_SUFFIX), nearest=nearest, d2=d2, **voted, **aligned)
    dist = np.sqrt(d2.astype(np.float64))
    entry = {"source_V": int(src_xyz.shape[0]), "target_V": int(dst_xyz.shape[0]), "max_distance": float(dist.max()) if dist.size else 0.0,
             "median_distance": float(np.median(dist)) if dist.size else 0.0,
             "farther_than": {"%g" % t: int((dist > t).sum()) for t in FAR}}
    if voted:
        entry.update(vote=int(vote_k), vote_on=vote_on, moved=int((gather != nearest).sum()), tied=int(voted["tied"].sum()))
    if aligned:
        entry["align"] = record
    return entry, files


def transfer_results(from_scans: str, to_scans: str, exp: str, stage: str, out_root: str, root: str = ".", scenes=None, workers: int = 4,
                     index: str = "grid", device=None, vote_k=None, vote_on=None, align=None, align_max_dist=None, align_metric=None,
                     align_init=None, align_voxel=None):
    """Every scene of `from_scans` (or the named ones) that both trees hold -> (report {scene: entry}, missing {scene: why}); writes
    <out_root>/transfer_report.json.  Workers are threads, each with its own stream.  `vote_k`, `vote_on`, `align`, `align_max_dist`,
    `align_metric`, `align_init`, `align_voxel`: transfer_scene's."""
    hip.knn_index(index)
    check_vote(vote_k, vote_on, index)
    check_align(align, align_max_dist, index, align_metric, align_init, align_voxel)
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
                                                                                           index, device=dev, stream=stream, vote_k=vote_k,
                                                                                           vote_on=vote_on, align=align,
                                                                                           align_max_dist=align_max_dist,
                                                                                           align_metric=align_metric, align_init=align_init,
                                                                                           align_voxel=align_voxel)[0]))
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
    ap.add_argument("--vote", type=int, choices=VOTE_K, default=None, metavar="K",
                    help="majority vote over the K nearest source vertices (5, 10 or 20; needs --index grid): every value comes from the nearest "
                         "of them that holds the winning label")
    ap.add_argument("--vote-on", choices=VOTE_ON, default=None, metavar="NAME",
                    help="what the neighbours vote on: seg (the default: the .sgl's seg_of_vertex) or a vector name such as final.ins")
    ap.add_argument("--align", default=None, metavar="icp|DIR",
                    help="move the target into the source's frame before the search (needs --index grid): icp fits the transform here "
                         "(with --align-max-dist), DIR reads <scene>.align.json as python -m seggroup_amd.align writes it")
    ap.add_argument("--align-max-dist", type=float, default=None, metavar="D", help="the ICP's inlier radius in the scans' unit (--align icp only)")
    ap.add_argument("--align-metric", choices=rigid.METRICS, default=None,
                    help="the ICP's metric (--align icp only): point (the default) or plane, point-to-plane on the source's normals")
    ap.add_argument("--align-init", choices=ALIGN_INITS, default=None,
                    help="where the ICP starts (--align icp only): global runs a global registration of the two scans first (with --align-voxel)")
    ap.add_argument("--align-voxel", type=float, default=None, metavar="H", help="the edge both scans are thinned at for --align-init global")
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    try:
        check_vote(a.vote, a.vote_on, a.index)
        check_align(a.align, a.align_max_dist, a.index, a.align_metric, a.align_init, a.align_voxel)
    except ValueError as e:
        ap.error(str(e))
    try:
        report, missing = transfer_results(a.from_scans, a.to_scans, a.exp_name, a.stage, a.out, a.root, scans.scene_list(a.scenes), a.workers,
                                           a.index, a.device, vote_k=a.vote, vote_on=a.vote_on, align=a.align,
                                           align_max_dist=a.align_max_dist, align_metric=a.align_metric, align_init=a.align_init,
                                           align_voxel=a.align_voxel)
    except ValueError as e:
        if "--index grid" not in str(e) and "--vote-on" not in str(e) and "max_dist" not in str(e) and "global_registration" not in str(e):
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
