"""Geodesic distances over a scan's graph on the GPU: how far a vertex is from the nearest click ALONG the surface, and
which click that is.  Every other search of the cloud tools is Euclidean, and a Euclidean nearest click spreads a chair's label onto the
table top 5 cm away; the graph -- the mesh edges, or a face-less scan's kNN / radius graph, the rows of adj.pth -- does not.

    geo    = geodesic(V, seeds, edges= | faces=, xyz= | weights=, max_dist=)   -- sg_graph_geodesic: Geodesic(dist float64 [V], owner int32 [V])
    labels = propagate(labels, owner)                                           -- labels[owner], -1 where owner < 0
    snapped, moved = snap_to_segments(seg, labels)                              -- every segment takes the label most of its vertices hold

THE RULES (include/seggroup_hip.h; tests/geodesic_ref.py restates them).  `seeds` is one whole number per vertex, a seed where it is >= 0
(a weak-label `ins` vector as it stands).  dist is what Dijkstra in double gives over the undirected graph of the rows -- lengths from
`xyz`, explicit `weights`, or hops with neither --, +inf where no seed reaches; owner is the lowest seed (its vertex index) from which
the vertex is reached over tight arcs (D(u) + w == D(v)), -1 where none.  `max_dist`: everything farther is +inf / -1.  Both are exact
and order-free: equality with the restatement is the gate, and the same bytes come back on every run.

    python -m seggroup_amd.geodesic --scans DIR --root ROOT --label_style STYLE --out DIR [--metric length|hops] [--max-dist D] [--snap]
        [--style-name NAME] [--score] [--scenes FILE --workers W --device D --force]
    Per scene it reads the PLY's coordinates, ROOT/adj/mesh/raw/<s>/<s>.adj.pth (what `prepare` writes for meshes and face-less scans
    alike) and the clicks ROOT/label/seg/<STYLE>/raw/<s>/<s>.{ins,sem}.txt (a seed where ins >= 0); every vertex takes the labels of its
    owner: the training-free baseline every pseudo-labelling result is compared against.  --snap makes the result constant on the scene's
    segments (<s>_vh_clean_2.0.010000.segs.json in the scan directory, else ROOT/label/real/raw/<s>/<s>.seg.txt) by majority.  Written:
    OUT/<scene>.geodesic.npz (dist, owner, ins, sem; with --snap ins_snapped, sem_snapped) -- `boxes --labels-from OUT --suffix
    .geodesic.npz --key ins` reads the tree as it is -- and OUT/geodesic_report.json.  --style-name NAME also writes the labels (the
    snapped ones with --snap) as ROOT/label/seg/<NAME>/raw/<s>/<s>.{ins,sem}.txt, -1 where unreached or beyond --max-dist, and the
    resampled label.pth where the scene's map.pth exists: the clicks grown to a geodesic radius, for `infer` / `train --label_style
    NAME`.  --score reads ROOT/label/real/raw/<s>/<s>.{ins,sem}.txt and reports through evaluate.eval_vectors and evaluate.ap_vectors
    with the labels as layer `final`: the numbers `evaluate` and `evaluate --ap` print for such labels.  A scene whose .npz OUT holds
    already is skipped without --force.

Not here: exact polyhedral geodesics across faces (this is the graph metric of the scan's edges), path extraction (predecessors), a
label gate on edges, weights from colour or normals, a results/<exp> tree or .sgl files, graphs of more than 2^26 rows.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import sys
from typing import NamedTuple

import numpy as np

from . import hip, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_EDGES = 1 << 26
TILE = 256                             # kTile of csrc/kernels_geodesic.hip, the vertices a workgroup of k_gd_relax owns: the tests sit either side
                                       # of it, and tests/test_geodesic_ref.py reads the kernel file to hold the two together
METRICS = ("length", "hops")
NPZ_SUFFIX = ".geodesic.npz"
REPORT_NAME = "geodesic_report.json"
STAT_NAMES = ("arcs", "distance_launches", "owner_launches", "tight_arcs", "reached")


class Geodesic(NamedTuple):
    """geodesic's result: `dist` float64 [V] (+inf where no seed reaches), `owner` int32 [V] (the owning seed's vertex index, -1 where none)"""
    dist: np.ndarray
    owner: np.ndarray


def _whole(a, who: str, what: str, shape_text: str, cols=None) -> np.ndarray:
    if hasattr(a, "cpu") and hasattr(a, "numpy"):
        a = a.cpu().numpy()
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_:
        raise ValueError("%s: %s holds whole numbers, %s, not %s" % (who, what, shape_text, a.dtype))
    if (a.ndim != 1) if cols is None else (a.ndim != 2 or a.shape[1] != cols):
        raise ValueError("%s: %s is %s, not %r" % (who, what, shape_text, a.shape))
    if a.size and (int(a.max()) > 0x7fffffff or int(a.min()) < -0x80000000):
        raise ValueError("%s: %s holds a value outside int32" % (who, what))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_max_dist(max_dist) -> float:
    """None -> +inf; else a number >= 0 that is not NaN"""
    if max_dist is None:
        return math.inf
    if isinstance(max_dist, (bool, str)) or not isinstance(max_dist, (int, float, np.integer, np.floating)) or not float(max_dist) >= 0.0:
        raise ValueError("max_dist (max_dist=, --max-dist) is a length >= 0, or None for no limit, not %r" % (max_dist,))
    return float(max_dist)


def check_graph(V, seeds, edges=None, faces=None, xyz=None, weights=None, max_dist=None):
    """every refusal of `geodesic` about shape, dtype, exclusivity or limits (ValueError), before any device call
    -> (V, seeds int32 [V], rows int32 [E,2] or [F,3], is_faces, weights float64 [E] or None, limit)"""
    who = "geodesic"
    if isinstance(V, bool) or not isinstance(V, (int, np.integer)) or V < 1:
        raise ValueError("%s: V is the number of vertices, a whole number >= 1, not %r" % (who, V))
    V = int(V)
    if V > hip.MAX_CLOUD_POINTS:
        raise ValueError("%s: %d vertices; a graph holds at most 2^27" % (who, V))
    seeds = _whole(seeds, who, "seeds", "one per vertex, [%d]" % V)
    if seeds.shape[0] != V:
        raise ValueError("%s: seeds is one per vertex, [%d], not %r" % (who, V, seeds.shape))
    if (edges is None) == (faces is None):
        raise ValueError("%s: exactly one of edges= ([E,2]) and faces= ([F,3]) is needed" % who)
    is_faces = faces is not None
    rows = _whole(faces, who, "faces", "[F,3]", 3) if is_faces else _whole(edges, who, "edges", "[E,2]", 2)
    if rows.shape[0] * (3 if is_faces else 1) > MAX_EDGES:
        raise ValueError("%s: %d edge rows; a call takes at most 2^26" % (who, rows.shape[0] * (3 if is_faces else 1)))
    if xyz is not None and weights is not None:
        raise ValueError("%s: xyz= (lengths) and weights= are two metrics; give at most one" % who)
    if weights is not None:
        if is_faces:
            raise ValueError("%s: weights= goes with edges= (one per row); faces= takes xyz= or hops" % who)
        weights = np.asarray(weights)
        if weights.shape != (rows.shape[0],) or not (np.issubdtype(weights.dtype, np.floating) or np.issubdtype(weights.dtype, np.integer)):
            raise ValueError("%s: weights holds one number per edge row, [%d], not %s %r" % (who, rows.shape[0], weights.dtype, weights.shape))
        weights = np.ascontiguousarray(weights, dtype=np.float64)
    if xyz is not None:
        shape = tuple(xyz.shape) if hasattr(xyz, "shape") else np.shape(xyz)
        if len(shape) != 2 or shape[1] < 3 or shape[0] != V:
            raise ValueError("%s: xyz is [V, >= 3] rows with xyz first, [%d, >= 3], not %r" % (who, V, shape))
    return V, seeds, rows, is_faces, weights, check_max_dist(max_dist)


def last_stats() -> dict:
    """sg_graph_geodesic_stats: the calling thread's last call -> {arcs, distance_launches, owner_launches, tight_arcs, reached}; the launch
    counts are launches enqueued, whole batches of 8"""
    h = (C.c_int64 * len(STAT_NAMES))()
    hip.check(hip.lib().sg_graph_geodesic_stats(h, len(STAT_NAMES)))
    return dict(zip(STAT_NAMES, (int(v) for v in h)))


def geodesic(V, seeds, *, edges=None, faces=None, xyz=None, weights=None, max_dist=None, device=None, stream=None) -> Geodesic:
    """sg_graph_geodesic.  `seeds` [V] whole numbers (a seed where >= 0); exactly one of `edges` [E,2] and `faces` [F,3] (their three
    sides, made on the device); `xyz` [V, >= 3] (array or tensor, float32: other types are CONVERTED to float32 first, and the lengths are
    those of the converted coordinates) or `weights` [E] (with `edges` only) or neither (hops);
    `max_dist` None or a length >= 0.  -> Geodesic of NumPy arrays.  An index outside 0..V-1, a bad weight and a coordinate of an
    edge's end that is not finite are the library's ValueError."""
    V, seeds, rows, is_faces, weights, limit = check_graph(V, seeds, edges, faces, xyz, weights, max_dist)
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_rows = device_tensor(rows, torch.int32, dev)
        if is_faces:
            d_rows = torch.cat([d_rows[:, [0, 1]], d_rows[:, [1, 2]], d_rows[:, [0, 2]]]).contiguous()
        E = int(d_rows.shape[0])
        d_seed = device_tensor(seeds, torch.int32, dev)
        d_xyz = None if xyz is None else device_tensor(xyz, torch.float32, dev)
        d_w = None if weights is None else device_tensor(weights if E else np.zeros(1), torch.float64, dev)
        d_dist = torch.empty(V, dtype=torch.float64, device=dev)
        d_owner = torch.empty(V, dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_graph_geodesic_ws_bytes(V, E), dev)
        hip.check_arg(lib.sg_graph_geodesic(d_rows.data_ptr() if E else None, E, V, hip.ptr(d_xyz), int(d_xyz.shape[1]) if d_xyz is not None else 0,
                                            hip.ptr(d_w), d_seed.data_ptr(), limit, d_dist.data_ptr(), d_owner.data_ptr(), ws.data_ptr(), ws.numel(),
                                            stream_ptr(stream)))
        sync(stream)
        return Geodesic(d_dist.cpu().numpy(), d_owner.cpu().numpy())


def propagate(labels, owner) -> np.ndarray:
    """labels[owner], -1 where owner < 0: every vertex takes what its owning seed holds"""
    labels, owner = np.asarray(labels), np.asarray(owner)
    if labels.ndim != 1 or owner.shape != labels.shape or not np.issubdtype(owner.dtype, np.integer):
        raise ValueError("propagate: labels and owner hold one value per vertex, not %r and %s %r" % (labels.shape, owner.dtype, owner.shape))
    if owner.size and int(owner.max()) >= labels.shape[0]:
        raise ValueError("propagate: an owner outside the %d vertices" % labels.shape[0])
    return np.where(owner >= 0, labels[np.maximum(owner, 0)], -1).astype(labels.dtype)


def label_columns(labels):
    """-> (cols int32 [V], values int64 [K]): the labels >= 0 ranked to the columns 0..K-1 in ascending order -- a tie of a vote goes to
    the lowest column, so to the lowest label --, everything negative (unreached) to the column K of its own"""
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("snap_to_segments: labels is one whole number per vertex, not %s %r" % (labels.dtype, labels.shape))
    values = np.unique(labels[labels >= 0]).astype(np.int64)
    cols = np.where(labels >= 0, np.searchsorted(values, labels), values.shape[0]).astype(np.int32)
    return cols, values


def snapped_labels(seg, labels, values, row_ids, winner):
    """a vote's rows -> (the segment-constant vector, the share of vertices whose label moved)"""
    seg, labels = np.asarray(seg).reshape(-1), np.asarray(labels)
    table = np.concatenate([np.asarray(values, np.int64), [-1]])             # the unreached column is the last
    out = table[np.asarray(winner, np.int64)][np.searchsorted(np.asarray(row_ids), seg)].astype(labels.dtype)
    return out, (float((out != labels).mean()) if labels.size else 0.0)


def snap_to_segments(seg, labels, device=None, stream=None):
    """Every segment takes the label most of its vertices hold (rekey.vote: ties to the lowest label, unreached a column of its own,
    the last) -> (the segment-constant vector, the share of vertices that moved)."""
    from . import rekey
    seg = _whole(seg, "snap_to_segments", "seg", "one per vertex")
    cols, values = label_columns(labels)
    if seg.shape != cols.shape:
        raise ValueError("snap_to_segments: %d segment ids for %d labels" % (seg.shape[0], cols.shape[0]))
    v = rekey.vote(seg, cols, int(values.shape[0]) + 1, device=device, stream=stream).host()
    return snapped_labels(seg, labels, values, v.row_ids, v.winner)


# ---- scans ------------------------------------------------------------------------------------------------------------------------------------
def check_command(label_style, metric, max_dist, snap, style_name, score) -> dict:
    """the combinations of the command's options that are refused before anything runs (ValueError) -> the parameters in force"""
    for name, s in (("--label_style", label_style), ("--style-name", style_name)):
        if s is not None and (not s or s in (".", "..") or os.sep in s or "/" in s):
            raise ValueError("%s is the name of one directory under label/seg, not %r" % (name, s))
    if label_style is None:
        raise ValueError("--label_style is needed: the clicks are label/seg/<STYLE>/raw/<scene>/<scene>.{ins,sem}.txt")
    metric = METRICS[0] if metric is None else metric
    if metric not in METRICS:
        raise ValueError("--metric is %s, not %r" % (" or ".join(METRICS), metric))
    if style_name is not None and style_name == label_style:
        raise ValueError("--style-name %s is --label_style: the style written is another one than the clicks read" % style_name)
    limit = check_max_dist(max_dist)
    return dict(label_style=label_style, metric=metric, max_dist=None if math.isinf(limit) else limit, snap=bool(snap), style_name=style_name,
                score=bool(score))


def scene_files(scene_path: str, root: str, p: dict) -> dict:
    """the files of one scene the command reads; one that is missing is a ValueError that names it"""
    scene = scans.scene_name(scene_path)
    style = os.path.join(root, "label", "seg", p["label_style"], "raw", scene)
    real = os.path.join(root, "label", "real", "raw", scene)
    f = dict(ply=os.path.join(scene_path, scene + scans.PLY_SUFFIX), adj=os.path.join(root, "adj", "mesh", "raw", scene, scene + ".adj.pth"),
             ins=os.path.join(style, scene + ".ins.txt"), sem=os.path.join(style, scene + ".sem.txt"))
    if not os.path.exists(f["adj"]):
        raise ValueError("%s: %s is missing: `python -m seggroup_amd.prepare` writes the scan's graph" % (scene, f["adj"]))
    for k in ("ply", "ins", "sem"):
        if not os.path.exists(f[k]):
            raise ValueError("%s: %s is missing" % (scene, f[k]))
    if p["snap"]:
        cands = [os.path.join(scene_path, scene + "_vh_clean_2.0.010000.segs.json"), os.path.join(real, scene + ".seg.txt")]
        found = [c for c in cands if os.path.exists(c)]
        if not found:
            raise ValueError("%s: --snap needs the scene's segments: neither %s nor %s is there" % (scene, cands[0], cands[1]))
        f["seg"] = found[0]
    if p["score"]:
        f["real_ins"], f["real_sem"] = os.path.join(real, scene + ".ins.txt"), os.path.join(real, scene + ".sem.txt")
        for k in ("real_ins", "real_sem"):
            if not os.path.exists(f[k]):
                raise ValueError("%s: --score needs %s" % (scene, f[k]))
    return f


def _vector(path: str, n: int, scene: str) -> np.ndarray:
    from . import labels
    v = np.array(labels.load_labels(path), dtype=np.int64)
    if v.shape[0] != n:
        raise ValueError("%s: %s holds %d values for %d vertices" % (scene, path, v.shape[0], n))
    return v


def geodesic_scan(scene_path: str, root: str, out_dir: str, p: dict, force: bool = False, device=None, stream=None):
    """One scan directory -> OUT/<scene>.geodesic.npz (and the label files of --style-name) -> its entry of geodesic_report.json with the
    score matrices under "_score" when asked for, or None when the .npz was there already (never overwritten without `force`)."""
    from . import labels
    from .prepare import mesh_arrays, read_ply
    from .pth import load_tensor
    scene = scans.scene_name(scene_path)
    out = os.path.join(out_dir, scene + NPZ_SUFFIX)
    if os.path.exists(out) and not force:
        return None
    f = scene_files(scene_path, root, p)
    xyz = mesh_arrays(read_ply(f["ply"]))[0]
    n = int(xyz.shape[0])
    adj = np.asarray(load_tensor(f["adj"]))
    if adj.ndim != 2 or adj.shape[1] != 2:
        raise ValueError("%s: %s holds %r, not [E,2] rows" % (scene, f["adj"], adj.shape))
    ins_weak, sem_weak = _vector(f["ins"], n, scene), _vector(f["sem"], n, scene)
    geo = geodesic(n, ins_weak, edges=adj, xyz=xyz if p["metric"] == "length" else None, max_dist=p["max_dist"], device=device, stream=stream)
    stats = last_stats()
    ins, sem = propagate(ins_weak, geo.owner), propagate(sem_weak, geo.owner)
    arrays = dict(dist=geo.dist, owner=geo.owner, ins=ins.astype(np.int32), sem=sem.astype(np.int32))
    finite = geo.dist[np.isfinite(geo.dist)]
    entry = dict(vertices=n, seeds=int((ins_weak >= 0).sum()), reached=int((geo.owner >= 0).sum()), unreached=int((geo.owner < 0).sum()),
                 largest_distance=float(finite.max()) if finite.size else None, distance_launches=stats["distance_launches"],
                 owner_launches=stats["owner_launches"])
    final_ins, final_sem = ins, sem
    if p["snap"]:
        seg = np.asarray(labels.load_labels(f["seg"]), dtype=np.int64)
        if seg.shape[0] != n:
            raise ValueError("%s: %s holds %d segment ids for %d vertices" % (scene, f["seg"], seg.shape[0], n))
        final_ins, entry["moved"] = snap_to_segments(seg, ins, device=device, stream=stream)
        final_sem, _ = snap_to_segments(seg, sem, device=device, stream=stream)
        arrays.update(ins_snapped=final_ins.astype(np.int32), sem_snapped=final_sem.astype(np.int32))
    os.makedirs(out_dir, exist_ok=True)
    np.savez(out, **arrays)
    if p["style_name"] is not None:
        raw = os.path.join(root, "label", "seg", p["style_name"], "raw", scene)
        labels._write_txt(os.path.join(raw, scene + ".ins.txt"), final_ins)
        labels._write_txt(os.path.join(raw, scene + ".sem.txt"), final_sem)
        if os.path.exists(os.path.join(root, "data", "resampled", scene, scene + ".map.pth")):
            labels.generate_weak_label_pth(scene, p["style_name"], root)
            entry["resampled"] = "written"
        else:
            entry["resampled"] = "not written: no data/resampled/%s/%s.map.pth under the root" % (scene, scene)
    if p["score"]:
        from . import evaluate
        import torch
        dev = torch_device(device)
        gt = np.stack([_vector(f["real_sem"], n, scene), _vector(f["real_ins"], n, scene)], 1).astype(np.int32)
        lab = {"final": (np.ascontiguousarray(final_ins, dtype=np.int32), np.ascontiguousarray(final_sem, dtype=np.int32))}
        with torch.cuda.device(dev), on_stream(stream):
            m = evaluate.eval_vectors(gt, lab, ["final"], dev)
            match = evaluate.ap_vectors(gt, lab, ["final"], dev)[0]
            sync(stream)
        entry["accuracy"] = dict(zip(("sem", "ins", "sem_selected", "ins_selected"), (float(x) for x in m[0, 160:164])))
        entry["_score"] = (m, match)
    return entry


def geodesic_scans(scans_dir: str, root: str, out_dir: str, scenes=None, workers: int = 4, device=None, force: bool = False, **options):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names, the score or None);
    writes OUT/geodesic_report.json.  The files of every scene are looked for, and a missing one refused, before a device call."""
    p = check_command(options.get("label_style"), options.get("metric"), options.get("max_dist"), options.get("snap"), options.get("style_name"),
                      options.get("score"))
    names = scans.scan_names(scans_dir) if scenes is None else list(scenes)
    skipped = [s for s in names if os.path.exists(os.path.join(out_dir, s + NPZ_SUFFIX)) and not force]
    todo = [s for s in names if s not in skipped]
    for s in todo:
        scene_files(os.path.join(scans_dir, s), root, p)
    report = {}
    if todo:                                                                 # a run that skips every scene needs no device
        dev = torch_device(device)
        done = scans.map_scans(todo, workers, dev, lambda s, stream: geodesic_scan(os.path.join(scans_dir, s), root, out_dir, p, True, dev, stream))
        report = dict(done)
    scored = [e.pop("_score") for e in report.values() if "_score" in e]
    doc = {"parameters": {k: v for k, v in p.items() if v is not None}, "scenes": report, "skipped": skipped}
    score = None
    if p["score"] and scored:
        from . import ap, evaluate
        accs = evaluate.accumulate([m for m, _ in scored], ["final"])
        ap_acc = ap.APAccumulator()
        for _, match in scored:
            ap_acc.add(match)
        score = (accs, {"final": ap_acc})
        doc["score"] = {"v": accs["final"].v.tolist(), "scenes": len(scored), "ap": ap.to_json(ap.compute_averages(ap_acc.ap()))}
    os.makedirs(out_dir, exist_ok=True)
    scans.write_report(os.path.join(out_dir, REPORT_NAME), doc)
    return report, skipped, score


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.geodesic", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--root", required=True, help="the dataset root: adj/mesh/raw and label/seg/<STYLE>/raw are read")
    ap.add_argument("--label_style", default=None, metavar="STYLE", help="the clicks: label/seg/<STYLE>/raw/<s>/<s>.{ins,sem}.txt, a seed where ins >= 0")
    ap.add_argument("--out", required=True, metavar="DIR", help="where <scene>.geodesic.npz and geodesic_report.json go")
    ap.add_argument("--metric", default=None, help="length (default: the edges' lengths) or hops")
    ap.add_argument("--max-dist", type=float, default=None, metavar="D", help="vertices farther from every click stay unlabelled")
    ap.add_argument("--snap", action="store_true", help="make the labels constant on the scene's segments, by majority")
    ap.add_argument("--style-name", default=None, metavar="NAME", help="also write the labels as the label style label/seg/<NAME>")
    ap.add_argument("--score", action="store_true", help="score the labels against label/real/raw as `evaluate` and `evaluate --ap` would")
    scans.add_batch_arguments(ap, "overwrite the files of a scene that OUT holds already")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    options = dict(label_style=a.label_style, metric=a.metric, max_dist=a.max_dist, snap=a.snap, style_name=a.style_name, score=a.score)
    np.seterr(divide="ignore", invalid="ignore")
    try:
        check_command(*(options[k] for k in ("label_style", "metric", "max_dist", "snap", "style_name", "score")))
        report, skipped, score = geodesic_scans(a.scans, a.root, a.out, scans.scene_list(a.scenes), a.workers, a.device, a.force, **options)
    except ValueError as e:
        ap.error(str(e))
    scans.print_outcome(report, skipped, lambda scene, e: ("geodesic", scene, e["vertices"], "vertices,", e["seeds"], "seeds,", e["reached"], "reached,",
                                                           e["distance_launches"], "+", e["owner_launches"], "launches"),
                        "(its .geodesic.npz is in --out: --force overwrites)")
    if score is not None:
        from . import evaluate
        evaluate.report_ap(score[0], score[1], "geodesic:" + a.label_style, a.out, False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
