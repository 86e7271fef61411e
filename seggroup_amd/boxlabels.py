"""Weak labels from 3D boxes on the GPU: the way back from boxes to points.  Which boxes hold this vertex -- and so boxes,
a detector's, an annotator's or the ground truth's own as a simulated annotator, become seed labels for the pipeline: a vertex inside
exactly one box almost surely belongs to that instance, and a segment whose vertices all do is a click nobody had to make.

    rows  = box_frames(boxes)                              -- float64 [K,15] = cx cy cz sx sy sz r00 .. r22 of a Boxes of ANY kind (the
                                                              test needs no upright box), of [K,15], [K,8] or [K,7] rows; the row
                                                              layouts, the box files and the limits of a call are seggroup_amd/boxset.py's
    pib   = points_in_boxes(xyz, boxes, margin)            -- sg_points_in_boxes: per point count (boxes that hold it), first (the lowest
                                                              such box) and inner (the one of smallest volume), -1 where none
    owner = vertex_owner(pib, K, overlap)                  -- one code per vertex: 0 no box, 1 + k box k only; in several boxes K + 1
                                                              ("several", overlap="skip") or 1 + inner (overlap="inner")
    sb    = segment_boxes(seg, owner, K, purity)           -- rekey.vote over the codes: a segment takes box k when its winner is 1 + k, it
                                                              is not tied and winner_count >= purity * row_count
    ins, sem, report = weak_labels(xyz, seg, boxes, ids, sem, margin, purity, overlap)

    python -m seggroup_amd.boxlabels --scans DIR --root ROOT
        ( --from-real [--kind aabb|yaw|pca] [--angles A] [--min-points M]
        | --boxes DIR [--suffix .boxes.npz|_bbox.npy] )
        [--margin M] [--purity P] [--overlap skip|inner] [--style-name box] [--scenes FILE --workers W --device D --force]
    Vertices are the scan PLY's, segments <scene>_vh_clean_2.0.010000.segs.json, as `labels.generate_weak_labels` reads them for
    `manual`.  --from-real simulates the annotator: the boxes are boxes.label_boxes of ROOT/label/real/raw/<s>/<s>.ins.txt (ins == 0
    ignored, --min-points defaults to 1), ids the instance values, the class is the .sem.txt value at each instance's first vertex, and
    the report gains `agree`, the labelled vertices whose real instance is the label they got.  --boxes reads DIR/<scene>.boxes.npz
    (it needs `sem`; ids = `values` where the file has them, else 1 + k) or DIR/<scene>_bbox.npy ([K,7], ids = 1 + k).  Written:
    ROOT/label/seg/<style-name>/raw/<s>/<s>.{ins,sem}.txt, <s>.boxlabels.npz beside them (count, first, inner, owner, the segment
    table), ROOT/label/seg/<style-name>/boxlabels_report.json, and -- where ROOT/data/resampled/<s>/<s>.map.pth exists -- the resampled
    label.pth through labels.generate_weak_label_pth; `infer` and `train` then take --label_style <style-name>.

Not here: a spatial index over the boxes (brute force), refining the labels inside a box, IoU of tilted boxes, scene packs for a dataset
without label/real; non-maximum suppression -- a detector's overlapping proposals leave every vertex "in several boxes" -- is
seggroup_amd/boxnms.py, whose filtered tree --boxes reads as it is.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import NamedTuple

import numpy as np

from . import boxset, hip, scans
from .boxset import box_frames                                                # the layout of every row this module sends to the device
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_POINTS = 1 << 24
OVERLAPS = ("skip", "inner")
NPZ_SUFFIX = ".boxlabels.npz"
REPORT_NAME = "boxlabels_report.json"
DEFAULT_STYLE = "box"


class PointsInBoxes(NamedTuple):
    """points_in_boxes' result, int32 device tensors [N]: `count`, `first`, `inner` (indices within the scene's boxes, -1 where no box
    holds the point); `held` int32 [K], points per box, or None when it was not asked for"""
    count: object
    first: object
    inner: object
    held: object = None


class SegmentBoxes(NamedTuple):
    """segment_boxes' result, host arrays, rows in ascending segment id: `seg_ids`, `box` (-1: the segment took none), `votes` (the
    winner's vertices) and `size` (the segment's vertices)"""
    seg_ids: np.ndarray
    box: np.ndarray
    votes: np.ndarray
    size: np.ndarray


def check_margin(margin) -> float:
    if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)) or not math.isfinite(margin) or margin < 0:
        raise ValueError("margin (margin=, --margin) is a finite length >= 0, not %r" % (margin,))
    return float(margin)


def check_purity(purity) -> float:
    if isinstance(purity, bool) or not isinstance(purity, (int, float, np.integer, np.floating)) or not 0.5 < purity <= 1.0:
        raise ValueError("purity (purity=, --purity) lies in (0.5, 1], not %r" % (purity,))
    return float(purity)


def check_overlap(overlap) -> str:
    if overlap not in OVERLAPS:
        raise ValueError("overlap (overlap=, --overlap) is one of %s, not %r" % (", ".join(OVERLAPS), overlap))
    return overlap


def points_in_boxes(xyz, boxes, margin=0.0, off_points=None, off_boxes=None, device=None, stream=None, held: bool = False) -> PointsInBoxes:
    """sg_points_in_boxes: `xyz` [N, >= 3] (array or tensor, float32 on the device), `boxes` anything box_frames takes -> PointsInBoxes of
    device tensors.  `off_points` / `off_boxes` ([B+1] each, both or neither) delimit scenes: only points and boxes of one scene meet,
    and first / inner count within the scene's boxes.  `held`: also the points per box.  Every refusal about shape or kind comes before
    any device call."""
    rows = box_frames(boxes)
    margin = check_margin(margin)
    shape = tuple(xyz.shape) if hasattr(xyz, "shape") else np.shape(xyz)
    if len(shape) != 2 or shape[1] < 3:
        raise ValueError("points_in_boxes: a cloud is [N, >= 3] rows with xyz first, not %r" % (shape,))
    n, k = int(shape[0]), int(rows.shape[0])
    if n > MAX_POINTS or k > boxset.MAX_BOXES:
        raise hip.SgError(hip.SG_EUNSUP, "points_in_boxes: %d points and %d boxes; a call takes at most 2^24 points and 2^20 boxes" % (n, k))
    op, ob = boxset.paired_offsets("points_in_boxes", (off_points, n, "off_points", "points"), (off_boxes, k, "off_boxes", "boxes"))
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    scenes = int(op.shape[0]) - 1
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_tensor(xyz, torch.float32, dev)
        d_box = device_tensor(rows, torch.float64, dev)
        out = torch.empty((3, max(n, 1)), dtype=torch.int32, device=dev)
        d_held = torch.empty(max(k, 1), dtype=torch.int32, device=dev) if held else None
        ws = workspace(lib.sg_points_in_boxes_ws_bytes(n, k, scenes), dev)
        hip.check_arg(lib.sg_points_in_boxes(d_xyz.data_ptr() if n else None, int(shape[1]), n, d_box.data_ptr() if k else None, k, op.ctypes.data,
                                             ob.ctypes.data, scenes, margin, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                             hip.ptr(d_held), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return PointsInBoxes(out[0, :n], out[1, :n], out[2, :n], d_held[:k] if held else None)


def vertex_owner(pib: PointsInBoxes, K: int, overlap: str = "skip"):
    """-> int32 [N], on the device the counts are on: 0 in no box, 1 + k in box k only; where count > 1, K + 1 ("several") under `skip`
    and 1 + inner under `inner` -- the chair under the table goes to the chair."""
    import torch
    check_overlap(overlap)
    count, first, inner = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t)) for t in (pib.count, pib.first, pib.inner))
    several = torch.full_like(first, int(K) + 1) if overlap == "skip" else inner + 1
    owner = torch.where(count == 1, first + 1, several)
    return torch.where(count == 0, torch.zeros_like(owner), owner).to(torch.int32)


def segment_rule(winner, winner_count, row_count, tied, K: int, purity: float = 1.0) -> np.ndarray:
    """the rule of segment_boxes on a vote's rows (host arrays) -> int32 box per row, -1 where the segment takes none"""
    purity = check_purity(purity)
    winner, votes, size = np.asarray(winner).astype(np.int64), np.asarray(winner_count), np.asarray(row_count)
    ok = (winner >= 1) & (winner <= int(K)) & (np.asarray(tied) == 0) & (votes.astype(np.float64) >= purity * size.astype(np.float64))
    return np.where(ok, winner - 1, -1).astype(np.int32)


def segment_boxes(seg, owner, K: int, purity: float = 1.0, device=None, stream=None) -> SegmentBoxes:
    """rekey.vote(seg, owner, K + 2) and the rule: segment s takes box k when its winner is the code 1 + k, it is not tied and
    float64(winner_count) >= purity * float64(row_count); otherwise -1.  `purity` lies in (0.5, 1]."""
    from . import rekey
    purity = check_purity(purity)
    v = rekey.vote(seg, owner, int(K) + 2, device=device, stream=stream).host()
    return SegmentBoxes(v.row_ids, segment_rule(v.winner, v.winner_count, v.row_count, v.tied, K, purity), v.winner_count, v.row_count)


def _box_labels(values, k: int, what: str) -> np.ndarray:
    v = np.asarray(values)
    if v.shape != (k,) or not np.issubdtype(v.dtype, np.integer):
        raise ValueError("weak_labels: %s is one whole number per box, [%d]" % (what, k))
    if k and int(v.min()) < 1:
        raise ValueError("weak_labels: %s must be >= 1 (the label files count from 1 and -1 is \"no label\"), not %d" % (what, int(v.min())))
    return v.astype(np.int64)


def weak_labels(xyz, seg, boxes, ids, sem, margin=0.0, purity=1.0, overlap="skip", device=None, stream=None, detail: bool = False):
    """-> (ins_weak, sem_weak int64 [V], report): every vertex of a segment that took box k gets ids[k] / sem[k], every other vertex -1
    -- the content of the .ins.txt / .sem.txt pair.  `ids`, `sem` [K] are >= 1.  report: per box `inside` (vertices it holds), `owned`
    (vertices whose owner code it is), `segments` and `vertices` (what took it); the scene's `labelled`, `several` (vertices in more
    than one box) and `boxes_without_segment`.  With `detail` the report also carries the arrays of <scene>.boxlabels.npz under
    "arrays"."""
    rows = box_frames(boxes)
    k = int(rows.shape[0])
    ids, sem = _box_labels(ids, k, "ids"), _box_labels(sem, k, "sem")
    margin, purity, overlap = check_margin(margin), check_purity(purity), check_overlap(overlap)
    seg = np.asarray(seg).reshape(-1)
    shape = tuple(xyz.shape) if hasattr(xyz, "shape") else np.shape(xyz)
    if len(shape) != 2 or shape[0] != seg.shape[0] or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError("weak_labels: seg is one whole number per vertex, [%d], not %s %r" % (shape[0] if shape else 0, seg.dtype, seg.shape))
    import torch
    dev = torch_device(device)
    pib = points_in_boxes(xyz, rows, margin, device=dev, stream=stream, held=True)
    with torch.cuda.device(dev), on_stream(stream):
        owner = vertex_owner(pib, k, overlap)
    sb = segment_boxes(seg, owner, k, purity, device=dev, stream=stream)
    with torch.cuda.device(dev), on_stream(stream):
        h_owner, h_count, h_held = owner.cpu().numpy(), pib.count.cpu().numpy(), pib.held.cpu().numpy()
    vbox = sb.box[np.searchsorted(sb.seg_ids, seg)].astype(np.int64)           # every id of seg is a row of the vote
    hit = vbox >= 0
    ins_weak = np.where(hit, ids[np.maximum(vbox, 0)] if k else -1, -1).astype(np.int64)
    sem_weak = np.where(hit, sem[np.maximum(vbox, 0)] if k else -1, -1).astype(np.int64)
    owned = np.bincount(h_owner[(h_owner >= 1) & (h_owner <= k)] - 1, minlength=k)[:k]
    segments = np.bincount(sb.box[sb.box >= 0], minlength=k)[:k]
    vertices = np.bincount(vbox[hit], minlength=k)[:k]
    report = {"boxes": [{"inside": int(h_held[j]), "owned": int(owned[j]), "segments": int(segments[j]), "vertices": int(vertices[j])} for j in range(k)],
              "labelled": int(hit.sum()), "several": int((h_count > 1).sum()), "boxes_without_segment": int((segments == 0).sum())}
    if detail:
        with torch.cuda.device(dev), on_stream(stream):
            report["arrays"] = dict(count=h_count, first=pib.first.cpu().numpy(), inner=pib.inner.cpu().numpy(), owner=h_owner, seg_ids=sb.seg_ids,
                                    seg_box=sb.box, seg_votes=sb.votes, seg_size=sb.size)
    return ins_weak, sem_weak, report


# ---- scans ------------------------------------------------------------------------------------------------------------------------------------
def check_command(from_real, boxes_dir, suffix, kind, angles, min_points, margin, purity, overlap, style_name) -> dict:
    """the combinations of the command's options that are refused before anything runs (ValueError) -> the parameters in force"""
    from . import boxes
    if bool(from_real) == (boxes_dir is not None):
        raise ValueError("exactly one source of boxes is needed: --from-real or --boxes DIR")
    style = DEFAULT_STYLE if style_name is None else style_name
    if not style or style in (".", "..") or os.sep in style or "/" in style:
        raise ValueError("--style-name is the name of one directory under label/seg, not %r" % (style_name,))
    p = dict(margin=check_margin(0.0 if margin is None else margin), purity=check_purity(1.0 if purity is None else purity),
             overlap=check_overlap("skip" if overlap is None else overlap), style_name=style)
    if from_real:
        if suffix is not None:
            raise ValueError("--suffix belongs to --boxes DIR")
        kind, a, min_points = boxes.check_box_parameters("aabb" if kind is None else kind, angles, 1 if min_points is None else min_points)
        return dict(p, from_real=True, kind=kind, angles=a, min_points=min_points)
    if kind is not None or angles is not None or min_points is not None:
        raise ValueError("--kind, --angles and --min-points belong to --from-real: the files of --boxes are made already")
    suffix = boxset.SUFFIXES[0] if suffix is None else suffix
    if suffix not in boxset.SUFFIXES:
        raise ValueError("--suffix is %s, not %r" % (" or ".join(boxset.SUFFIXES), suffix))
    return dict(p, boxes=boxes_dir, suffix=suffix)


def file_scenes(scans_dir: str, boxes_dir: str, suffix: str, scenes=None) -> list:
    """the scenes that have a scan and a box file; one that is on one side only is a ValueError that names it"""
    return boxset.listed_scenes([("scan under --scans", set(scans.scan_names(scans_dir))),
                                 ("{}%s under --boxes" % suffix, boxset.scene_files(boxes_dir, suffix))], scenes)


def file_boxes(path: str):
    """<scene>.boxes.npz (it needs `sem`; a box of kind pca is taken) or <scene>_bbox.npy ([K,7]) -> (rows float64 [K,15], ids int64 [K],
    sem int64 [K]): ids are the file's `values`, 1 + k where it has none"""
    f = boxset.read_boxes(path)
    sem = boxset.file_classes(f).astype(np.int64)
    rows = box_frames(f)
    ids = 1 + np.arange(rows.shape[0], dtype=np.int64) if f.values is None else np.asarray(f.values).astype(np.int64)
    if ids.shape != (rows.shape[0],):
        raise ValueError("%s: %d ids for %d boxes" % (path, ids.size, rows.shape[0]))
    if rows.shape[0] and (int(sem.min()) < 1 or int(ids.min()) < 1):
        raise ValueError("%s: classes and ids must be >= 1 (the label files count from 1)" % path)
    return rows, ids, sem


def boxlabels_scan(scene_path: str, root: str, p: dict, made=None, force: bool = False, device=None, stream=None):
    """One scan directory -> the label files of the scene under ROOT/label/seg/<style-name>/raw -> its entry of boxlabels_report.json, or
    None when the .ins.txt was there already (never overwritten without `force`).  `made`: (rows, ids, sem) read already."""
    from . import boxes, labels
    from .prepare import mesh_arrays, read_ply
    scene = scans.scene_name(scene_path)
    out = os.path.join(root, "label", "seg", p["style_name"], "raw", scene)
    if os.path.exists(os.path.join(out, scene + ".ins.txt")) and not force:
        return None
    xyz = mesh_arrays(read_ply(os.path.join(scene_path, scene + scans.PLY_SUFFIX)))[0]
    n = int(xyz.shape[0])
    seg = np.asarray(labels.load_seg_labels(os.path.join(scene_path, scene + "_vh_clean_2.0.010000.segs.json")), dtype=np.int64)
    if seg.shape[0] != n:
        raise ValueError(f"{scene}: {seg.shape[0]} segment ids for {n} vertices")
    real = None
    if p.get("from_real"):
        raw = os.path.join(root, "label", "real", "raw", scene)
        real = np.array(labels.load_labels(os.path.join(raw, scene + ".ins.txt")), dtype=np.int64)
        real_sem = np.array(labels.load_labels(os.path.join(raw, scene + ".sem.txt")), dtype=np.int64)
        if real.shape[0] != n or real_sem.shape[0] != n:
            raise ValueError(f"{scene}: {real.shape[0]} real instance and {real_sem.shape[0]} class labels for {n} vertices")
        found = boxes.label_boxes(xyz, np.where(real > 0, real, -1).astype(np.int32), p["kind"], p["angles"] if p["kind"] == "yaw" else None,
                                  p["min_points"], device=device, stream=stream)
        rows, ids, sem = box_frames(found), found.values.astype(np.int64), real_sem[found.first]
        if rows.shape[0] and int(sem.min()) < 1:
            raise ValueError(f"{scene}: instance {int(ids[int(np.argmin(sem))])} has class {int(sem.min())} at its first vertex; classes are >= 1")
    else:
        rows, ids, sem = made if made is not None else file_boxes(os.path.join(p["boxes"], scene + p["suffix"]))
    ins_weak, sem_weak, rep = weak_labels(xyz, seg, rows, ids, sem, p["margin"], p["purity"], p["overlap"], device=device, stream=stream, detail=True)
    arrays = rep.pop("arrays")
    labels._write_txt(os.path.join(out, scene + ".ins.txt"), ins_weak)
    labels._write_txt(os.path.join(out, scene + ".sem.txt"), sem_weak)
    np.savez(os.path.join(out, scene + NPZ_SUFFIX), ids=ids, sem=sem, **arrays)
    entry = dict(rep, V=n, K=int(rows.shape[0]), segments=int(arrays["seg_ids"].shape[0]), segments_labelled=int((arrays["seg_box"] >= 0).sum()))
    for j, b in enumerate(entry["boxes"]):
        b["id"], b["sem"] = int(ids[j]), int(sem[j])
    if real is not None:
        entry["agree"] = int(((ins_weak >= 0) & (ins_weak == real)).sum())
    if os.path.exists(os.path.join(root, "data", "resampled", scene, scene + ".map.pth")):
        labels.generate_weak_label_pth(scene, p["style_name"], root)
        entry["resampled"] = "written"
    else:
        entry["resampled"] = "not written: no data/resampled/%s/%s.map.pth under the root" % (scene, scene)
    return entry


def boxlabels_scans(scans_dir: str, root: str, scenes=None, workers: int = 4, device=None, force: bool = False, **options):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    ROOT/label/seg/<style-name>/boxlabels_report.json.  On the --boxes route every file is read, and refused, before a device call."""
    p = check_command(options.get("from_real"), options.get("boxes"), options.get("suffix"), options.get("kind"), options.get("angles"),
                      options.get("min_points"), options.get("margin"), options.get("purity"), options.get("overlap"), options.get("style_name"))
    made = {}
    if "boxes" in p:
        scenes = file_scenes(scans_dir, p["boxes"], p["suffix"], scenes)
        made = {s: file_boxes(os.path.join(p["boxes"], s + p["suffix"])) for s in scenes}
    dev = torch_device(device)
    out_dir = os.path.join(root, "label", "seg", p["style_name"])
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, {"parameters": p},
                           lambda path, stream: boxlabels_scan(path, root, p, made.get(scans.scene_name(path)), force, dev, stream))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.boxlabels", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply and its segs.json)")
    ap.add_argument("--root", required=True, help="the dataset root: label/real/raw is read, label/seg/<style-name> written, data/resampled looked at")
    ap.add_argument("--from-real", action="store_true", help="simulate the annotator: the boxes of the real instances")
    ap.add_argument("--kind", default=None, help="--from-real: aabb, yaw or pca (default aabb)")
    ap.add_argument("--angles", type=int, default=None, metavar="A", help="--from-real, kind yaw: steps of (pi/2)/A about z, 1..1024 (default 90)")
    ap.add_argument("--min-points", type=int, default=None, metavar="M", help="--from-real: no box for an instance of fewer points (default 1)")
    ap.add_argument("--boxes", default=None, metavar="DIR", help="box files: DIR/<scene><suffix>")
    ap.add_argument("--suffix", default=None, help="--boxes: .boxes.npz (default; it needs `sem`) or _bbox.npy ([K,7])")
    ap.add_argument("--margin", type=float, default=None, metavar="M", help="every box grows by M on every side (default 0)")
    ap.add_argument("--purity", type=float, default=None, metavar="P", help="the share of a segment's vertices its box must own, in (0.5, 1] (default 1)")
    ap.add_argument("--overlap", default=None, help="a vertex in several boxes: skip (default: it votes for no box) or inner (the smallest)")
    ap.add_argument("--style-name", default=None, help="the label style written, label/seg/<style-name> (default box)")
    scans.add_batch_arguments(ap, "overwrite existing label files")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    options = dict(from_real=a.from_real, boxes=a.boxes, suffix=a.suffix, kind=a.kind, angles=a.angles, min_points=a.min_points, margin=a.margin,
                   purity=a.purity, overlap=a.overlap, style_name=a.style_name)
    try:
        p = check_command(*(options[k] for k in ("from_real", "boxes", "suffix", "kind", "angles", "min_points", "margin", "purity", "overlap",
                                                  "style_name")))
        if "boxes" in p:
            for s in file_scenes(a.scans, p["boxes"], p["suffix"], scans.scene_list(a.scenes)):
                file_boxes(os.path.join(p["boxes"], s + p["suffix"]))
    except ValueError as e:
        ap.error(str(e))
    try:
        report, skipped = boxlabels_scans(a.scans, a.root, scans.scene_list(a.scenes), a.workers, a.device, a.force, **options)
    except ValueError as e:
        ap.error(str(e))
    scans.print_outcome(report, skipped, lambda scene, e: ("boxlabels", scene, e["V"], "vertices,", e["K"], "boxes,", e["labelled"], "labelled in",
                                                           e["segments_labelled"], "of", e["segments"], "segments,", e["several"], "in several boxes"),
                        "(its .ins.txt exists; --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
