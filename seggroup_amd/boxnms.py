"""Non-maximum suppression of 3D boxes on the GPU: the duplicates of a box set removed before it is scored (`boxap`) or
turned into labels (`boxlabels`).  A detector hands over several overlapping proposals per object, and a pseudo instance that fell into
pieces gives stacked near-identical boxes; both count as false positives and both leave every vertex "in several boxes".

    nms   = box_nms(boxes, scores, iou, cls, off)         -- sg_box_nms: Nms(keep, rep, rank), int32 [K] each, by the box's position;
                                                             indices within the scene when `off` ([B+1]) delimits scenes
    sizes = cluster_sizes(nms, off)                       -- host: the boxes every kept box represents (itself included)

THE RULE (include/seggroup_hip.h; tests/boxnms_ref.py restates it).  Within a scene box i comes before box j iff its score is higher, or
equal and i < j.  The scene is visited in that order; a box is SUPPRESSED iff an earlier box that was KEPT, of its class (when classes
are given), has IoU with it above `iou`, strictly -- the upright IoU of 8u with the earlier box as `a`.  Its representative `rep` is the
first such box; a kept box represents itself.  A box that only a suppressed box overlaps is kept.  Boxes are upright (kind aabb or
yaw, or [K,8] rows cx cy cz sx sy sz c s); kind pca is refused.  The row layout, the two kinds of box file and the limits of a call are
seggroup_amd/boxset.py's.

    python -m seggroup_amd.boxnms --boxes DIR --out DIR [--suffix .boxes.npz|_bbox.npy] --iou T [--score-key NAME] [--class-agnostic]
        [--min-score S] [--scenes FILE --workers W --device D --force]
    --suffix .boxes.npz (default): what `boxes` writes; --score-key names the array of scores and is required (`count`, the points of a
    pseudo instance, is the natural score of pseudo boxes), classes are `sem`.  --suffix _bbox.npy: [K,7] rows, the class in column 6,
    scores in <scene>_score.npy beside the file.  --min-score drops boxes before the suppression; indices always refer to the input file.
    ONE sg_box_nms call serves a batch of scenes.  Written: OUT/<scene><suffix>, the same kind of file with every array whose first
    dimension is K cut to the kept boxes in ascending index (everything else copied; _bbox.npy takes its _score.npy along), so `boxap
    --pred OUT` and `boxlabels --boxes OUT` read the tree as it is; OUT/<scene>.nms.npz (keep, rep, rank, score); OUT/nms_report.json (per
    scene boxes, dropped, kept and the largest cluster; per class in and kept; the parameters).  Nothing is overwritten without --force.

Not here: soft-NMS and score decay, merging a cluster into one box (`rep` is where such a tool starts), IoU of tilted (pca) boxes, a
spatial index over the boxes, scenes of more than 2^14 boxes.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import NamedTuple

import numpy as np

from . import boxset, hip, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_SCENE_BOXES = 1 << 14
MAX_WORDS = 1 << 24
NMS_SUFFIX = ".nms.npz"
REPORT_NAME = "nms_report.json"


class Nms(NamedTuple):
    """box_nms' result, int32 [K] by the box's position: `keep` 1 or 0; `rep` a kept box's own index, a suppressed box's suppressor;
    `rank` the place in the scene's order.  Indices count within the scene."""
    keep: np.ndarray
    rep: np.ndarray
    rank: np.ndarray


def check_iou(iou) -> float:
    if isinstance(iou, (bool, str)) or not isinstance(iou, (int, float, np.floating, np.integer)):
        raise ValueError("the IoU threshold (iou=, --iou) is a number in [0, 1), not %r" % (iou,))
    t = float(iou)
    if not (math.isfinite(t) and 0.0 <= t < 1.0):
        raise ValueError("the IoU threshold (iou=, --iou) is a number in [0, 1), not %r" % (iou,))
    return t


def matrix_words(off) -> int:
    """the 64-bit words of the suppression bit matrix: the sum over the scenes of n * ceil(n / 64)"""
    n = np.diff(np.asarray(off, np.int64))
    return int((n * ((n + 63) // 64)).sum())


def _offsets(off, k: int, who: str) -> np.ndarray:
    """boxset.offsets (one scene without `off`), and on top what the bit matrix limits: the boxes of a scene and the words of a call"""
    o = boxset.offsets([0, k] if off is None else off, k, who, "off", "boxes")
    n = np.diff(o)
    if n.size and int(n.max()) > MAX_SCENE_BOXES:
        raise hip.SgError(hip.SG_EUNSUP, "%s: a scene of %d boxes; a scene takes at most 2^14" % (who, int(n.max())))
    if matrix_words(o) > MAX_WORDS:
        raise hip.SgError(hip.SG_EUNSUP, "%s: the bit matrix has %d words; a call takes at most 2^24 (the sum over scenes of n * ceil(n / 64))"
                          % (who, matrix_words(o)))
    return o


def box_nms(boxes, scores, iou, cls=None, off=None, device=None, stream=None) -> Nms:
    """sg_box_nms: `boxes` [K,8] rows (or Boxes of kind aabb or yaw), `scores` [K], `iou` in [0, 1), `cls` [K] whole numbers or None
    (class-agnostic), `off` [B+1] or None (one scene) -> Nms.  Every refusal about shape, kind, threshold or limits comes before any
    device call."""
    import torch
    who = "box_nms"
    rows = boxset.box_rows(boxes, who)
    k = rows.shape[0]
    thresh = check_iou(iou)
    sc = np.asarray(scores)
    if sc.shape != (k,) or not (np.issubdtype(sc.dtype, np.floating) or np.issubdtype(sc.dtype, np.integer)):
        raise ValueError("%s: scores hold one number per box, [%d], not %s %r" % (who, k, sc.dtype, sc.shape))
    sc = np.ascontiguousarray(sc, dtype=np.float64)
    if cls is not None:
        cls = boxset.class_vector(cls, k, who, "cls")
    o = _offsets(off, k, who)
    scenes, words = int(o.shape[0]) - 1, matrix_words(o)
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_box = device_tensor(rows.reshape(-1) if k else np.zeros(8), torch.float64, dev)
        d_score = device_tensor(sc if k else np.zeros(1), torch.float64, dev)
        d_cls = None if cls is None else device_tensor(cls, torch.int32, dev)       # [K+1]
        out = torch.empty((3, max(k, 1)), dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_box_nms_ws_bytes(k, scenes, words), dev)
        hip.check_arg(lib.sg_box_nms(d_box.data_ptr(), d_score.data_ptr(), hip.ptr(d_cls), k, o.ctypes.data, scenes, thresh, out[0].data_ptr(),
                                     out[1].data_ptr(), out[2].data_ptr(), words, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
        rank, keep, rep = out[:, :k].cpu().numpy()
    return Nms(np.ascontiguousarray(keep), np.ascontiguousarray(rep), np.ascontiguousarray(rank))


def cluster_sizes(nms: Nms, off=None) -> np.ndarray:
    """int64 [K]: the boxes every kept box represents (itself included), 0 at a suppressed box.  Host NumPy."""
    keep, rep = np.asarray(nms.keep), np.asarray(nms.rep, np.int64)
    k = keep.shape[0]
    o = np.array([0, k], np.int64) if off is None else np.asarray(off, np.int64)
    start = np.repeat(o[:-1], np.diff(o))
    return np.bincount(start + rep, minlength=k).astype(np.int64) if k else np.zeros(0, np.int64)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def check_command(suffix, iou, score_key, class_agnostic, min_score) -> dict:
    """the combinations of the command's options that are refused before anything runs (ValueError) -> the parameters in force"""
    suffix = boxset.SUFFIXES[0] if suffix is None else suffix
    if suffix not in boxset.SUFFIXES:
        raise ValueError("--suffix is %s, not %r" % (" or ".join(boxset.SUFFIXES), suffix))
    if iou is None:
        raise ValueError("--iou is needed: the IoU above which an earlier kept box suppresses a later one has no default")
    thresh = check_iou(iou)
    if suffix == boxset.SUFFIXES[0] and not score_key:
        raise ValueError("--score-key is needed with --suffix .boxes.npz: the array of the file that holds the scores (`count` is the "
                         "natural score of pseudo boxes)")
    if suffix == boxset.SUFFIXES[1] and score_key is not None:
        raise ValueError("--score-key names an array of a .boxes.npz; the scores of <scene>_bbox.npy are <scene>%s beside it" % boxset.SCORE_SUFFIX)
    if min_score is not None and (isinstance(min_score, (bool, str)) or not math.isfinite(float(min_score))):
        raise ValueError("--min-score is a finite number, not %r" % (min_score,))
    return dict(suffix=suffix, iou=thresh, score_key=score_key, class_agnostic=bool(class_agnostic),
                min_score=None if min_score is None else float(min_score))


class SceneFile(NamedTuple):
    """one input file: rows [K,8], score [K], cls int32 [K] or None, and what the file held ({name: array}; a .npy: {"rows": [K,7]})"""
    rows: np.ndarray
    score: np.ndarray
    cls: object
    arrays: dict


def read_scene(boxes_dir: str, scene: str, p: dict) -> SceneFile:
    f = boxset.read_boxes(os.path.join(boxes_dir, scene + p["suffix"]))
    rows = boxset.box_rows(f, f.path)
    score = boxset.file_scores(f, p["score_key"])
    cls = None if p["class_agnostic"] else boxset.file_classes(f, "; or pass --class-agnostic").astype(np.int32)
    arrays = dict(f.arrays, score=score) if p["suffix"] == boxset.NPY_SUFFIX else f.arrays       # the _score.npy travels with its _bbox.npy
    return SceneFile(rows, score.astype(np.float64), cls, arrays)


def write_scene(out_dir: str, scene: str, p: dict, f: SceneFile, nms: Nms) -> None:
    """the kept boxes as the same kind of file, and <scene>.nms.npz"""
    k = f.rows.shape[0]
    sel = np.flatnonzero(nms.keep == 1)
    if p["suffix"] == boxset.NPY_SUFFIX:
        np.save(os.path.join(out_dir, scene + boxset.NPY_SUFFIX), f.arrays["rows"][sel])
        np.save(os.path.join(out_dir, scene + boxset.SCORE_SUFFIX), f.arrays["score"][sel])
    else:
        cut = {n: (a[sel] if a.ndim >= 1 and a.shape[0] == k else a) for n, a in f.arrays.items()}
        np.savez(os.path.join(out_dir, scene + boxset.NPZ_SUFFIX), **cut)
    np.savez(os.path.join(out_dir, scene + NMS_SUFFIX), keep=nms.keep, rep=nms.rep, rank=nms.rank, score=f.score)


def nms_batch(batch: list, p: dict, device=None, stream=None) -> list:
    """[SceneFile] -> [Nms], indices referring to each file: boxes below --min-score are dropped first (keep 0, rep -1, rank -1); ONE
    sg_box_nms call per batch of at most 2^16 scenes, 2^20 boxes and 2^24 words"""
    live = [np.ones(f.rows.shape[0], bool) if p["min_score"] is None else f.score >= p["min_score"] for f in batch]
    n = [int(m.sum()) for m in live]
    for f, m in zip(batch, n):
        if m > MAX_SCENE_BOXES:
            raise hip.SgError(hip.SG_EUNSUP, "boxnms: a scene of %d boxes; a scene takes at most 2^14" % m)
    out = []
    for at, end in boxset.pack([(m, m * ((m + 63) // 64)) for m in n], (boxset.MAX_BOXES, MAX_WORDS), boxset.MAX_SCENES):
        part = range(at, end)
        off = np.concatenate([[0], np.cumsum([n[i] for i in part])]).astype(np.int64)
        cls = None if p["class_agnostic"] else np.concatenate([batch[i].cls[live[i]] for i in part]).astype(np.int32)
        got = box_nms(np.concatenate([batch[i].rows[live[i]] for i in part]).reshape(-1, 8), np.concatenate([batch[i].score[live[i]] for i in part]),
                      p["iou"], cls, off, device=device, stream=stream)
        for s, i in enumerate(part):
            back = np.flatnonzero(live[i]).astype(np.int32)                  # the file's index of every box that took part
            a, b = int(off[s]), int(off[s + 1])
            keep, rep, rank = (np.full(batch[i].rows.shape[0], v, np.int32) for v in (0, -1, -1))
            keep[back], rep[back], rank[back] = got.keep[a:b], back[got.rep[a:b]], got.rank[a:b]
            out.append(Nms(keep, rep, rank))
    return out


def scene_names(boxes_dir: str, suffix: str, scenes=None) -> list:
    return boxset.listed_scenes([("{}%s under --boxes" % suffix, boxset.scene_files(boxes_dir, suffix))], scenes)


def nms_scans(boxes_dir: str, out_dir: str, scenes=None, workers: int = 4, device=None, force: bool = False, **options):
    """The command: every file read (and refused) on the host first, ONE sg_box_nms per batch, the cut files, <scene>.nms.npz and
    nms_report.json -> (the report document, the per-scene entries, the skipped scenes)"""
    p = check_command(options.get("suffix"), options.get("iou"), options.get("score_key"), options.get("class_agnostic", False),
                      options.get("min_score"))
    names = scene_names(boxes_dir, p["suffix"], scenes)
    if os.path.abspath(boxes_dir) == os.path.abspath(out_dir):
        raise ValueError("--out is --boxes: the filtered tree is another directory")
    skipped = [s for s in names if os.path.exists(os.path.join(out_dir, s + p["suffix"])) and not force]
    todo = [s for s in names if s not in skipped]
    files = [read_scene(boxes_dir, s, p) for s in todo]                      # a file of more than 2^20 boxes is refused there, by box_rows
    dev = torch_device(device)
    results = nms_batch(files, p, dev)
    os.makedirs(out_dir, exist_ok=True)
    report, classes = {}, {}
    for s, f, r in zip(todo, files, results):
        write_scene(out_dir, s, p, f, r)
        sizes = cluster_sizes(r._replace(rep=np.where(r.rep < 0, np.arange(r.rep.shape[0]), r.rep)))
        sizes[r.rank < 0] = 0
        report[s] = {"boxes": int(f.rows.shape[0]), "dropped": int((r.rank < 0).sum()), "kept": int(r.keep.sum()),
                     "largest_cluster": int(sizes.max()) if sizes.size else 0}
        if f.cls is not None:
            for c in np.unique(f.cls).tolist():
                e = classes.setdefault(str(c), {"in": 0, "kept": 0})
                e["in"] += int((f.cls == c).sum())
                e["kept"] += int(r.keep[f.cls == c].sum())
    doc = {"parameters": {k: v for k, v in p.items() if v is not None}, "scenes": report, "classes": classes, "skipped": skipped}
    scans.write_report(os.path.join(out_dir, REPORT_NAME), doc)
    return doc, report, skipped


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.boxnms", description=__doc__.split("\n\n")[0])
    ap.add_argument("--boxes", required=True, metavar="DIR", help="the tree of <scene>.boxes.npz or <scene>_bbox.npy (with <scene>_score.npy)")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the filtered files, <scene>.nms.npz and nms_report.json go")
    ap.add_argument("--suffix", default=None, help=".boxes.npz (default) or _bbox.npy ([K,7], the class in column 6)")
    ap.add_argument("--iou", type=float, default=None, metavar="T", help="an earlier kept box suppresses a later one above this IoU, in [0, 1); no default")
    ap.add_argument("--score-key", default=None, metavar="NAME", help=".boxes.npz: the array of scores (required); `count` is the natural score of "
                    "pseudo boxes")
    ap.add_argument("--class-agnostic", action="store_true", help="boxes of different classes suppress each other")
    ap.add_argument("--min-score", type=float, default=None, metavar="S", help="drop boxes that score below S before the suppression")
    scans.add_batch_arguments(ap, "overwrite the files of a scene that OUT holds already")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    options = dict(suffix=a.suffix, iou=a.iou, score_key=a.score_key, class_agnostic=a.class_agnostic, min_score=a.min_score)
    try:
        p = check_command(*(options[k] for k in ("suffix", "iou", "score_key", "class_agnostic", "min_score")))
        scene_names(a.boxes, p["suffix"], scans.scene_list(a.scenes))
        doc, report, skipped = nms_scans(a.boxes, a.out, scans.scene_list(a.scenes), a.workers, a.device, a.force, **options)
    except ValueError as e:
        ap.error(str(e))
    scans.print_outcome(report, skipped, lambda scene, e: ("boxnms", scene, e["boxes"], "boxes,", e["kept"], "kept, largest cluster", e["largest_cluster"]),
                        "(its file is in --out: --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
