"""Box IoU and detection AP for label boxes on the GPU: the consumer of what `boxes` makes.  How good are pseudo boxes,
judged the way a 3D detector is judged -- by the IoU of BOXES, not of point masks?

    rows      = boxset.box_rows(boxes)                   -- float64 [K,8] = cx cy cz sx sy sz c s of a Boxes of kind aabb or yaw; the row
                                                            layout, the box files and the limits of a call are seggroup_amd/boxset.py's
    blocks    = box_iou(a, b, off_a, off_b)              -- sg_box_iou: [Ka,Kb], or one block per scene when offsets delimit scenes
    best, iou = box_best(a, b, cls_a, cls_b, off_a, ..)  -- sg_box_best: per box of a the best partner of b in its scene (and class), the
                                                            lowest index among equals, -1 / 0.0 when every IoU is 0; no Ka x Kb table
    m         = match(best, iou, cls, scene_of_pred, n_gt_per_scene_class, score, thresholds)
    report    = evaluate(...)                            -- AP, recall and counts per class and threshold, mAP per threshold

A box is upright (z is its axis) with footprint axes u = (c, s), v = (-s, c).  A box of kind pca is tilted, so it is refused: its exact
3D IoU is another algorithm.

THE SCORING RULE (host NumPy, K-sized; tests/boxap_ref.py implements it independently).  Per class and threshold t, the predictions of
the class over all scenes are visited by descending score, scene order and then box index breaking ties (pseudo boxes carry no score:
1.0 for all).  A prediction is a TRUE POSITIVE when its best same-class ground-truth box of its scene has IoU > t (strict) and no
earlier prediction took that box; otherwise it is a false positive.  A ground-truth box nobody took is a miss.  The precision-recall
curve has one point per distinct score (everything at or above it counts), as `ap.average_precision` does it -- so the result does
not depend on the order among equal scores: a box is taken once whoever comes first.  AP is the area under the monotone precision
envelope, sum (r_j - r_{j-1}) * max_{k >= j} p_k with r_0 = 0, in ascending j; no 11-point sampling.  AP of a class without ground
truth is NaN, with ground truth and no prediction 0.  mAP is the mean over the classes that have at least one ground-truth box; recall
is true positives / ground-truth boxes.

    python -m seggroup_amd.boxap --scans DIR --out DIR
        ( -n EXP --stage S [--layer final] [--root .] [--label_style manual]    # predictions and ground truth made here
        | --pred DIR --gt DIR )                                                 # two trees of <scene>.boxes.npz that hold `sem`
        [--kind aabb|yaw] [--angles A] [--min-points M] [--classes scannet18|all] [--score-key NAME] [--thresholds 0.25 0.5]
        [--scenes FILE --workers W --device D]
    Experiment route: the predictions are what `boxes` makes (boxes.scene_labels + label_boxes under AP's rules: --min-points 100,
    scannet18); the ground-truth boxes are label_boxes of ap.gt_ids(evaluate.load_gt(..)), id 0 ignored, class = id // 1000, the same
    --kind and class filter, no minimum count.  File route: every <scene>.boxes.npz of --pred has its partner in --gt (a scene on one
    side only is refused by name), both hold `sem`, neither is of kind pca; --score-key names the array of scores in the --pred files;
    --kind, --angles and --min-points belong to the experiment route.  ONE sg_box_best call serves a batch of scenes.  Per scene
    OUT/<scene>.boxmatch.npz (best, iou, cls per prediction, and the ground truth's classes), one OUT/boxap_report.json (per class and
    threshold AP, recall, predictions, ground truth, true positives; mAP per threshold; the parameters), and the table on the terminal.

Not here: exact 3D IoU of tilted (pca) boxes, rotating calipers, an up axis other than z; which boxes hold a point (any kind, pca too) is
seggroup_amd/boxlabels.py; non-maximum suppression -- a prediction tree with duplicates counts each as a false positive
-- is seggroup_amd/boxnms.py, whose filtered tree --pred reads as it is.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import NamedTuple

import numpy as np

from . import boxset, hip, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_PAIRS = 1 << 24
MATCH_SUFFIX = ".boxmatch.npz"
REPORT_NAME = "boxap_report.json"
DEFAULT_THRESHOLDS = (0.25, 0.5)


def _sets(a, b, off_a, off_b, who: str):
    """the two sets of an entry -> their rows [Ka,8], [Kb,8] and their scene offsets, int32 [B+1] each"""
    ra, rb = boxset.box_rows(a, who), boxset.box_rows(b, who)
    oa, ob = boxset.paired_offsets(who, (off_a, ra.shape[0], "off_a", "boxes of its set"), (off_b, rb.shape[0], "off_b", "boxes of its set"))
    return ra, rb, oa, ob


def box_iou(a, b, off_a=None, off_b=None, device=None, stream=None):
    """sg_box_iou: `a` [Ka,8] and `b` [Kb,8] rows (or Boxes) -> float64 [Ka,Kb]; with `off_a` / `off_b` ([B+1] each) the list of the B
    scenes' [Ka_b,Kb_b] blocks.  More than 2^24 pairs are refused (box_best has no such limit)."""
    import torch
    ra, rb, oa, ob = _sets(a, b, off_a, off_b, "box_iou")
    na, nb = np.diff(oa).astype(np.int64), np.diff(ob).astype(np.int64)
    pairs = int((na * nb).sum())
    if pairs > MAX_PAIRS:
        raise hip.SgError(hip.SG_EUNSUP, "box_iou: %d pairs; a call writes at most 2^24 (box_best has no such limit)" % pairs)
    dev = torch_device(device)
    lib = hip.lib()
    scenes = int(oa.shape[0]) - 1
    with torch.cuda.device(dev), on_stream(stream):
        d_a, d_b = device_tensor(ra, torch.float64, dev), device_tensor(rb, torch.float64, dev)
        d_iou = torch.empty(max(pairs, 1), dtype=torch.float64, device=dev)
        ws = workspace(lib.sg_box_iou_ws_bytes(ra.shape[0], rb.shape[0], scenes), dev)
        hip.check_arg(lib.sg_box_iou(d_a.data_ptr(), ra.shape[0], d_b.data_ptr(), rb.shape[0], oa.ctypes.data, ob.ctypes.data, scenes,
                                     d_iou.data_ptr(), pairs, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
        flat = d_iou[:pairs].cpu().numpy()
    ends = np.concatenate([[0], np.cumsum(na * nb)])
    blocks = [flat[ends[s]:ends[s + 1]].reshape(int(na[s]), int(nb[s])) for s in range(scenes)]
    return blocks if off_a is not None else blocks[0]


def box_best(a, b, cls_a=None, cls_b=None, off_a=None, off_b=None, device=None, stream=None):
    """sg_box_best -> (best int32 [Ka], iou float64 [Ka]): per box of `a` the index, within its scene's boxes of `b`, of the highest IoU
    (the lowest index among equals) and that IoU -- the bits box_iou gives for the pair; -1 and 0.0 when every IoU is 0.  `cls_a` /
    `cls_b` (both or neither) restrict partners to the same class."""
    import torch
    ra, rb, oa, ob = _sets(a, b, off_a, off_b, "box_best")
    if (cls_a is None) != (cls_b is None):
        raise ValueError("box_best: classes are given for both sets or for neither")
    if cls_a is not None:
        cls_a, cls_b = boxset.class_vector(cls_a, ra.shape[0], "box_best", "cls_a"), boxset.class_vector(cls_b, rb.shape[0], "box_best", "cls_b")
    dev = torch_device(device)
    lib = hip.lib()
    scenes = int(oa.shape[0]) - 1
    with torch.cuda.device(dev), on_stream(stream):
        d_a, d_b = device_tensor(ra, torch.float64, dev), device_tensor(rb, torch.float64, dev)
        d_ca = d_cb = None
        if cls_a is not None:
            d_ca, d_cb = device_tensor(cls_a, torch.int32, dev), device_tensor(cls_b, torch.int32, dev)     # [K+1]: both or neither are pointers
        best = torch.empty(max(ra.shape[0], 1), dtype=torch.int32, device=dev)
        top = torch.empty(max(ra.shape[0], 1), dtype=torch.float64, device=dev)
        ws = workspace(lib.sg_box_best_ws_bytes(ra.shape[0], rb.shape[0], scenes), dev)
        hip.check_arg(lib.sg_box_best(d_a.data_ptr(), ra.shape[0], d_b.data_ptr(), rb.shape[0], hip.ptr(d_ca), hip.ptr(d_cb), oa.ctypes.data,
                                      ob.ctypes.data, scenes, best.data_ptr(), top.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
        return best[:ra.shape[0]].cpu().numpy(), top[:ra.shape[0]].cpu().numpy()


# ---- the scoring rule (host) ----------------------------------------------------------------------------------------------------------------
class Matched(NamedTuple):
    """match's result: `tp` bool [T,K], a row per threshold; `n_gt` {class: ground-truth boxes over the scenes}; `missed` [T] of
    {class: ground-truth boxes nobody took}"""
    tp: np.ndarray
    n_gt: dict
    missed: list


def check_thresholds(thresholds) -> tuple:
    t = tuple(float(v) for v in (thresholds if np.ndim(thresholds) else (thresholds,)))
    if not t or any(not (0.0 <= v < 1.0) for v in t) or len(set(t)) != len(t):
        raise ValueError("thresholds (thresholds=, --thresholds) are distinct IoU values in [0, 1), not %r" % (thresholds,))
    return t


def _prediction_vectors(best, iou, cls, scene_of_pred, score):
    best, iou, cls, scene = (np.asarray(v) for v in (best, iou, cls, scene_of_pred))
    k = best.shape[0] if best.ndim == 1 else -1
    if k < 0 or iou.shape != (k,) or cls.shape != (k,) or scene.shape != (k,):
        raise ValueError("match: best, iou, cls and scene_of_pred hold one value per prediction, [K]")
    sc = np.ones(k) if score is None else np.asarray(score, np.float64)
    if sc.shape != (k,) or not np.isfinite(sc).all():
        raise ValueError("match: score is one finite number per prediction, [%d]" % k)
    return best.astype(np.int64), iou.astype(np.float64), cls.astype(np.int64), scene.astype(np.int64), sc


def match(best, iou, cls, scene_of_pred, n_gt_per_scene_class, score=None, thresholds=DEFAULT_THRESHOLDS) -> Matched:
    """The first-comer rule of the module docstring.  `best`, `iou` as box_best gives them WITH classes, `cls` and `scene_of_pred` per
    prediction; `n_gt_per_scene_class` {(scene, class): ground-truth boxes}; `score` [K] or None (1.0 for all)."""
    best, iou, cls, scene, sc = _prediction_vectors(best, iou, cls, scene_of_pred, score)
    thresholds = check_thresholds(thresholds)
    n_gt: dict = {}
    for (s, c), n in n_gt_per_scene_class.items():
        if int(n) < 0:
            raise ValueError("match: a negative count of ground-truth boxes for scene %r, class %r" % (s, c))
        n_gt[int(c)] = n_gt.get(int(c), 0) + int(n)
    k = best.shape[0]
    order = np.lexsort((np.arange(k), scene, -sc))                          # descending score, then scene, then index
    tp = np.zeros((len(thresholds), k), bool)
    missed = []
    for row, t in enumerate(thresholds):
        taken = set()
        for i in order:
            if best[i] < 0 or not iou[i] > t:
                continue
            key = (int(scene[i]), int(cls[i]), int(best[i]))
            if key not in taken:
                taken.add(key)
                tp[row, i] = True
        got: dict = {}
        for _, c, _ in taken:
            got[c] = got.get(c, 0) + 1
        missed.append({c: n - got.get(c, 0) for c, n in n_gt.items()})
    return Matched(tp, n_gt, missed)


def average_precision(tp, score, n_gt: int) -> tuple:
    """One class at one threshold -> (AP, recall): a point per distinct score, the area under the monotone precision envelope.  NaN
    without ground truth, 0 with ground truth and no prediction."""
    tp = np.asarray(tp, bool)
    score = np.asarray(score, np.float64)
    if tp.ndim != 1 or score.shape != tp.shape:
        raise ValueError("average_precision: tp and score hold one value per prediction")
    if n_gt <= 0:
        return float("nan"), float("nan")
    if tp.shape[0] == 0:
        return 0.0, 0.0
    order = np.argsort(-score, kind="stable")
    s = score[order]
    ntp = np.cumsum(tp[order]).astype(np.float64)
    last = np.append(s[1:] != s[:-1], True)                                 # the last prediction of every distinct score
    ntp = ntp[last]
    seen = (np.flatnonzero(last) + 1).astype(np.float64)
    recall = ntp / float(n_gt)
    envelope = np.maximum.accumulate((ntp / seen)[::-1])[::-1]
    ap, prev = 0.0, 0.0
    for r, p in zip(recall.tolist(), envelope.tolist()):
        ap = ap + (r - prev) * p
        prev = r
    return ap, float(recall[-1])


def evaluate(best, iou, cls, scene_of_pred, n_gt_per_scene_class, score=None, thresholds=DEFAULT_THRESHOLDS) -> dict:
    """-> {"thresholds": {"0.25": {"map": .., "classes": {"5": {"ap", "recall", "pred", "gt", "tp"}}}}}: every class that has a
    prediction or a ground-truth box; mAP over the classes with ground truth."""
    m = match(best, iou, cls, scene_of_pred, n_gt_per_scene_class, score, thresholds)
    _, _, cls, _, sc = _prediction_vectors(best, iou, cls, scene_of_pred, score)
    classes = sorted(set(cls.tolist()) | set(m.n_gt))
    out = {}
    for row, t in enumerate(check_thresholds(thresholds)):
        per, aps = {}, []
        for c in classes:
            mine = cls == c
            g = int(m.n_gt.get(c, 0))
            ap, rec = average_precision(m.tp[row, mine], sc[mine], g)
            per[str(c)] = {"ap": ap, "recall": rec, "pred": int(mine.sum()), "gt": g, "tp": int(m.tp[row, mine].sum())}
            if g > 0:
                aps.append(ap)
        out[repr(t)] = {"map": (sum(aps) / len(aps) if aps else float("nan")), "classes": per}
    return {"thresholds": out}


def report_lines(table: dict) -> list:
    """the table in the layout of `evaluate --ap`: a row per class, per threshold AP and recall, the means"""
    from .ap import CLASS_IDS, CLASS_LABELS
    names = {str(int(c)): n for c, n in zip(CLASS_IDS, CLASS_LABELS)}
    ts = list(table["thresholds"])
    width = 16 + 30 * len(ts) + 24
    head = "{:<15}:".format("what") + "".join("{:>15}{:>15}".format("AP_%g%%" % (100 * float(t)), "recall_%g%%" % (100 * float(t))) for t in ts)
    lines = ["", "#" * width, head + "{:>12}{:>12}".format("pred", "gt"), "#" * width]
    classes = sorted({c for t in ts for c in table["thresholds"][t]["classes"]}, key=int)
    for c in classes:
        cells = [table["thresholds"][t]["classes"][c] for t in ts]
        lines.append("{:<15}:".format(names.get(c, "class " + c)) + "".join("{:>15.3f}{:>15.3f}".format(x["ap"], x["recall"]) for x in cells) +
                     "{:>12d}{:>12d}".format(cells[0]["pred"], cells[0]["gt"]))
    lines.append("-" * width)
    lines.append("{:<15}:".format("average") + "".join("{:>15.3f}{:>15}".format(table["thresholds"][t]["map"], "") for t in ts))
    lines.append("")
    return lines


# ---- scans ------------------------------------------------------------------------------------------------------------------------------------
def check_command(exp, stage, layer, root, label_style, pred, gt, kind, angles, min_points, classes, score_key, thresholds) -> dict:
    """the combinations of the command's options that are refused before anything runs (ValueError) -> the parameters in force"""
    from . import boxes
    if (exp is None) == (pred is None and gt is None):
        raise ValueError("exactly one source of boxes is needed: -n EXP (with --stage) or --pred DIR with --gt DIR")
    if kind == "pca":
        boxset.check_upright(kind, "--kind")
    if classes not in (None, "scannet18", "all"):
        raise ValueError("--classes is scannet18 or all, not %r" % (classes,))
    thresholds = check_thresholds(thresholds)
    if exp is not None:
        if score_key is not None:
            raise ValueError("--score-key names an array of the --pred files: pseudo boxes of an experiment carry no score")
        kind, a, min_points = boxes.check_box_parameters("yaw" if kind is None else kind, angles, boxes.AP_MIN_POINTS if min_points is None else min_points)
        return dict(exp=exp, stage=stage or "epoch_last", layer=layer or "final", root=root or ".", label_style=label_style or "manual", kind=kind,
                    angles=a, min_points=min_points, classes=classes or "scannet18", thresholds=list(thresholds))
    if pred is None or gt is None:
        raise ValueError("--pred DIR and --gt DIR go together")
    if stage is not None or layer is not None or root is not None or label_style is not None:
        raise ValueError("--stage, --layer, --root and --label_style belong to the experiment route (-n EXP)")
    if kind is not None or angles is not None or min_points is not None:
        raise ValueError("--kind, --angles and --min-points belong to the experiment route (-n EXP): the files of --pred / --gt are made already")
    return dict(pred=pred, gt=gt, classes=classes or "all", score_key=score_key, thresholds=list(thresholds))


class SceneBoxes(NamedTuple):
    """one scene of the batch: rows [K,8] and classes [K] of the predictions and of the ground truth, scores [K] or None"""
    pred: np.ndarray
    pred_cls: np.ndarray
    gt: np.ndarray
    gt_cls: np.ndarray
    score: object


def _class_filter(cls, classes):
    if classes == "scannet18":
        from .ap import CLASS_IDS
        return np.isin(cls, CLASS_IDS)
    return np.ones(cls.shape[0], bool)


def experiment_scene(scene_path: str, p: dict, device=None, stream=None) -> tuple:
    """the experiment route for one scan -> (SceneBoxes, vertices)"""
    from . import ap, boxes, evaluate as ev
    from .prepare import mesh_arrays, read_ply
    scene = scans.scene_name(scene_path)
    xyz = mesh_arrays(read_ply(os.path.join(scene_path, scene + scans.PLY_SUFFIX)))[0]
    n = int(xyz.shape[0])
    labels, sem = boxes.scene_labels(scene, n, p["exp"], p["stage"], p["layer"], p["root"])
    angles = p["angles"] if p["kind"] == "yaw" else None
    found = boxes.label_boxes(xyz, labels, p["kind"], angles, 1, device=device, stream=stream)
    cls = sem[found.first].astype(np.int32)
    keep = (found.count >= p["min_points"]) & _class_filter(cls, p["classes"])
    gt = ev.load_gt(p["root"], scene, p["label_style"])
    if gt.shape[0] != n:
        raise ValueError(f"{scene}: {gt.shape[0]} ground-truth labels for {n} vertices")
    ids = ap.gt_ids(gt)
    truth = boxes.label_boxes(xyz, np.where(ids > 0, ids, -1).astype(np.int32), p["kind"], angles, 1, device=device, stream=stream)
    gcls = (truth.values // 1000).astype(np.int32)
    gkeep = _class_filter(gcls, p["classes"])
    return SceneBoxes(boxset.box_rows(found)[keep], cls[keep], boxset.box_rows(truth)[gkeep], gcls[gkeep], None), n


def _file_boxes(path: str, score_key=None):
    """<scene>.boxes.npz -> (rows [K,8], classes int32 [K], scores float64 [K] or None): it needs `sem` and an upright kind"""
    f = boxset.read_boxes(path)
    sem = boxset.file_classes(f).astype(np.int32)
    rows = boxset.box_rows(f, path)
    score = None if score_key is None else boxset.file_scores(f, score_key).astype(np.float64)
    return rows, sem, score


def file_scene(scene: str, p: dict) -> SceneBoxes:
    rows, cls, score = _file_boxes(os.path.join(p["pred"], scene + boxset.NPZ_SUFFIX), p["score_key"])
    grows, gcls, _ = _file_boxes(os.path.join(p["gt"], scene + boxset.NPZ_SUFFIX))
    keep, gkeep = _class_filter(cls, p["classes"]), _class_filter(gcls, p["classes"])
    return SceneBoxes(rows[keep], cls[keep], grows[gkeep], gcls[gkeep], None if score is None else score[keep])


def file_scenes(pred: str, gt: str, scenes=None) -> list:
    """the scenes of the two trees; one that is on one side only is a ValueError that names it"""
    return boxset.listed_scenes([("{}%s under %s" % (boxset.NPZ_SUFFIX, option), boxset.scene_files(d, boxset.NPZ_SUFFIX))
                                 for option, d in (("--pred", pred), ("--gt", gt))], scenes)


def match_batch(batch: list, device=None, stream=None):
    """[SceneBoxes] -> (best [K], iou [K], cls [K], scene_of_pred [K], n_gt {(scene, class): n}, score [K] or None): sg_box_best
    over all the scenes at once, in calls of at most 2^16 scenes and 2^20 boxes a side"""
    best, top = [], []
    for at, end in boxset.pack([(s.pred.shape[0], s.gt.shape[0]) for s in batch], (boxset.MAX_BOXES, boxset.MAX_BOXES), boxset.MAX_SCENES):
        part = batch[at:end]
        off_a = np.concatenate([[0], np.cumsum([s.pred.shape[0] for s in part])]).astype(np.int64)
        off_b = np.concatenate([[0], np.cumsum([s.gt.shape[0] for s in part])]).astype(np.int64)
        b, t = box_best(np.concatenate([s.pred for s in part]).reshape(-1, 8), np.concatenate([s.gt for s in part]).reshape(-1, 8),
                        np.concatenate([s.pred_cls for s in part]).astype(np.int32), np.concatenate([s.gt_cls for s in part]).astype(np.int32),
                        off_a, off_b, device=device, stream=stream)
        best.append(b)
        top.append(t)
    cls = np.concatenate([s.pred_cls for s in batch]).astype(np.int64) if batch else np.zeros(0, np.int64)
    scene = np.concatenate([np.full(s.pred.shape[0], k, np.int64) for k, s in enumerate(batch)]) if batch else np.zeros(0, np.int64)
    n_gt = {}
    for k, s in enumerate(batch):
        for c, n in zip(*np.unique(s.gt_cls, return_counts=True)):
            n_gt[(k, int(c))] = int(n)
    score = None
    if any(s.score is not None for s in batch):
        score = np.concatenate([s.score if s.score is not None else np.ones(s.pred.shape[0]) for s in batch])
    cat = (lambda v, d: np.concatenate(v) if v else np.zeros(0, d))
    return cat(best, np.int32), cat(top, np.float64), cls, scene, n_gt, score


def boxap_scans(scans_dir: str, out_dir: str, scenes=None, workers: int = 4, device=None, **options):
    """The command: boxes of every scene (threads, scans.run_scans), ONE batch of sg_box_best, <scene>.boxmatch.npz per scene and
    boxap_report.json -> (the report document, the per-scene entries)"""
    p = check_command(options.get("exp"), options.get("stage"), options.get("layer"), options.get("root"), options.get("label_style"),
                      options.get("pred"), options.get("gt"), options.get("kind"), options.get("angles"), options.get("min_points"),
                      options.get("classes"), options.get("score_key"), options.get("thresholds", DEFAULT_THRESHOLDS))
    if "exp" in p:
        if scenes is None:
            base = os.path.join(p["root"], "results", p["exp"])
            scenes = [s for s in scans.scan_names(scans_dir) if os.path.isdir(os.path.join(base, s, p["stage"]))]
    made = {}
    if "exp" not in p:                                                       # host work only: every file is read, and refused, before a device call
        scenes = file_scenes(p["pred"], p["gt"], scenes)
        made = {s: file_scene(s, p) for s in scenes}
    dev = torch_device(device)

    def one(path, stream):
        scene, n = scans.scene_name(path), None
        if "exp" in p:
            made[scene], n = experiment_scene(path, p, dev, stream)
        entry = {"pred": int(made[scene].pred.shape[0]), "gt": int(made[scene].gt.shape[0])}
        if n is not None:
            entry["V"] = n
        return entry

    head = {"parameters": {k: v for k, v in p.items() if v is not None}}
    report, _ = scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, head, one)
    batch = [made[s] for s in scenes]
    best, top, cls, scene_of, n_gt, score = match_batch(batch, dev)
    table = evaluate(best, top, cls, scene_of, n_gt, score, p["thresholds"])
    at = 0
    for s, b in zip(scenes, batch):
        k = b.pred.shape[0]
        np.savez(os.path.join(out_dir, s + MATCH_SUFFIX), best=best[at:at + k], iou=top[at:at + k], cls=b.pred_cls, gt_cls=b.gt_cls)
        at += k
    doc = dict(head, scenes=report, skipped=[], **table)
    scans.write_report(os.path.join(out_dir, REPORT_NAME), doc)
    return doc, report


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.boxap", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply); the experiment route reads them")
    ap.add_argument("--out", required=True, help="where <scene>.boxmatch.npz and boxap_report.json go")
    ap.add_argument("-n", "--exp_name", default=None, help="experiment route: name of the experiment")
    ap.add_argument("--stage", default=None, help="experiment route: the export directory's name (default epoch_last)")
    ap.add_argument("--layer", default=None, help="experiment route: final or layer_1 .. layer_4 (default final)")
    ap.add_argument("--root", default=None, help="experiment route: directory holding results/ and dataset/ (default: CWD)")
    ap.add_argument("--label_style", default=None, help="experiment route: the pack's label style (default manual)")
    ap.add_argument("--pred", default=None, metavar="DIR", help="file route: <scene>.boxes.npz of the predictions, with `sem`")
    ap.add_argument("--gt", default=None, metavar="DIR", help="file route: <scene>.boxes.npz of the ground truth, with `sem`")
    ap.add_argument("--kind", default=None, help="experiment route: aabb or yaw (default yaw)")
    ap.add_argument("--angles", type=int, default=None, metavar="A", help="kind yaw: steps of (pi/2)/A about z, 1..1024 (default 90)")
    ap.add_argument("--min-points", type=int, default=None, metavar="M", help="experiment route: drop predictions of fewer points (default 100)")
    ap.add_argument("--classes", default=None, help="scannet18 (the experiment route's default) keeps the 18 benchmark classes; all")
    ap.add_argument("--score-key", default=None, metavar="NAME", help="file route: the array of scores in the --pred files (default: 1.0 for all)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=list(DEFAULT_THRESHOLDS), help="IoU thresholds (default 0.25 0.5)")
    scans.add_batch_arguments(ap, "accepted for symmetry with the other commands: the matches are always computed anew")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    options = dict(exp=a.exp_name, stage=a.stage, layer=a.layer, root=a.root, label_style=a.label_style, pred=a.pred, gt=a.gt, kind=a.kind,
                   angles=a.angles, min_points=a.min_points, classes=a.classes, score_key=a.score_key, thresholds=a.thresholds)
    try:
        check_command(*(options[k] for k in ("exp", "stage", "layer", "root", "label_style", "pred", "gt", "kind", "angles", "min_points",
                                              "classes", "score_key", "thresholds")))
        if a.exp_name is None:
            file_scenes(a.pred, a.gt, scans.scene_list(a.scenes))
    except ValueError as e:
        ap.error(str(e))
    try:
        doc, report = boxap_scans(a.scans, a.out, scans.scene_list(a.scenes), a.workers, a.device, **options)
    except ValueError as e:
        ap.error(str(e))
    scans.print_outcome(report, [], lambda scene, e: ("boxap", scene, e["pred"], "predictions,", e["gt"], "ground-truth boxes"), "", verb="matched")
    print("\n".join(report_lines(doc)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
