"""ScanNet instance AP / AP50 / AP25 of pseudo labels.

The V-sized work runs on the GPU (`sg_ap_contingency`: one pass over a scene's vertices gives the label-slot x ground-truth-instance
contingency as a few thousand (slot, g, count) triples, which serves every layer of a `.sgl` file); the S-sized work runs on the host:
`sg_ap_fold` turns the triples and one layer's (ins, sem) table rows into that layer's match record, `sg_ap_match` matches greedily at
the ten overlap thresholds, and this module accumulates the (y_true, y_score) pairs over the scenes, integrates the precision-recall
curves in float64 and formats the table.

Semantics (the benchmark script as the label consumer's evaluator carries it): ground-truth id = sem*1000 + ins where ins > 0, else 0;
all vertices count; predicted instances of a layer are the distinct values > 0 of its ins vector in ascending order, labelled with the sem
value at their lowest vertex, dropped when that label is not one of the 18 classes or the instance has fewer than 100 vertices.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import hip

CLASS_IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
CLASS_LABELS = ["cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
                "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture"]
OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)      # the thresholds as the benchmark script forms them (the last one is AP25)
DEFAULT_GT_CAP = 256          # ground-truth ids per scene the first call's workspace allows for (ScanNet scenes hold a few dozen)


def gt_ids(gt: np.ndarray) -> np.ndarray:
    """[V] int64 ground-truth ids of a [V,2] (sem, ins) array; refuses what would be miscounted."""
    gt = np.asarray(gt)
    if gt.ndim != 2 or gt.shape[1] != 2:
        raise ValueError("ground truth must be [V, 2] (sem, ins)")
    sem, ins = gt[:, 0].astype(np.int64), gt[:, 1].astype(np.int64)
    if sem.size and (sem.min() < 0 or sem.max() > 40):
        raise ValueError("ground-truth sem outside 0..40")
    if ins.size and ins.max() >= 1000:
        raise ValueError("ground-truth ins >= 1000 does not fit gt_id = sem*1000 + ins")
    return np.where(ins > 0, sem * 1000 + ins, 0)


class Contingency:
    """One scene: gt [G,2] (id, count; entry 0 = id 0), first_vertex [n_slots], triples [T,3] (slot, g, count) in (slot, g) order."""

    def __init__(self, gt: np.ndarray, first_vertex: np.ndarray, triples: np.ndarray):
        self.gt = np.ascontiguousarray(gt, dtype=np.int32).reshape(-1, 2)
        self.first_vertex = np.ascontiguousarray(first_vertex, dtype=np.int32)
        self.triples = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)


class Record:
    """One (scene, layer): pred [P,6] (mask index, ins value, label id, vertex count, void intersection, matches), match [M,2]
    (ground-truth record, intersection), gtrec [Gv,3] (gt_id, class id, vertex count)."""

    def __init__(self, pred, match, gtrec):
        self.pred, self.match, self.gtrec = pred, match, gtrec

    def dicts(self):
        """(gt2pred, pred2gt) per class name, in the benchmark script's shape but integers only."""
        g2p = {n: [] for n in CLASS_LABELS}
        p2g = {n: [] for n in CLASS_LABELS}
        name = {int(c): n for c, n in zip(CLASS_IDS, CLASS_LABELS)}
        gts = []
        for gid, cls, cnt in self.gtrec.tolist():
            gts.append({"instance_id": gid, "vert_count": cnt, "matched_pred": []})
            g2p[name[cls]].append(gts[-1])
        m = 0
        for k, (_mask, _val, lab, cnt, void, nm) in enumerate(self.pred.tolist()):
            p = {"pred_id": k, "label_id": lab, "vert_count": cnt, "void_intersection": void, "matched_gt": []}
            for g, inter in self.match[m:m + nm].tolist():
                p["matched_gt"].append([gts[g]["instance_id"], gts[g]["vert_count"], inter])
                gts[g]["matched_pred"].append([k, cnt, inter])
            m += nm
            p2g[name[lab]].append(p)
        return g2p, p2g


class Matches:
    """y_true / y_score per (class, overlap), info [18*n, 3] = hard false negatives, has_gt, has_pred."""

    def __init__(self, y_true, y_score, y_off, info):
        self.y_true, self.y_score, self.y_off, self.info = y_true, y_score, y_off, info


def _desc(items, gts, sov_width: Optional[int] = None):
    """Host staging of B scenes: (h_desc [B,6] int64 as sg_eval_tables', seg_of_vertex flat as uint16 (0xFFFF = -1) or int32, width)."""
    width = sov_width or (2 if all(p.S < 65535 for p in items) else 4)
    if width not in (2, 4) or (width == 2 and any(p.S >= 65535 for p in items)):
        raise ValueError("seg_of_vertex width %r does not hold these scenes" % (sov_width,))
    h = np.zeros((len(items), 6), dtype=np.int64)
    sovs, off = [], 0
    for b, p in enumerate(items):
        if np.asarray(gts[b]).shape[0] != p.V:
            raise ValueError("scene %d: %d vertices in the labels, %d in the ground truth" % (b, p.V, np.asarray(gts[b]).shape[0]))
        sov = p.seg_of_vertex
        sovs.append(np.where(sov < 0, 0xFFFF, sov).astype(np.uint16) if width == 2 else sov)
        h[b] = (0, p.S, off, p.V, off, 0)
        off += p.V
    return h, np.concatenate(sovs), width


def _run(call, ws_bytes, B, n_first, v_total, device, gt_cap):
    """Allocate outputs and workspace, run `call`; a scene with more ground-truth ids than gt_cap sizes a second call."""
    import torch
    for _ in range(2):
        counts = np.zeros((B, 2), np.int64)
        h_gt = np.empty((B * gt_cap, 2), np.int32)
        h_first = np.empty(n_first, np.int32)
        h_trip = np.empty((max(v_total, 1), 3), np.int32)
        ws = torch.empty(max(int(ws_bytes(gt_cap)), 256), dtype=torch.uint8, device=device)
        rc = call(gt_cap, counts, h_gt, h_first, h_trip, ws)
        if rc == hip.SG_ENOMEM and counts[:, 0].max() > gt_cap:
            gt_cap = int(counts[:, 0].max())
            continue
        hip.check_arg(rc)
        return counts, h_gt, h_first, h_trip
    raise RuntimeError("sg_ap_contingency: ground-truth list did not fit twice")


def contingency_batch(items, gts: Sequence[np.ndarray], device=None, flags: int = 0, gt_cap: int = DEFAULT_GT_CAP,
                      sov_width: Optional[int] = None) -> List[Contingency]:
    """`sg_ap_contingency` over B scenes (PseudoLabels + [V,2] ground truth each): segments x ground-truth instances."""
    import torch
    from .pseudo_labels import upload
    hip.require_device()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    B = len(items)
    if B == 0:
        return []
    h_desc, sov_all, width = _desc(items, gts, sov_width)
    gt_all = np.concatenate([np.ascontiguousarray(g, dtype=np.int32).reshape(-1, 2) for g in gts])
    lib = hip.lib()
    n_first = int((h_desc[:, 1] + 1).sum())
    with torch.cuda.device(dev):
        g_sov = upload(sov_all if sov_all.size else np.zeros(1, sov_all.dtype), dev)
        g_gt = upload(gt_all if gt_all.size else np.zeros((1, 2), np.int32), dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def call(cap, counts, h_gt, h_first, h_trip, ws):
            return lib.sg_ap_contingency(B, h_desc.ctypes.data, g_sov.data_ptr(), width, g_gt.data_ptr(), cap, flags, counts.ctypes.data,
                                         h_gt.ctypes.data, h_first.ctypes.data, h_trip.ctypes.data, h_trip.shape[0], ws.data_ptr(),
                                         int(ws.numel()), st)
        counts, h_gt, h_first, h_trip = _run(call, lambda cap: lib.sg_ap_contingency_ws_bytes(B, h_desc.ctypes.data, cap), B, n_first,
                                             int(h_desc[:, 3].sum()), dev, gt_cap)
    out, go, fo, to = [], 0, 0, 0
    for b in range(B):
        G, T, S1 = int(counts[b, 0]), int(counts[b, 1]), int(h_desc[b, 1]) + 1
        out.append(Contingency(h_gt[go:go + G].copy(), h_first[fo:fo + S1].copy(), h_trip[to:to + T].copy()))
        go, fo, to = go + G, fo + S1, to + T
    return out


def contingency_vector(ins: np.ndarray, gt: np.ndarray, device=None, flags: int = 0, gt_cap: int = DEFAULT_GT_CAP, g_gt=None) -> Contingency:
    """`sg_ap_contingency_vectors`: one scene from an instance vector (slot = the value, values <= 0 share slot 0)."""
    import torch
    hip.require_device()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ins = np.ascontiguousarray(ins, dtype=np.int32)
    V = ins.shape[0]
    if np.asarray(gt).shape[0] != V:
        raise ValueError("%d label values for %d ground-truth vertices" % (V, np.asarray(gt).shape[0]))
    S = max(int(ins.max()) if V else 0, 0)
    h_desc = np.array([[0, S, 0, V, 0, 0]], dtype=np.int64)
    lib = hip.lib()
    with torch.cuda.device(dev):
        g_ins = torch.from_numpy(ins if V else np.zeros(1, np.int32)).to(dev)
        if g_gt is None:
            g = np.ascontiguousarray(gt, dtype=np.int32).reshape(-1, 2)
            g_gt = torch.from_numpy(g if V else np.zeros((1, 2), np.int32)).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def call(cap, counts, h_gt, h_first, h_trip, ws):
            return lib.sg_ap_contingency_vectors(g_ins.data_ptr(), V, S, g_gt.data_ptr(), cap, flags, counts.ctypes.data, h_gt.ctypes.data,
                                                 h_first.ctypes.data, h_trip.ctypes.data, h_trip.shape[0], ws.data_ptr(), int(ws.numel()), st)
        counts, h_gt, h_first, h_trip = _run(call, lambda cap: lib.sg_ap_contingency_ws_bytes(1, h_desc.ctypes.data, cap), 1, S + 1, V, dev, gt_cap)
    return Contingency(h_gt[:int(counts[0, 0])].copy(), h_first.copy(), h_trip[:int(counts[0, 1])].copy())


def vector_rows(cont: Contingency, sem: np.ndarray):
    """The (ins, sem) rows of the vector form: ins_row[slot] = slot, sem_row[slot] = the sem value at the slot's lowest vertex."""
    n = cont.first_vertex.shape[0]
    ins_row = np.arange(n, dtype=np.int32)
    sem = np.asarray(sem)
    fv = cont.first_vertex
    if fv.size and fv.max() >= sem.shape[0]:
        raise ValueError("a first vertex lies beyond the sem vector's %d values" % sem.shape[0])
    sem_row = np.where(fv >= 0, sem[np.maximum(fv, 0)] if sem.size else -1, -1).astype(np.int32)
    return ins_row, sem_row


def fold(cont: Contingency, ins_row: np.ndarray, sem_row: np.ndarray) -> Record:
    """`sg_ap_fold`: one layer's match record from a scene's contingency and that layer's (ins, sem) table rows."""
    ins_row = np.ascontiguousarray(ins_row, dtype=np.int32)
    sem_row = np.ascontiguousarray(sem_row, dtype=np.int32)
    if ins_row.ndim != 1 or ins_row.shape != sem_row.shape:
        raise ValueError("ins and sem rows differ in length (%s, %s)" % (ins_row.shape, sem_row.shape))
    T, G, n_slots, n_row = cont.triples.shape[0], cont.gt.shape[0], cont.first_vertex.shape[0], ins_row.shape[0]
    pred = np.zeros((max(n_row, 1), 6), np.int32)
    match = np.zeros((max(T, 1), 2), np.int32)
    gtrec = np.zeros((max(G, 1), 3), np.int32)
    n = np.zeros(3, np.int64)
    hip.check_arg(hip.lib().sg_ap_fold(cont.triples.ctypes.data, T, cont.first_vertex.ctypes.data, n_slots, cont.gt.ctypes.data, G, ins_row.ctypes.data,
                                sem_row.ctypes.data, n_row, pred.ctypes.data, pred.shape[0], match.ctypes.data, match.shape[0],
                                gtrec.ctypes.data, gtrec.shape[0], n.ctypes.data))
    return Record(pred[:n[0]].copy(), match[:n[1]].copy(), gtrec[:n[2]].copy())


def match(rec: Record, conf: Optional[np.ndarray] = None, overlaps: np.ndarray = OVERLAPS) -> Matches:
    """`sg_ap_match`: greedy matching at every overlap.  conf: one confidence per mask (indexed by mask index), default 1.0."""
    P, M, Gv = rec.pred.shape[0], rec.match.shape[0], rec.gtrec.shape[0]
    ov = np.ascontiguousarray(overlaps, dtype=np.float64)
    n = ov.shape[0]
    c = None
    if conf is not None:
        conf = np.asarray(conf, dtype=np.float64)
        if P and int(rec.pred[:, 0].max()) >= conf.shape[0]:
            raise ValueError("%d confidences for mask index %d" % (conf.shape[0], int(rec.pred[:, 0].max())))
        c = np.ascontiguousarray(conf[rec.pred[:, 0]])
    cap = max(n * (Gv + M + P), 1)
    y_score, y_true = np.zeros(cap, np.float64), np.zeros(cap, np.uint8)
    y_off, info = np.zeros(len(CLASS_LABELS) * n + 1, np.int64), np.zeros((len(CLASS_LABELS) * n, 3), np.int32)
    hip.check_arg(hip.lib().sg_ap_match(rec.pred.ctypes.data, P, rec.match.ctypes.data, M, rec.gtrec.ctypes.data, Gv, None if c is None else c.ctypes.data,
                                 ov.ctypes.data, n, y_score.ctypes.data, y_true.ctypes.data, cap, y_off.ctypes.data, info.ctypes.data))
    return Matches(y_true[:y_off[-1]], y_score[:y_off[-1]], y_off, info)


def average_precision(y_true: np.ndarray, y_score: np.ndarray, hard_fn: int) -> float:
    """Area under the precision-recall curve of one (class, overlap), float64: a point per distinct score (everything at or above it
    counts as predicted), the artificial end point (precision 1, recall 0), recall steps centred on each point."""
    y_true = np.asarray(y_true, dtype=np.float64)
    y_score = np.asarray(y_score, dtype=np.float64)
    order = np.argsort(y_score, kind="stable")
    score, true = y_score[order], y_true[order]
    cum = np.cumsum(true)
    _, first = np.unique(score, return_index=True)
    n = score.shape[0]
    total = cum[-1] if n else 0.0
    below = np.where(first > 0, cum[np.maximum(first - 1, 0)], 0.0) if n else np.zeros(0)
    tp = total - below
    fp = n - first - tp
    fn = below + hard_fn
    precision = np.append(tp / (tp + fp), 1.0)
    recall = np.append(tp / (tp + fn), 0.0)
    r = np.concatenate([recall[:1], recall, [0.0]])
    return float(np.dot(precision, 0.5 * (r[:-2] - r[2:])))


class APAccumulator:
    """The pairs of every (class, overlap) over the scenes added, in the order added."""

    def __init__(self, overlaps: np.ndarray = OVERLAPS):
        self.overlaps = np.asarray(overlaps, dtype=np.float64)
        k = len(CLASS_LABELS) * self.overlaps.shape[0]
        self.y_true: List[List[np.ndarray]] = [[] for _ in range(k)]
        self.y_score: List[List[np.ndarray]] = [[] for _ in range(k)]
        self.info = np.zeros((k, 3), np.int64)
        self.scenes = 0

    def add(self, m: Matches) -> None:
        for i in range(self.info.shape[0]):
            a, b = int(m.y_off[i]), int(m.y_off[i + 1])
            if b > a:
                self.y_true[i].append(m.y_true[a:b])
                self.y_score[i].append(m.y_score[a:b])
        self.info[:, 0] += m.info[:, 0]
        self.info[:, 1:] |= m.info[:, 1:]
        self.scenes += 1

    def ap(self) -> np.ndarray:
        """[18, overlaps] float64: NaN without ground truth, 0 with ground truth and no prediction."""
        n = self.overlaps.shape[0]
        out = np.full((len(CLASS_LABELS), n), np.nan)
        for i in range(self.info.shape[0]):
            hard_fn, has_gt, has_pred = self.info[i]
            if has_gt and has_pred:
                yt = np.concatenate(self.y_true[i]) if self.y_true[i] else np.zeros(0)
                ys = np.concatenate(self.y_score[i]) if self.y_score[i] else np.zeros(0)
                out[i // n, i % n] = average_precision(yt, ys, int(hard_fn))
            elif has_gt:
                out[i // n, i % n] = 0.0
        return out


def compute_averages(ap: np.ndarray, overlaps: np.ndarray = OVERLAPS) -> dict:
    """AP = mean over the overlaps other than 0.25, AP50, AP25; per class plain means (NaN stays), over the classes nanmean."""
    o50, o25 = np.isclose(overlaps, 0.5), np.isclose(overlaps, 0.25)
    rest = ~o25
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = {"all_ap": float(np.nanmean(ap[:, rest])), "all_ap_50%": float(np.nanmean(ap[:, o50])), "all_ap_25%": float(np.nanmean(ap[:, o25])),
                   "classes": {}}
            for k, name in enumerate(CLASS_LABELS):
                out["classes"][name] = {"ap": float(np.average(ap[k, rest])), "ap50%": float(np.average(ap[k, o50])),
                                        "ap25%": float(np.average(ap[k, o25]))}
    return out


def report_lines(avgs: dict) -> List[str]:
    """The table in the label consumer's layout: what : AP AP_50% AP_25%, a row per class, the averages."""
    width = 64
    lines = ["", "#" * width, "{:<15}:{:>15}{:>15}{:>15}".format("what", "AP", "AP_50%", "AP_25%"), "#" * width]
    for name in CLASS_LABELS:
        c = avgs["classes"][name]
        lines.append("{:<15}:{:>15.3f}{:>15.3f}{:>15.3f}".format(name, c["ap"], c["ap50%"], c["ap25%"]))
    lines.append("-" * width)
    lines.append("{:<15}:{:>15.3f}{:>15.3f}{:>15.3f}".format("average", avgs["all_ap"], avgs["all_ap_50%"], avgs["all_ap_25%"]))
    lines.append("")
    return lines


def to_json(avgs: dict) -> dict:
    return {"ap": avgs["all_ap"], "ap50": avgs["all_ap_50%"], "ap25": avgs["all_ap_25%"],
            "classes": {n: {"ap": c["ap"], "ap50": c["ap50%"], "ap25": c["ap25%"]} for n, c in avgs["classes"].items()}}


def layer_matches(cont: Contingency, ins_row, sem_row, conf=None) -> Matches:
    return match(fold(cont, ins_row, sem_row), conf)
