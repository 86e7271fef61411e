#!/usr/bin/env python3
"""Golden results of the label consumer's instance-AP evaluator (build container only): runs the UNMODIFIED `pointgroup/util/eval.py`
and `pointgroup/util/utils_3d.py` of the reference (stub `util` / `util.utils` modules, the aliases np.float = float, np.bool = bool) on
eight generated scenes and stores the inputs in tests/golden/ap_cases.npz and what the evaluator computed in tests/golden/ap_expected.json:
per scene and layer every integer of gt2pred / pred2gt, per layer ap[18,10] over the set and the averages.  Predictions are formed from the
label vectors as the reference's conversion of pseudo-label files does (distinct instance values in ascending order, 0 skipped, the label
of the first vertex); -1 (no label) is skipped too.

    python tools/capture_ap.py [--reference DIR]            write the two fixture files
    python tools/capture_ap.py --time [--scenes 6]          the evaluator's own time per 150k-vertex scene on this host (prints JSON)

Nothing of the reference is copied; this script never runs on the GPU box.
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
LAYER_ROWS = {"1": (1, 2), "2": (4, 5), "3": (7, 8), "4": (10, 11), "final": (12, 13)}
CLASS_IDS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
# ground truth uses these: 33 (toilet) is never predicted, 36 and 39 appear nowhere, 1 / 2 / 13 / 40 are void classes
GT_SEMS = [3, 4, 5, 5, 5, 6, 7, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 1, 2, 13, 40]
SCENES = [(20000, 260, 1), (30000, 420, 2), (12000, 150, 3), (26000, 300, 4), (8000, 90, 5), (18000, 240, 6), (30000, 380, 7), (15000, 200, 8)]


def load_reference(ref_root):
    d = os.path.join(ref_root, "pointgroup", "util")
    if not hasattr(np, "float"):
        np.float = float
    if not hasattr(np, "bool"):
        np.bool = bool
    util = types.ModuleType("util")
    util.__path__ = []
    utils = types.ModuleType("util.utils")

    def print_error(msg):
        raise RuntimeError(msg)
    utils.print_error = print_error
    sys.modules["util"], sys.modules["util.utils"] = util, utils
    util.utils = utils
    for name in ("utils_3d", "eval"):
        spec = importlib.util.spec_from_file_location("util." + name, os.path.join(d, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["util." + name] = mod
        setattr(util, name, mod)
        spec.loader.exec_module(mod)
    return sys.modules["util.eval"]


def make_case(V, S, seed):
    """seg_of_vertex [V], tables [14,S], gt [V,2], conf [max id + 1]: contiguous segments in vertex order, ground-truth instances = runs of
    segments, each layer's grouping = the ground truth's perturbed (moved segments, split instances, wrong and void classes, id gaps)."""
    rng = np.random.default_rng(1000 + seed)
    cuts = np.sort(rng.choice(np.arange(1, V), S - 1, replace=False))
    sov = np.searchsorted(cuts, np.arange(V), side="right").astype(np.int32)
    size = np.bincount(sov, minlength=S)
    # ground-truth instances over the segments
    seg_gt = np.zeros(S, np.int64)
    s, k = 0, 0
    while s < S:
        n = int(rng.integers(1, 14))
        k += 1
        seg_gt[s:s + n] = k
        s += n
    n_gt = k
    gt_sem = np.array([GT_SEMS[i] for i in rng.integers(0, len(GT_SEMS), n_gt + 1)])
    gt_sem[1:6] = [5, 7, 33, 5, 1][:max(0, min(5, n_gt))]
    gt = np.stack([gt_sem[seg_gt[sov]], seg_gt[sov]], 1).astype(np.int32)
    gt[rng.random(V) < 0.02] = 0                                   # unannotated vertices
    odd = rng.random(V) < 0.003
    gt[odd, 0] = 0                                                 # ins > 0 with sem == 0
    blank = rng.integers(0, S, max(1, S // 30))                    # whole unannotated segments
    gt[np.isin(sov, blank)] = 0
    tables = np.full((14, S), -1, np.int32)
    for li, (ir, sr) in enumerate(LAYER_ROWS.values()):
        move = rng.random(S) < (0.30 - 0.05 * li)
        ins = np.where(move, np.clip(seg_gt + rng.integers(-1, 2, S), 1, n_gt), seg_gt)
        sem = gt_sem[ins].copy()
        split = rng.choice(np.arange(1, n_gt + 1), max(1, n_gt // 6), replace=False)      # an instance in two halves
        for g in split:
            segs = np.nonzero(ins == g)[0]
            ins[segs[len(segs) // 2:]] = n_gt + g
        wrong = rng.random(S) < 0.08
        sem[wrong] = np.array([1, 2, 13, 0, 5, 12])[rng.integers(0, 6, int(wrong.sum()))]
        ins = ins * 3 + 2                                          # gaps in the ids
        ins[rng.random(S) < 0.03] = -1
        ins[rng.random(S) < 0.02] = 0
        lone = rng.choice(S, max(2, S // 25), replace=False)       # single segments as their own instance (many under 100 vertices)
        ins[lone] = 7000 + 3 * np.arange(lone.size)
        sem[lone] = gt_sem[seg_gt[lone]]
        sem[sem == 33] = 34                                        # toilets are never predicted
        tables[ir], tables[sr] = ins, sem
        tables[3 * li if li < 4 else 0] = np.arange(S)
    sov = sov.copy()
    sov[rng.random(V) < 0.03] = -1                                 # vertices without a segment
    conf = rng.choice([0.3, 0.5, 0.5, 0.9, 0.9, 1.0], int(tables.max()) + 1) + np.where(rng.random(int(tables.max()) + 1) < 0.5, 0.0,
                                                                                        rng.random(int(tables.max()) + 1) * 0.05)
    return sov, tables, gt, conf, size


def expand(tables, sov, row):
    return np.where(sov >= 0, tables[row][np.maximum(sov, 0)], -1)


def gt_id_vector(gt):
    sem, ins = gt[:, 0].astype(np.int64), gt[:, 1].astype(np.int64)
    return np.where(ins > 0, sem * 1000 + ins, 0)


def pred_info(ins, sem, conf):
    vals = [int(v) for v in np.unique(ins) if v > 0]
    masks = [(ins == v).astype(np.int64) for v in vals]
    label = np.array([int(sem[np.nonzero(m)[0][0]]) for m in masks], dtype=np.int64)
    return {"label_id": label, "conf": np.array([conf[v] for v in vals], dtype=np.float64), "mask": masks}


def ints_of(gt2pred, pred2gt):
    g = {n: [{"instance_id": int(x["instance_id"]), "vert_count": int(x["vert_count"]),
              "matched_pred": [[int(p["pred_id"]), int(p["vert_count"]), int(p["intersection"])] for p in x["matched_pred"]]} for x in v]
         for n, v in gt2pred.items()}
    p = {n: [{"pred_id": int(x["pred_id"]), "label_id": int(x["label_id"]), "vert_count": int(x["vert_count"]),
              "void_intersection": int(x["void_intersection"]),
              "matched_gt": [[int(q["instance_id"]), int(q["vert_count"]), int(q["intersection"])] for q in x["matched_gt"]]} for x in v]
         for n, v in pred2gt.items()}
    return g, p


def run_reference(ev, cases, td):
    """-> per layer {scenes: [ints], ap, averages} and the raw matches per layer"""
    out = {}
    for layer, (ir, sr) in LAYER_ROWS.items():
        matches, scenes = {}, []
        for k, (sov, tables, gt, conf, _) in enumerate(cases):
            gt_file = os.path.join(td, "gt_%d.txt" % k)
            if not os.path.exists(gt_file):
                np.savetxt(gt_file, gt_id_vector(gt), fmt="%d")
            info = pred_info(expand(tables, sov, ir), expand(tables, sov, sr), conf)
            g2p, p2g = ev.assign_instances_for_scan("case%d" % k, info, gt_file)
            matches["case%d" % k] = {"gt": g2p, "pred": p2g}
            g, p = ints_of(g2p, p2g)
            scenes.append({"gt2pred": g, "pred2gt": p})
        ap = ev.evaluate_matches(matches)
        avgs = ev.compute_averages(ap)
        out[layer] = {"scenes": scenes, "ap": ap[0].tolist(), "all_ap": float(avgs["all_ap"]), "all_ap_50%": float(avgs["all_ap_50%"]),
                      "all_ap_25%": float(avgs["all_ap_25%"]),
                      "classes": {n: {k: float(v) for k, v in c.items()} for n, c in avgs["classes"].items()}}
    return out


def assert_edge_cases(cases, res):
    """every situation the fixture exists for occurs somewhere in the set"""
    seen = dict.fromkeys(("gt_no_pred", "neither", "small_pred", "small_gt_overlap", "void_label", "double_match", "no_segment", "id_gaps",
                          "conf_tied", "conf_distinct", "ins_without_sem"), False)
    for sov, tables, gt, conf, _ in cases:
        seen["no_segment"] |= bool((sov < 0).any())
        seen["ins_without_sem"] |= bool(((gt[:, 1] > 0) & (gt[:, 0] == 0)).any())
        u = np.unique(conf)
        seen["conf_tied"] |= u.size < conf.size
        seen["conf_distinct"] |= u.size > 1
        for ir, sr in LAYER_ROWS.values():
            ins, sem = expand(tables, sov, ir), expand(tables, sov, sr)
            vals = np.unique(ins[ins > 0])
            seen["id_gaps"] |= bool(vals.size and vals.size < vals.max())
            for v in vals:
                m = ins == v
                seen["small_pred"] |= int(m.sum()) < 100
                seen["void_label"] |= int(sem[np.nonzero(m)[0][0]]) not in CLASS_IDS
    for layer in res.values():
        ap = np.array(layer["ap"])
        seen["gt_no_pred"] |= bool((ap == 0).all(axis=1).any()) and any(
            all(len(sc["pred2gt"][n]) == 0 for sc in layer["scenes"]) and any(len(sc["gt2pred"][n]) for sc in layer["scenes"])
            for n in layer["scenes"][0]["gt2pred"])
        seen["neither"] |= bool(np.isnan(ap).all(axis=1).any())
        for sc in layer["scenes"]:
            for n, preds in sc["pred2gt"].items():
                for p in preds:
                    ious = [(q[2] / (q[1] + p["vert_count"] - q[2]), q[1]) for q in p["matched_gt"]]
                    seen["small_gt_overlap"] |= any(c < 100 for _, c in ious) and all(i <= 0.5 for i, _ in ious)
            for n, gts in sc["gt2pred"].items():
                for g in gts:
                    above = [q for q in g["matched_pred"] if q[2] / (g["vert_count"] + q[1] - q[2]) > 0.25]
                    seen["double_match"] |= g["vert_count"] >= 100 and len(above) >= 2
    missing = [k for k, v in seen.items() if not v]
    assert not missing, "the fixture scenes lack: %s" % missing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SEGGROUP_REFERENCE", "/root/reference"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--scenes", type=int, default=6)
    a = ap.parse_args()
    ev = load_reference(a.reference)
    with tempfile.TemporaryDirectory(prefix="sgap_") as td:
        if a.time:
            cases = [make_case(150000, 1500, 100 + i) for i in range(a.scenes)]
            t0 = time.time()
            for k, (sov, tables, gt, conf, _) in enumerate(cases):
                gt_file = os.path.join(td, "gt_%d.txt" % k)
                np.savetxt(gt_file, gt_id_vector(gt), fmt="%d")
            t_write = time.time() - t0
            per_layer = []
            for layer, (ir, sr) in LAYER_ROWS.items():
                t0 = time.time()
                matches = {}
                for k, (sov, tables, gt, conf, _) in enumerate(cases):
                    info = pred_info(expand(tables, sov, ir), expand(tables, sov, sr), conf)
                    g2p, p2g = ev.assign_instances_for_scan("case%d" % k, info, os.path.join(td, "gt_%d.txt" % k))
                    matches["case%d" % k] = {"gt": g2p, "pred": p2g}
                t1 = time.time()
                ev.compute_averages(ev.evaluate_matches(matches))
                per_layer.append({"layer": layer, "assign_s_per_scene": (t1 - t0) / a.scenes, "evaluate_s_per_scene": (time.time() - t1) / a.scenes})
            tot = sum(x["assign_s_per_scene"] + x["evaluate_s_per_scene"] for x in per_layer)
            print(json.dumps({"vertices": 150000, "segments": 1500, "scenes": a.scenes, "layers": per_layer,
                              "reference_s_per_scene_all_layers": tot, "reference_s_per_scene_and_layer": tot / len(per_layer),
                              "gt_text_write_s_per_scene": t_write / a.scenes}))
            return
        cases = [make_case(V, S, seed) for V, S, seed in SCENES]
        res = run_reference(ev, cases, td)
    assert_edge_cases(cases, res)
    arrays = {}
    for k, (sov, tables, gt, conf, _) in enumerate(cases):
        arrays.update({"sov_%d" % k: sov.astype(np.int32), "tables_%d" % k: tables.astype(np.int32), "gt_%d" % k: gt.astype(np.int32),
                       "conf_%d" % k: conf.astype(np.float64)})
    np.savez_compressed(os.path.join(GOLDEN, "ap_cases.npz"), **arrays)
    with open(os.path.join(GOLDEN, "ap_expected.json"), "w") as f:
        json.dump({"num_scenes": len(cases), "layers": res}, f, separators=(",", ":"))
    print("wrote ap_cases.npz (%d bytes), ap_expected.json (%d bytes)" % (os.path.getsize(os.path.join(GOLDEN, "ap_cases.npz")),
                                                                         os.path.getsize(os.path.join(GOLDEN, "ap_expected.json"))))
    for layer, r in res.items():
        print(layer, "AP %.4f AP50 %.4f AP25 %.4f" % (r["all_ap"], r["all_ap_50%"], r["all_ap_25%"]))


if __name__ == "__main__":
    main()
