#!/usr/bin/env python3
"""Re-score saved pseudo labels of any layer and any stage: the working counterpart of the reference's `seggroup/evaluate.py`.

    python -m seggroup_amd.evaluate -n EXP [--layer 1|2|3|4|final|all] [--stage epoch_last] [--root .] [--scenes LIST]
                                    [--format auto|sgl|npy|txt] [--json PATH] [--ap]

Reads `results/<exp>/<scene>/<stage>/` of every scene in the list: `pseudo_labels.sgl` (seggroup_amd/pseudo_labels.py), or the per-vector
`layer_<k>.{ins,sem}` / `final.{ins,sem}` files as `.npy` or `.txt`; `--format auto` takes the first of those three a scene has.  Ground
truth comes from the scene's pack when it is current (cache.is_current), else from `label/real/raw/<s>/<s>.label.pth`.

Semantics are model.py:608-655's (what `sg_evaluate` and the NumPy oracle pin): only vertices with GT semantic label != 0 count,
instance -1 is skipped, every predicted instance takes the semantic label of its first valid vertex (a negative class slot wraps),
instance ids are checked against the class-id lists, an empty set gives NaN accuracy.  So `--layer final` on an ins_infer run (and
`--layer 2` on a sem_infer run: that forward is scored at layer 2, model.py:781-783) reproduces the summary infer.py logged.
Deviations from the reference script, on purpose:
  * its instance loop also counts instance -1 as an instance; this one does not (as model.py's evaluate, which infer.py reports);
  * its `--stage` default `last` names no directory the reference writes (it writes `epoch_<n>`, `epoch_last`, `ins_infer`,
    `sem_infer`): the default here is `epoch_last`;
  * `--layer all` (every layer the files hold in one pass) and `--format` / `--json` are additions.
`.sgl` inputs are evaluated from their tables on the GPU (`sg_eval_tables`: every layer in one pass over a scene's vertices);
`.npy` / `.txt` vectors through `sg_evaluate` per scene and layer.  All three give identical accumulators.
`--ap` adds the ScanNet instance benchmark's AP / AP_50% / AP_25% over the 18 instance classes under each layer's report (seggroup_amd/ap.py,
DESIGN.md 9d: all vertices count, confidence 1.0 for every instance): one `sg_ap_contingency` pass per `.sgl` scene serves every layer, the
vector formats take one `sg_ap_contingency_vectors` pass per layer.  sem_infer directories hold no instance grouping beyond layer 2, so AP
is defined there for layers 1 and 2 only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import hip
from .infer import Accumulator, final_report

# layer -> (ins row, sem row) in hip.LABEL_NAMES order, and the file stems
LAYER_ROWS = {"1": (1, 2), "2": (4, 5), "3": (7, 8), "4": (10, 11), "final": (12, 13)}
LAYERS_OF_MODE = {"ins": ["1", "2", "3", "4", "final"], "sem": ["1", "2"]}
FORMATS = ("sgl", "npy", "txt")


def stem(layer: str) -> str:
    return "final" if layer == "final" else "layer_%s" % layer


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Evaluate saved pseudo labels")
    p.add_argument("-n", "--exp_name", required=True, type=str, help="Name of the experiment.")
    p.add_argument("--layer", type=str, default="final", choices=["1", "2", "3", "4", "final", "all"], help="Layer to evaluate (all = every layer the files hold).")
    p.add_argument("--stage", type=str, default="epoch_last",
                   help="Directory of the run: epoch_N | epoch_last | ins_infer | sem_infer (the reference's default 'last' names none).")
    p.add_argument("--root", type=str, default=".", help="directory holding dataset/ and results/ (default: CWD)")
    p.add_argument("--scenes", type=str, default=None, help="scene list (default: <root>/dataset/scannet/scannetv2_train.txt)")
    p.add_argument("--format", type=str, default="auto", choices=["auto"] + list(FORMATS), help="label files to read (auto: sgl, then npy, then txt)")
    p.add_argument("--json", type=str, default=None, help="write the per-layer accumulators (165 float64 sums) to this file")
    p.add_argument("--label_style", type=str, default="manual", help="label style of the scene packs the ground truth is read from")
    p.add_argument("--batch", type=int, default=64, help="scenes per GPU launch")
    p.add_argument("-j", "--workers", type=int, default=8, help="threads reading label and ground-truth files")
    p.add_argument("--ap", action="store_true", help="also print ScanNet instance AP / AP_50%% / AP_25%% per layer (and an \"ap\" object in --json)")
    return p


def scene_names(root: str, scenes: Optional[str]) -> List[str]:
    path = scenes or os.path.join(root, "dataset", "scannet", "scannetv2_train.txt")
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def find_format(d: str, fmt: str = "auto") -> Optional[Tuple[str, str]]:
    """(format, mode) of the labels in export directory `d`, or None.  mode 'ins' (14 vectors, final.* present) or 'sem' (6)."""
    from . import pseudo_labels
    for f in (FORMATS if fmt == "auto" else (fmt,)):
        if f == "sgl":
            p = os.path.join(d, pseudo_labels.SGL_NAME)
            if os.path.isfile(p):
                h = pseudo_labels.read_header(p)
                return "sgl", "ins" if h["nvec"] == pseudo_labels.INS_NVEC else "sem"
        elif os.path.isfile(os.path.join(d, "layer_1.ins." + f)):
            return f, "ins" if os.path.isfile(os.path.join(d, "final.ins." + f)) else "sem"
    return None


def discover(root: str, exp: str, stage: str, names: Sequence[str], fmt: str, layer: str, ap: bool = False):
    """-> ([(scene, directory, format, mode)], layers to evaluate).  Raises SystemExit naming every scene without labels, and when the
    requested layer does not exist in a scene's mode (sem_infer files stop at layer 2)."""
    found, missing = [], []
    for s in names:
        d = os.path.join(root, "results", exp, s, stage)
        ff = find_format(d, fmt)
        if ff is None:
            missing.append(s)
        else:
            found.append((s, d, ff[0], ff[1]))
    if missing:
        shown = ", ".join(missing[:20]) + (" ... (%d more)" % (len(missing) - 20) if len(missing) > 20 else "")
        raise SystemExit("no %s labels under results/%s/<scene>/%s for %d of %d scenes: %s" % (
            "sgl / npy / txt" if fmt == "auto" else fmt, exp, stage, len(missing), len(names), shown))
    modes = sorted({m for (_, _, _, m) in found})
    if len(modes) > 1:
        raise SystemExit("results/%s/*/%s mixes ins_infer (14 vectors) and sem_infer (6 vectors) labels" % (exp, stage))
    mode = modes[0] if modes else "ins"
    if layer == "all":
        layers = LAYERS_OF_MODE[mode]
    else:
        if layer not in LAYERS_OF_MODE[mode]:
            raise SystemExit("--layer %s: the labels under results/%s/*/%s are sem_infer labels (layers 1 and 2 only; that forward returns "
                             "after layer 2, model.py:781-783)%s" % (layer, exp, stage, "; they hold no instance grouping beyond layer 2, so "
                                                                    "--ap is defined for --layer 1, 2 or all there" if ap else ""))
        layers = [layer]
    return found, layers


def load_gt(root: str, scene: str, label_style: str = "manual") -> np.ndarray:
    """[V,2] int32 (sem, ins) ground truth: the pack's copy when the pack is current, else the raw `.label.pth`."""
    from . import cache
    if cache.is_current(root, scene, label_style):
        return np.ascontiguousarray(cache.read_pack(cache.pack_path(root, scene, label_style))["gt"], dtype=np.int32)
    from .pth import load_tensor
    return np.ascontiguousarray(load_tensor(os.path.join(root, "dataset", "scannet", "label", "real", "raw", scene, scene + ".label.pth")),
                                dtype=np.int32)


def read_vector(d: str, name: str, fmt: str) -> np.ndarray:
    path = os.path.join(d, name + "." + fmt)
    if fmt == "npy":
        return np.ascontiguousarray(np.load(path), dtype=np.int32)
    with open(path, "rb") as f:
        return np.array(f.read().split(), dtype=np.int32)


def load_scene(job):
    """One scene's inputs on the host: (scene, gt, format, PseudoLabels | {layer: (ins, sem)})."""
    (s, d, fmt, _mode), layers, root, label_style = job
    gt = load_gt(root, s, label_style)
    if fmt == "sgl":
        from . import pseudo_labels
        lab = pseudo_labels.load(d)
        if lab.V != gt.shape[0]:
            raise ValueError("%s: %d vertices in the labels, %d in the ground truth" % (s, lab.V, gt.shape[0]))
    else:
        lab = {l: (read_vector(d, stem(l) + ".ins", fmt), read_vector(d, stem(l) + ".sem", fmt)) for l in layers}
        for l, (ins, sem) in lab.items():
            if ins.shape[0] != gt.shape[0] or sem.shape[0] != gt.shape[0]:
                raise ValueError("%s: layer %s has %d / %d values for %d vertices" % (s, l, ins.shape[0], sem.shape[0], gt.shape[0]))
    return s, gt, fmt, lab


def eval_tables_batch(items, gts: Sequence[np.ndarray], layers: Sequence[str], device) -> np.ndarray:
    """sg_eval_tables over B scenes: -> float32 [B, L, 164] = iou_sem [80] | iou_ins [80] | acc [4] per scene and layer."""
    import torch
    from .pseudo_labels import pack_for_device, upload
    tab_all, sov_all, width, desc = pack_for_device(items)
    rows = np.array([r for l in layers for r in LAYER_ROWS[l]], dtype=np.int32)
    B, L = len(items), len(layers)
    h_desc = np.zeros((B, 6), dtype=np.int64)
    for b, (p, (t_off, S, s_off, V)) in enumerate(zip(items, desc)):
        ins_max = int(max(p.tables[LAYER_ROWS[l][0]].max() for l in layers))
        h_desc[b] = (t_off, S, s_off, V, s_off, max(ins_max + 1, 1))
    if any(np.asarray(g).shape[0] != p.V for p, g in zip(items, gts)):
        raise ValueError("eval_tables_batch: a scene's ground truth and labels differ in vertex count")
    gt_all = np.concatenate([np.ascontiguousarray(g, dtype=np.int32).reshape(-1, 2) for g in gts]) if B else np.zeros((0, 2), np.int32)
    lib = hip.lib()
    ws_bytes = lib.sg_eval_tables_ws_bytes(B, L, h_desc.ctypes.data)
    out_sem = np.zeros((B, L, 80), np.float32)
    out_ins = np.zeros((B, L, 80), np.float32)
    out_acc = np.zeros((B, L, 4), np.float32)
    with torch.cuda.device(device):
        g_tab, g_sov = upload(tab_all, device), upload(sov_all if sov_all.size else np.zeros(1, sov_all.dtype), device)
        g_gt = upload(gt_all if gt_all.size else np.zeros((1, 2), np.int32), device)
        ws = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device=device)
        st = torch.cuda.current_stream(device).cuda_stream
        hip.check(lib.sg_eval_tables(B, h_desc.ctypes.data, g_tab.data_ptr(), items[0].tables.shape[0], g_sov.data_ptr(), width, g_gt.data_ptr(),
                                     L, rows.ctypes.data, out_sem.ctypes.data, out_ins.ctypes.data, out_acc.ctypes.data, ws.data_ptr(),
                                     int(ws.numel()), st))
    return np.concatenate([out_sem, out_ins, out_acc], axis=2)


def eval_vectors(gt: np.ndarray, lab, layers: Sequence[str], device) -> np.ndarray:
    """sg_evaluate per layer on uploaded vectors: -> float32 [L, 164]."""
    import torch
    lib = hip.lib()
    out = np.zeros((len(layers), 164), np.float32)
    with torch.cuda.device(device):
        st = torch.cuda.current_stream(device).cuda_stream
        g_gt = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.int32)).to(device)
        for k, l in enumerate(layers):
            ins, sem = lab[l]
            max_ins = max(int(ins.max()) + 1 if ins.size else 1, 1)
            ws = torch.empty(int(lib.sg_eval_ws_bytes(max_ins)), dtype=torch.uint8, device=device)
            g_ins, g_sem = torch.from_numpy(ins).to(device), torch.from_numpy(sem).to(device)
            a_sem, a_ins, a_acc = np.zeros(80, np.float32), np.zeros(80, np.float32), np.zeros(4, np.float32)
            hip.check(lib.sg_evaluate(g_gt.data_ptr(), g_sem.data_ptr(), g_ins.data_ptr(), gt.shape[0], max_ins, a_sem.ctypes.data,
                                      a_ins.ctypes.data, a_acc.ctypes.data, ws.data_ptr(), int(ws.numel()), st))
            out[k] = np.concatenate([a_sem, a_ins, a_acc])
    return out


def ap_tables_batch(items, gts: Sequence[np.ndarray], layers: Sequence[str], device) -> list:
    """sg_ap_contingency over B scenes, then every layer's fold and matching on the host: -> [B][L] ap.Matches."""
    from . import ap
    conts = ap.contingency_batch(items, gts, device)
    return [[ap.layer_matches(c, p.tables[LAYER_ROWS[l][0]], p.tables[LAYER_ROWS[l][1]]) for l in layers] for c, p in zip(conts, items)]


def ap_vectors(gt: np.ndarray, lab, layers: Sequence[str], device) -> list:
    """sg_ap_contingency_vectors per layer on uploaded vectors: -> [L] ap.Matches."""
    import torch
    from . import ap
    g = np.ascontiguousarray(gt, dtype=np.int32).reshape(-1, 2)
    g_gt = torch.from_numpy(g if g.size else np.zeros((1, 2), np.int32)).to(device)
    out = []
    for l in layers:
        ins, sem = lab[l]
        cont = ap.contingency_vector(ins, gt, device, g_gt=g_gt)
        out.append(ap.layer_matches(cont, *ap.vector_rows(cont, sem)))
    return out


def report_ap(accs: Dict[str, Accumulator], ap_accs, exp: str, stage: str, sem_mode: bool) -> dict:
    """Each layer's report followed by its AP table; -> {layer: the "ap" object of --json}."""
    from . import ap
    out = {}
    for l in accs:
        report({l: accs[l]}, exp, stage)
        avgs = ap.compute_averages(ap_accs[l].ap())
        print("Instance AP, layer %s  (%d scenes, 18 classes, AP = mean over IoU 0.50:0.05:0.90, every instance with confidence 1)" % (l, ap_accs[l].scenes))
        for ln in ap.report_lines(avgs):
            print(ln)
        out[l] = ap.to_json(avgs)
    if sem_mode:
        print("note: sem_infer labels hold no instance grouping beyond layer 2: AP is defined for layers 1 and 2 only")
    return out


def accumulate(per_scene: Sequence[np.ndarray], layers: Sequence[str]) -> Dict[str, Accumulator]:
    """per_scene[i] = float32 [L, 164] of scene i (scene-list order) -> one Accumulator per layer (the float64 sums infer.py forms)."""
    accs = {l: Accumulator() for l in layers}
    for m in per_scene:
        for k, l in enumerate(layers):
            accs[l].add(m[k, 0:80], m[k, 80:160], m[k, 160:164])
    return accs


class _Print:
    def cprint(self, text):
        print(text)


def report(accs: Dict[str, Accumulator], exp: str, stage: str, io=None) -> None:
    """Per layer: a heading, then infer.py's summary ('==> Infer' line and the per-class tables)."""
    io = io or _Print()
    for l, acc in accs.items():
        io.cprint("Layer %s  (results/%s/*/%s, %d scenes)" % (l, exp, stage, int(acc.v[164])))
        final_report(acc.summary(), io)


def to_json(accs: Dict[str, Accumulator], exp: str, stage: str, formats: Dict[str, int], elapsed: float) -> dict:
    return {"exp_name": exp, "stage": stage, "formats": formats, "elapsed_s": elapsed,
            "layers": {l: {"v": a.v.tolist(), "n": int(a.v[164])} for l, a in accs.items()}}


def run(args) -> Dict[str, Accumulator]:
    import torch
    names = scene_names(args.root, args.scenes)
    want_ap = bool(getattr(args, "ap", False))
    found, layers = discover(args.root, args.exp_name, args.stage, names, args.format, args.layer, want_ap)
    if not torch.cuda.is_available():
        raise SystemExit("seggroup_amd.evaluate runs its counting on the GPU (no CPU fallback)")
    hip.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    t0 = time.time()
    jobs = [((f, layers, args.root, args.label_style)) for f in found]
    batches = [jobs[k:k + max(1, args.batch)] for k in range(0, len(jobs), max(1, args.batch))]
    per_scene: List[np.ndarray] = []
    ap_scene: list = []
    fmt_count: Dict[str, int] = {}
    with ThreadPoolExecutor(max_workers=max(1, args.workers)) as pool:
        nxt = pool.map(load_scene, batches[0]) if batches else None
        for bi in range(len(batches)):
            loaded = list(nxt)
            if bi + 1 < len(batches):
                nxt = pool.map(load_scene, batches[bi + 1])         # the next batch's files are read while this one is on the GPU
            sgl = [(i, x) for i, x in enumerate(loaded) if x[2] == "sgl"]
            res: List[Optional[np.ndarray]] = [None] * len(loaded)
            if sgl:
                m = eval_tables_batch([x[3] for _, x in sgl], [x[1] for _, x in sgl], layers, dev)
                for k, (i, _) in enumerate(sgl):
                    res[i] = m[k]
            for i, x in enumerate(loaded):
                fmt_count[x[2]] = fmt_count.get(x[2], 0) + 1
                if res[i] is None:
                    res[i] = eval_vectors(x[1], x[3], layers, dev)
            per_scene.extend(res)
            if want_ap:
                apm: list = [None] * len(loaded)
                if sgl:
                    for (i, _), m in zip(sgl, ap_tables_batch([x[3] for _, x in sgl], [x[1] for _, x in sgl], layers, dev)):
                        apm[i] = m
                ap_scene.extend(m if m is not None else ap_vectors(x[1], x[3], layers, dev) for m, x in zip(apm, loaded))
    accs = accumulate(per_scene, layers)
    ap_json = None
    if want_ap:
        from . import ap
        ap_accs = {l: ap.APAccumulator() for l in layers}
        for m in ap_scene:
            for k, l in enumerate(layers):
                ap_accs[l].add(m[k])
    elapsed = time.time() - t0
    if want_ap:
        ap_json = report_ap(accs, ap_accs, args.exp_name, args.stage, bool(found) and found[0][3] == "sem")
    else:
        report(accs, args.exp_name, args.stage)
    print("evaluated %d scenes x %d layer(s) in %.3f s (%s)" % (len(found), len(layers), elapsed, ", ".join("%s %d" % kv for kv in sorted(fmt_count.items()))))
    if args.json:
        with open(args.json, "w") as f:
            js = to_json(accs, args.exp_name, args.stage, fmt_count, elapsed)
            if ap_json is not None:
                for l, a in ap_json.items():
                    js["layers"][l]["ap"] = a
            json.dump(js, f)
    return accs


def main(argv=None):
    np.seterr(divide="ignore", invalid="ignore")
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
