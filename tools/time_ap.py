#!/usr/bin/env python3
"""Instance AP, measured: the contingency launch against its HBM byte count with and without the in-wave merge, and
`evaluate --layer all` with and without `--ap` on a tree of `.sgl` scenes.

    python tools/time_ap.py [--vertices 150000] [--segments 1500] [--scenes 8] [--tree-scenes 256] [--reference-json FILE]

The driver touches no GPU itself: every GPU step is a child process of its own under `timeout -k 10`, chained (the first failure ends
the run): `--step call` (wall time of sg_ap_contingency per batch), two `rocprofv3 --kernel-trace --stats` runs of `--step kernel` (vertices
in mesh order / shuffled), `--step evaluate`.  It writes profiles/ap_time.json and profiles/ap_kernel_stats.csv.  Bytes read per contingency
launch: scenes x V x (seg_of_vertex 2 or 4 + gt 8).  --reference-json: the output of `tools/capture_ap.py --time` (the label consumer's own
evaluator on the host CPU of the build container), merged in with the ratio.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def scenes_for(a, order):
    """B scenes in mesh order (a segment's vertices are consecutive: tools/capture_ap.py's generator) or with the vertices shuffled"""
    import capture_ap
    from seggroup_amd.pseudo_labels import PseudoLabels
    out = []
    for i in range(a.scenes):
        sov, tables, gt, _, _ = capture_ap.make_case(a.vertices, a.segments, 200 + i)
        if order == "shuffled":
            perm = np.random.default_rng(i).permutation(a.vertices)
            sov, gt = sov[perm], gt[perm]
        out.append((PseudoLabels(tables, sov), np.ascontiguousarray(gt, dtype=np.int32)))
    return out


def step_call(a):
    import torch
    from seggroup_amd import ap
    res = {"device": torch.cuda.get_device_name(0)}
    for order in ("mesh", "shuffled"):
        sc = scenes_for(a, order)
        items, gts = [p for p, _ in sc], [g for _, g in sc]
        for name, flags in (("merge", 0), ("plain", 1)):
            for _ in range(2):
                conts = ap.contingency_batch(items, gts, flags=flags)
            t = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                ap.contingency_batch(items, gts, flags=flags)
                t.append(time.perf_counter() - t0)
            res["call_%s_%s_ms" % (order, name)] = round(float(np.median(t)) * 1e3, 3)
        res["triples_per_scene_" + order] = int(np.mean([c.triples.shape[0] for c in conts]))
        res["d2h_bytes_per_scene_" + order] = int(np.mean([c.triples.nbytes + c.first_vertex.nbytes + c.gt.nbytes for c in conts]))
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            for c, p in zip(conts, items):
                for ir, sr in ((1, 2), (4, 5), (7, 8), (10, 11), (12, 13)):
                    ap.layer_matches(c, p.tables[ir], p.tables[sr])
            t.append(time.perf_counter() - t0)
        res["host_fold_match_ms_per_scene_and_layer_" + order] = round(float(np.median(t)) * 1e3 / (5 * len(items)), 4)
    print(json.dumps(res))


def step_kernel(a):
    from seggroup_amd import ap
    sc = scenes_for(a, a.order)
    items, gts = [p for p, _ in sc], [g for _, g in sc]
    for width in (2, 4):
        for flags in (0, 1):
            for _ in range(a.iters):
                ap.contingency_batch(items, gts, flags=flags, sov_width=width)
    print(json.dumps({"ok": True}))


def step_evaluate(a):
    import io
    from contextlib import redirect_stdout
    import torch
    from seggroup_amd import evaluate, pseudo_labels
    import capture_ap
    res = {"tree_scenes": a.tree_scenes}
    with tempfile.TemporaryDirectory(prefix="sgap_tree_") as root:
        names = ["scene%04d_00" % i for i in range(a.tree_scenes)]
        os.makedirs(os.path.join(root, "dataset", "scannet"))
        with open(os.path.join(root, "dataset", "scannet", "scannetv2_train.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
        for i, s in enumerate(names):                           # 8 distinct scenes, the others link to them
            lab = os.path.join(root, "dataset", "scannet", "label", "real", "raw", s)
            exp = os.path.join(root, "results", "exp", s, "ins_infer")
            os.makedirs(lab)
            os.makedirs(exp)
            if i < 8:
                sov, tables, gt, _, _ = capture_ap.make_case(a.vertices, a.segments, 300 + i)
                torch.save(torch.from_numpy(gt.astype(np.int64)), os.path.join(lab, s + ".label.pth"))
                pseudo_labels.write(exp, tables, sov)
            else:
                os.symlink(os.path.join(root, "dataset", "scannet", "label", "real", "raw", names[i % 8], names[i % 8] + ".label.pth"),
                           os.path.join(lab, s + ".label.pth"))
                os.symlink(os.path.join(root, "results", "exp", names[i % 8], "ins_infer", pseudo_labels.SGL_NAME), os.path.join(exp, pseudo_labels.SGL_NAME))
        for name, extra in (("plain", []), ("ap", ["--ap"])):
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    evaluate.main(["-n", "exp", "--stage", "ins_infer", "--root", root, "--layer", "all", "--format", "sgl", "--batch", str(a.batch)] + extra)
                t.append(time.perf_counter() - t0)
            res["evaluate_all_layers_%s_s" % name] = round(float(np.median(t)), 4)
    res["ap_part_ms_per_scene_all_layers"] = round((res["evaluate_all_layers_ap_s"] - res["evaluate_all_layers_plain_s"]) * 1e3 / a.tree_scenes, 4)
    print(json.dumps(res))


def kernel_rows(d):
    """rows of rocprofv3's kernel stats (Name, Calls, TotalDurationNs, AverageNs, ...) for the k_ap_ kernels"""
    fs = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not fs:
        raise SystemExit("no kernel stats under " + d)
    rows = []
    with open(fs[-1]) as f:
        for r in csv.DictReader(f):
            if "k_ap_" in r["Name"]:
                rows.append(dict(name=r["Name"], calls=int(r["Calls"]), total_ns=int(float(r["TotalDurationNs"])), avg_ns=float(r["AverageNs"]),
                                 min_ns=int(float(r["MinNs"])), max_ns=int(float(r["MaxNs"]))))
    return rows


def child(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=REPO, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("step failed with exit status %d: %s" % (r.returncode, " ".join(cmd)))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else {}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--vertices", type=int, default=150000)
    p.add_argument("--segments", type=int, default=1500)
    p.add_argument("--scenes", type=int, default=8)
    p.add_argument("--tree-scenes", type=int, default=256)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--order", default="mesh", choices=["mesh", "shuffled"])
    p.add_argument("--step", default=None, choices=["call", "kernel", "evaluate"])
    p.add_argument("--reference-json", default=None)
    p.add_argument("--step-limit", type=int, default=None, help="seconds every GPU step may take (default: 300 / 300 / 300 / 900)")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ap_time.json"))
    p.add_argument("--stats-out", default=os.path.join(REPO, "profiles", "ap_kernel_stats.csv"))
    a = p.parse_args()
    if a.step:
        return {"call": step_call, "kernel": step_kernel, "evaluate": step_evaluate}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__), "--vertices", str(a.vertices), "--segments", str(a.segments), "--scenes", str(a.scenes),
          "--tree-scenes", str(a.tree_scenes), "--batch", str(a.batch), "--iters", str(a.iters)]
    res = dict(vertices=a.vertices, segments=a.segments, scenes=a.scenes)
    res.update(child(me + ["--step", "call"], a.step_limit or 300))
    stats = []
    with tempfile.TemporaryDirectory(prefix="sgap_prof_") as td:
        for order in ("mesh", "shuffled"):
            d = os.path.join(td, order)
            child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"] + me + ["--step", "kernel", "--order", order], a.step_limit or 300)
            for r in kernel_rows(d):
                r["order"] = order
                stats.append(r)
    for r in stats:
        if "k_ap_contingency" in r["name"] and ("ILi2E" in r["name"] or "<2," in r["name"] or "ILi4E" in r["name"] or "<4," in r["name"]):
            width = 2 if ("ILi2E" in r["name"] or "<2," in r["name"]) else 4
            merge = "Lb1E" in r["name"] or "true" in r["name"]
            nbytes = a.scenes * a.vertices * (width + 8)
            res["contingency_%s_sov%d_%s" % (r["order"], width * 8, "merge" if merge else "plain")] = dict(
                us_per_launch=round(r["avg_ns"] / 1e3, 2), us_min=round(r["min_ns"] / 1e3, 2), bytes_per_launch=nbytes,
                tb_per_s=round(nbytes / r["avg_ns"] / 1e3, 3), calls=r["calls"])
    res.update(child(me + ["--step", "evaluate"], a.step_limit or 900))
    if a.reference_json:
        ref = json.load(open(a.reference_json))
        res["reference_evaluator_host_cpu"] = ref
        res["reference_over_ap_part"] = round(ref["reference_s_per_scene_all_layers"] * 1e3 / max(res["ap_part_ms_per_scene_all_layers"], 1e-9), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    with open(a.stats_out, "w") as f:
        f.write("# k_ap_* kernels, %d scenes of %d vertices / %d segments per launch; source: rocprofv3 --kernel-trace --stats of tools/time_ap.py --step kernel\n"
                % (a.scenes, a.vertices, a.segments))
        f.write("order,name,calls,total_ns,avg_ns,min_ns,max_ns\n")
        for r in stats:
            f.write('%s,"%s",%d,%d,%.1f,%d,%d\n' % (r["order"], r["name"], r["calls"], r["total_ns"], r["avg_ns"], r["min_ns"], r["max_ns"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
