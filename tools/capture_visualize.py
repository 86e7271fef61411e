#!/usr/bin/env python3
"""Golden colours of the reference's label visualisation (build container only): runs the UNMODIFIED visualize_labels and
visualize_grouping_process of the reference's dataset/scannet/util.py (located by tools/capture_prepare.py, chainer / plyfile stubbed)
with a stand-in for the `plydata` object, on
  * the committed label vectors of tests/golden/{tiny_4k,tiny_dup_4k,small_20k}.npz (`ins.label.*`, `sem.label.*`: seg as 'segment' --
    plain, and for layers 2-4 also shuffled under a seeded global `random` --, ins as 'instance', sem as 'semantic'), and
  * hand-made vectors for the corners: a -1 and a 0 among segment labels, more than 40 distinct values, instance labels with a semantic
    file that holds classes 1 and 2, every semantic class, an `adj_path` case in which labelled vertices share neighbours, and the
    grouping process with shuffle on / off and seeds 0 and 3.
Only recorded DATA is stored: the inputs' names or arrays, the generator seeds, the resulting [V,3] uint8 colours, the output path each
call chose (relative to the directory of the label file), the reference's colour table as a list and its functions' parameter names and
defaults.  -> tests/golden/visualize_cases.json + visualize_arrays.npz.  Nothing of the reference's text is copied.
usage: python tools/capture_visualize.py"""
import inspect
import json
import os
import random
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import capture_prepare as cp  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SCENES = ("tiny_4k", "tiny_dup_4k", "small_20k")
TYPE_OF = {"seg": "segment", "ins": "instance", "sem": "semantic"}


class _Column:
    def __init__(self, n):
        self.a = np.zeros(n, dtype=np.uint8)

    def __setitem__(self, i, v):
        self.a[i] = v


class _Vertex:
    def __init__(self, n):
        self.count = n
        self.cols = {k: _Column(n) for k in ("red", "green", "blue")}

    def __getitem__(self, k):
        return self.cols[k]


class FakePly:
    """What the two functions need of plyfile.PlyData: ['vertex'].count, ['vertex'][channel][i] = value, .write(path)."""

    def __init__(self, n):
        self.vertex = _Vertex(n)
        self.written = None

    def __getitem__(self, k):
        assert k == "vertex"
        return self.vertex

    def write(self, path):
        self.written = path

    def colours(self):
        return np.stack([self.vertex.cols[k].a for k in ("red", "green", "blue")], 1)


def hand_made():
    """name -> int32 vector (or [E,2] adjacency): the corner cases"""
    rng = np.random.default_rng(20)
    a = {}
    seg = rng.integers(0, 63, 700) * 3 + 5                 # 63 distinct values: rank % 40 wraps
    seg[rng.integers(0, 700, 40)] = -1                     # a -1 that occurs counts as rank 0
    seg[rng.integers(0, 700, 40)] = 0                      # 0 is a label like any other for 'segment'
    a["hand.seg_wrap"] = seg
    a["hand.seg_no_minus1"] = rng.integers(0, 45, 500) * 7
    ins = rng.integers(-1, 90, 900)
    a["hand.ins"] = ins
    a["hand.ins_sem"] = rng.integers(0, 6, 900)            # classes 1 and 2 whiten the instance colour
    a["hand.sem_all"] = np.concatenate([np.arange(-1, 41), rng.integers(-1, 41, 400)])
    # adj_path: 1,500 vertices, 60 labelled ones; a band graph (i, i+1), (i, i+7) plus random pairs, a self-loop and a repeated pair, so
    # labelled vertices share neighbours and later propagations see earlier ones
    V = 1500
    lab = np.full(V, -1)
    src = rng.choice(V, 60, replace=False)
    lab[src] = rng.integers(1, 30, 60)
    i = np.arange(V - 7)
    adj = np.concatenate([np.stack([i, i + 1], 1), np.stack([i + 7, i], 1), rng.integers(0, V, (300, 2)), [[5, 5], [10, 11], [10, 11]]])
    a["hand.adj_labels"] = lab
    a["hand.adj_pairs"] = adj
    gi = rng.integers(0, 50, 1200) * 2 + 1
    gi[rng.integers(0, 1200, 500)] = -1
    a["hand.group_ins"] = gi
    a["hand.group_seg"] = rng.integers(0, 300, 1200)
    return {k: np.asarray(v, dtype=np.int32) for k, v in a.items()}


def main():
    import torch
    util = cp._load_reference_util()
    if not hasattr(np, "bool"):
        np.bool = bool                                      # the adj_path branch spells the dtype the pre-1.24 way
    arrays = hand_made()
    gold = {s: np.load(os.path.join(GOLD, s + ".npz")) for s in SCENES}

    def vector(ref):
        return arrays[ref["array"]] if "array" in ref else gold[ref["golden"]][ref["key"]]

    cases = []
    for s in SCENES:
        for key in [k for k in gold[s].files if ".label." in k]:
            kind = TYPE_OF[key.rsplit(".", 1)[1]]
            cases.append(dict(fn="labels", labels=dict(golden=s, key=key), label_type=kind, shuffle=False))
            if kind == "segment" and ".layer_1." not in key:
                cases.append(dict(fn="labels", labels=dict(golden=s, key=key), label_type=kind, shuffle=True, random_seed=len(cases)))
    H = lambda n: dict(array=n)                             # noqa: E731
    cases += [
        dict(fn="labels", labels=H("hand.seg_wrap"), label_type="segment", shuffle=False),
        dict(fn="labels", labels=H("hand.seg_wrap"), label_type="segment", shuffle=True, random_seed=7),
        dict(fn="labels", labels=H("hand.seg_no_minus1"), label_type="segment", shuffle=False),
        dict(fn="labels", labels=H("hand.seg_no_minus1"), label_type="segment", shuffle=True, random_seed=8),
        dict(fn="labels", labels=H("hand.seg_wrap"), label_type="instance", shuffle=False),
        dict(fn="labels", labels=H("hand.ins"), label_type="instance", shuffle=False),
        dict(fn="labels", labels=H("hand.ins"), label_type="instance", shuffle=False, sem=H("hand.ins_sem")),
        dict(fn="labels", labels=H("hand.sem_all"), label_type="semantic", shuffle=False),
        dict(fn="labels", labels=H("hand.adj_labels"), label_type="instance", shuffle=False, adj="hand.adj_pairs"),
        dict(fn="labels", labels=H("hand.adj_labels"), label_type="segment", shuffle=True, random_seed=9, adj="hand.adj_pairs"),
        dict(fn="grouping", ins=H("hand.group_ins"), seg=H("hand.group_seg"), shuffle=False, seed=0),
        dict(fn="grouping", ins=H("hand.group_ins"), seg=H("hand.group_seg"), shuffle=True, seed=0),
        dict(fn="grouping", ins=H("hand.group_ins"), seg=H("hand.group_seg"), shuffle=True, seed=3),
    ]

    def write_txt(path, vec):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("".join("%d\n" % v for v in vec))

    with tempfile.TemporaryDirectory(prefix="sgvis_") as td:
        for ci, c in enumerate(cases):
            d = os.path.join(td, "case%03d" % ci, "epoch_1")
            if c["fn"] == "labels":
                vec = vector(c["labels"])
                name = c["labels"].get("key", c["labels"].get("array")).split("label.")[-1] + ".txt"
                write_txt(os.path.join(d, name), vec)
                sem_path = adj_path = None
                if "sem" in c:
                    sem_path = os.path.join(d, "sem_for_ins.txt")
                    write_txt(sem_path, vector(c["sem"]))
                if "adj" in c:
                    adj_path = os.path.join(d, "adj.pth")
                    torch.save(torch.from_numpy(arrays[c["adj"]].astype(np.int64)), adj_path)
                ply = FakePly(len(vec))
                if "random_seed" in c:
                    random.seed(c["random_seed"])
                util.visualize_labels("unused.ply", os.path.join(d, name), c["label_type"], plydata=ply, shuffle=c["shuffle"], adj_path=adj_path,
                                      sem_labels=sem_path)
                c["label_file"] = name
            else:
                write_txt(os.path.join(d, "grouping.ins.txt"), vector(c["ins"]))
                write_txt(os.path.join(d, "grouping.seg.txt"), vector(c["seg"]))
                ply = FakePly(len(vector(c["ins"])))
                util.visualize_grouping_process("unused.ply", os.path.join(d, "grouping.ins.txt"), os.path.join(d, "grouping.seg.txt"), plydata=ply,
                                                shuffle=c["shuffle"], seed=c["seed"])
                c["label_file"] = "grouping.seg.txt"
            c["output"] = os.path.relpath(ply.written, d)
            c["colours"] = "colours.%03d" % ci
            arrays[c["colours"]] = ply.colours()
            print(ci, c["fn"], c.get("label_type", ""), c["output"], "distinct colours", len(np.unique(arrays[c["colours"]], axis=0)), flush=True)

    def params(fn):
        return [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.default is not inspect.Parameter.empty]
                for p in inspect.signature(fn).parameters.values()]

    index = dict(colors=[list(map(int, c)) for c in util.colors], num_colors=int(util.num_colors),
                 signatures=dict(visualize_labels=params(util.visualize_labels), visualize_grouping_process=params(util.visualize_grouping_process)),
                 cases=cases)
    with open(os.path.join(GOLD, "visualize_cases.json"), "w") as f:
        json.dump(index, f, indent=1)
    np.savez_compressed(os.path.join(GOLD, "visualize_arrays.npz"), **arrays)
    print(len(cases), "cases;", os.path.getsize(os.path.join(GOLD, "visualize_arrays.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
