"""NumPy restatement of the reference's label colouring (dataset/scannet/util.py:431-527), the yardstick of the visualisation tests.

Closed forms, per vertex, with `palette` the 41-entry colour table (entry 0 white):
  semantic   -1, 0 -> white; l -> palette[l]
  instance   -1, 0 -> white; white where the semantic label is 1 or 2 (when one is given); l -> palette[(l - 1) % 40 + 1]
  segment    -1 -> white; l -> palette[rank % 40 + 1], rank = position of l in np.unique(labels) -- after random.shuffle of that array
             (Python's global generator) when shuffle is set
  adjacency  before colouring: every vertex labelled (!= -1) at the start, in ascending order, hands the value it holds at its turn to
             its neighbours
  grouping   ins != -1 -> palette[rank of ins in np.unique(ins)[1:] % 40 + 1]; otherwise palette[seg * m % 40 + 1], m = 1 or, with
             shuffle, the first np.random.randint(1, 10) after np.random.seed(seed)
tests/test_visualize.py pins this file to the colours captured from the reference itself (tests/golden/visualize_*), without a GPU.
"""
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    with open(os.path.join(GOLDEN, "visualize_cases.json")) as f:
        index = json.load(f)
    arrays = np.load(os.path.join(GOLDEN, "visualize_arrays.npz"))
    return index, arrays


_gold = {}


def case_vector(ref, arrays):
    """The int32 vector a case names: a hand-made array of visualize_arrays.npz or a label vector of another golden file."""
    if "array" in ref:
        return np.asarray(arrays[ref["array"]], dtype=np.int32)
    if ref["golden"] not in _gold:
        _gold[ref["golden"]] = np.load(os.path.join(GOLDEN, ref["golden"] + ".npz"))
    return np.asarray(_gold[ref["golden"]][ref["key"]], dtype=np.int32)


def dilate(labels, adj):
    lab = np.array(labels, copy=True)
    nbr = [[] for _ in range(lab.shape[0])]
    for a, b in np.asarray(adj).reshape(-1, 2):
        nbr[int(a)].append(int(b))
        nbr[int(b)].append(int(a))
    for i in np.nonzero(lab != -1)[0]:
        for j in nbr[i]:
            lab[j] = lab[i]
    return lab


def colour_indices(labels, label_type, shuffle=False, sem=None, adj=None):
    """Palette index [V] of every vertex; draws one random.shuffle from the global generator for a shuffled 'segment' vector."""
    lab = np.asarray(labels, dtype=np.int64)
    if adj is not None:
        lab = dilate(lab, adj)
    if label_type == "segment":
        distinct = np.unique(lab)
        order = list(range(distinct.shape[0]))
        if shuffle:
            random.shuffle(order)                      # the draws of one shuffle depend on the sequence's length only
        pos = np.empty(len(order), dtype=np.int64)
        pos[order] = np.arange(len(order))             # the value of rank order[j] sits at position j afterwards
        idx = pos[np.searchsorted(distinct, lab)] % 40 + 1
        return np.where(lab == -1, 0, idx)
    if label_type == "instance":
        idx = (lab - 1) % 40 + 1
        if sem is not None:
            s = np.asarray(sem)
            idx = np.where((s == 1) | (s == 2), 0, idx)
    elif label_type == "semantic":
        idx = lab.copy()
    else:
        raise ValueError(label_type)
    return np.where((lab == -1) | (lab == 0), 0, idx)


def grouping_indices(ins, seg, shuffle=True, seed=0):
    ins, seg = np.asarray(ins, dtype=np.int64), np.asarray(seg, dtype=np.int64)
    m = 1
    if shuffle:
        np.random.seed(seed)
        m = int(np.random.randint(1, 10))
    rest = np.unique(ins)[1:]
    rank = np.searchsorted(rest, ins)
    return np.where(ins != -1, rank % 40 + 1, seg * m % 40 + 1)


def case_indices(case, arrays):
    """Palette indices of a captured case, with the generators seeded as the capture recorded."""
    if case["fn"] == "grouping":
        return grouping_indices(case_vector(case["ins"], arrays), case_vector(case["seg"], arrays), case["shuffle"], case["seed"])
    if "random_seed" in case:
        random.seed(case["random_seed"])
    return colour_indices(case_vector(case["labels"], arrays), case["label_type"], case["shuffle"],
                          sem=case_vector(case["sem"], arrays) if "sem" in case else None,
                          adj=arrays[case["adj"]] if "adj" in case else None)


def colours(indices, palette):
    return np.asarray(palette, dtype=np.uint8)[np.asarray(indices, dtype=np.int64)]


def patched_block(block, stride, offsets, rgb):
    """The vertex block [V * stride] uint8 with the three colour bytes of every record replaced by rgb [V,3]."""
    out = np.array(block, dtype=np.uint8, copy=True).reshape(-1, stride)
    for ch in range(3):
        out[:, offsets[ch]] = rgb[:, ch]
    return out.reshape(-1)
