"""Non-maximum suppression of upright boxes restated: the rule of include/seggroup_hip.h in plain loops.  The order is a
plain sort on (-score, index) with -0.0 normalised; the IoU of every ordered pair (the earlier box as `a`) comes from
boxap_ref.pair_iou -- imported, not copied --, evaluated only where the z intervals overlap by the header's own two statements (the
others are 0 by the sequence); the greedy pass is loops.  It never calls the library.  `proposals` is the generator the tests use:
uniform random boxes hardly ever chain."""
import math

import numpy as np

import boxap_ref as A

F64 = np.float64


def offsets(off, k):
    return np.array([0, k], np.int64) if off is None else np.asarray(off, np.int64)


def words(off) -> int:
    """the 64-bit words of the bit matrix: the sum over the scenes of n * ceil(n / 64)"""
    n = np.diff(np.asarray(off, np.int64))
    return int((n * ((n + 63) // 64)).sum())


def order_of(score):
    """the visiting order of one scene: i before j iff s_i > s_j, or s_i == s_j and i < j"""
    s = np.asarray(score, F64) + 0.0                                         # -0.0 + 0.0 = 0.0: the two zeros tie
    return sorted(range(s.shape[0]), key=lambda i: (-s[i], i))


def ordered_iou(rows):
    """rows [n,8] in visiting order -> float64 [n,n]: entry (i, j), i < j, = pair_iou(a = row i, b = row j); 0 elsewhere and where
    the z intervals do not overlap (h = min(tops) - max(bottoms) not positive)"""
    rows = np.asarray(rows, F64).reshape(-1, 8)
    n = rows.shape[0]
    out = np.zeros((n, n))
    if n < 2:
        return out
    haz = 0.5 * rows[:, 5]
    top, bot = rows[:, 2] + haz, rows[:, 2] - haz
    h = np.minimum(top[:, None], top[None, :]) - np.maximum(bot[:, None], bot[None, :])
    i, j = np.nonzero(np.triu(h > 0.0, 1))
    if i.shape[0]:
        out[i, j] = A.pair_iou(rows[i], rows[j])[0]
    return out


def nms_scene(rows, score, thresh, cls=None):
    """one scene -> (keep, rep, rank) as lists"""
    n = len(score)
    order = order_of(score)
    rank = [0] * n
    for r, i in enumerate(order):
        rank[i] = r
    iou = ordered_iou(np.asarray(rows, F64).reshape(-1, 8)[order])
    over = iou > thresh
    if cls is not None:
        c = np.asarray(cls)[order]
        over &= c[:, None] == c[None, :]
    keep, rep = [0] * n, [-1] * n
    kept = np.zeros(n, bool)                                                 # by rank
    for r, j in enumerate(order):
        first = np.flatnonzero(kept[:r] & over[:r, r])                       # ascending rank: the first kept box that suppresses
        if first.shape[0] == 0:
            keep[j], rep[j] = 1, j
            kept[r] = True
        else:
            rep[j] = order[int(first[0])]
    return keep, rep, rank


def box_nms(rows, score, thresh, cls=None, off=None):
    """-> (keep, rep, rank) int32 [K]; indices within the scene"""
    rows = np.asarray(rows, F64).reshape(-1, 8)
    score = np.asarray(score, F64).reshape(-1)
    o = offsets(off, rows.shape[0])
    keep, rep, rank = [], [], []
    for s in range(o.shape[0] - 1):
        a, b = int(o[s]), int(o[s + 1])
        k, p, r = nms_scene(rows[a:b], score[a:b], thresh, None if cls is None else np.asarray(cls)[a:b])
        keep += k
        rep += p
        rank += r
    return np.array(keep, np.int32), np.array(rep, np.int32), np.array(rank, np.int32)


def cluster_sizes(keep, rep, off=None):
    """int64 [K]: the boxes a kept box represents (itself included), 0 at a suppressed box"""
    keep, rep = np.asarray(keep), np.asarray(rep)
    o = offsets(off, keep.shape[0])
    out = np.zeros(keep.shape[0], np.int64)
    for s in range(o.shape[0] - 1):
        for i in range(int(o[s]), int(o[s + 1])):
            out[int(o[s]) + int(rep[i])] += 1
    return out


def proposals(seed, k, z0=0.0):
    """k proposals -> (rows [k,8], score [k]): ceil(k/8) objects in a 2 m cube (sizes 0.2 .. 0.8, any yaw), each repeated 8 times with a
    centre jitter of +-0.3 of its size (float32-valued centres), a size factor 0.8 .. 1.2 and a yaw jitter of +-0.15 rad; every
    sixteenth box an exact copy of its neighbour; shuffled; scores round(rand, 2)"""
    rng = np.random.RandomState(seed)
    if k == 0:
        return np.zeros((0, 8)), np.zeros(0)
    m = (k + 7) // 8
    c = rng.rand(m, 3) * 2.0
    s = 0.2 + 0.6 * rng.rand(m, 3)
    yaw = rng.rand(m) * 2.0 * np.pi
    c, s, yaw = np.repeat(c, 8, 0), np.repeat(s, 8, 0), np.repeat(yaw, 8)
    c = c + (rng.rand(8 * m, 3) * 2.0 - 1.0) * 0.3 * s
    c[:, 2] += z0
    c = c.astype(np.float32).astype(F64)
    s = s * (0.8 + 0.4 * rng.rand(8 * m, 3))
    yaw = yaw + (rng.rand(8 * m) * 2.0 - 1.0) * 0.15
    rows = np.concatenate([c, s, np.cos(yaw)[:, None], np.sin(yaw)[:, None]], 1)
    rows[15::16] = rows[14::16][:rows[15::16].shape[0]]
    rows = rows[:k]
    rows = rows[rng.permutation(k)]
    return np.ascontiguousarray(rows), np.round(rng.rand(k), 2)


def census(rows, score, thresh, keep, rep, rank):
    """what the issue's table counts, for one scene: kept, boxes kept although an earlier SUPPRESSED box overlaps them, boxes whose
    representative is not their first overlapping box, tied scores, the largest cluster"""
    order = order_of(score)
    iou = ordered_iou(np.asarray(rows, F64).reshape(-1, 8)[order])
    over = iou > thresh
    kept_through, not_first = 0, 0
    for r, j in enumerate(order):
        earlier = np.flatnonzero(over[:r, r])
        if keep[j] and earlier.shape[0]:
            kept_through += 1
        if not keep[j] and earlier.shape[0] and order[int(earlier[0])] != rep[j]:
            not_first += 1
    s = np.asarray(score, F64)
    tied = int(s.shape[0] - np.unique(s).shape[0])
    sizes = cluster_sizes(keep, rep)
    return dict(kept=int(np.sum(keep)), kept_through=kept_through, not_first=not_first, tied=tied, largest=int(sizes.max()) if sizes.size else 0)


def layered(seed, sizes):
    """ONE scene of sum(sizes) proposals in z-layers that do not touch: layer l is proposals(seed + l, sizes[l]) lifted by 4 l (the cube
    is 2 m and a box at most 0.96 m tall) -> (rows, score, the layer of every box)"""
    parts = [proposals(seed + l, n, 4.0 * l) for l, n in enumerate(sizes)]
    rows = np.concatenate([p[0] for p in parts])
    score = np.concatenate([p[1] for p in parts])
    perm = np.random.RandomState(seed).permutation(rows.shape[0])
    layer = np.repeat(np.arange(len(sizes)), sizes)[perm]
    return np.ascontiguousarray(rows[perm]), score[perm], layer
