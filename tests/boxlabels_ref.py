"""NumPy restatement of sg_points_in_boxes and of the owner and segment rules behind seggroup_amd/boxlabels.py.  It never
calls the library.  The test of a point against a box is one NumPy statement per operation of include/seggroup_hip.h, in float64 on the
widened fp32 points, with the predicate as boolean arrays; the owner and the segment rules are plain loops."""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64


def row(cx, cy, cz, sx, sy, sz, R=None):
    """one box as 15 doubles: centre, full size, R row-major (the identity by default)"""
    return np.concatenate([[cx, cy, cz, sx, sy, sz], (np.eye(3) if R is None else np.asarray(R, F64)).reshape(9)]).astype(F64)


def yaw_frame(theta):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


QUARTER = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])       # a quarter turn about z: entries 0 / +-1, exact


def inside_matrix(xyz, boxes, margin=0.0):
    """-> (inside bool [N,K], vol float64 [K]) of one scene, every point against every box"""
    p = np.asarray(xyz)[:, :3].astype(F32).astype(F64)
    b = np.asarray(boxes, F64).reshape(-1, 15)
    inside = np.ones((p.shape[0], b.shape[0]), bool)
    d0 = p[:, 0:1] - b[None, :, 0]
    d1 = p[:, 1:2] - b[None, :, 1]
    d2 = p[:, 2:3] - b[None, :, 2]
    for k in range(3):
        t0 = b[None, :, 6 + 3 * k] * d0
        t1 = b[None, :, 7 + 3 * k] * d1
        t2 = b[None, :, 8 + 3 * k] * d2
        l = (t0 + t1) + t2
        half = 0.5 * b[:, 3 + k]
        h = half + margin
        inside = inside & (np.abs(l) <= h[None, :])
    vol = (b[:, 3] * b[:, 4]) * b[:, 5]
    return inside, vol


def scene_outputs(inside, vol):
    """count, first, inner int32 [N] of one scene from its matrix: the boxes in ascending index, a box replaces the kept one only when
    its vol is smaller"""
    n, k = inside.shape
    count = inside.sum(1).astype(np.int32)
    first = np.full(n, -1, np.int32)
    inner = np.full(n, -1, np.int32)
    kept = np.zeros(n)
    for j in range(k):
        hit = inside[:, j]
        first = np.where(hit & (first < 0), np.int32(j), first)
        take = hit & ((inner < 0) | (vol[j] < kept))
        inner = np.where(take, np.int32(j), inner)
        kept = np.where(take, vol[j], kept)
    return count, first.astype(np.int32), inner.astype(np.int32)


def points_in_boxes(xyz, boxes, margin=0.0, off_p=None, off_b=None):
    """-> (count, first, inner int32 [N], held int32 [K]); with offsets, scene by scene"""
    xyz = np.asarray(xyz).reshape(-1, np.asarray(xyz).shape[-1] if np.asarray(xyz).ndim == 2 else 3)
    boxes = np.asarray(boxes, F64).reshape(-1, 15)
    n, k = xyz.shape[0], boxes.shape[0]
    off_p = [0, n] if off_p is None else list(off_p)
    off_b = [0, k] if off_b is None else list(off_b)
    count, first, inner, held = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(k, np.int32)
    for s in range(len(off_p) - 1):
        p0, p1, b0, b1 = off_p[s], off_p[s + 1], off_b[s], off_b[s + 1]
        inside, vol = inside_matrix(xyz[p0:p1], boxes[b0:b1], margin)
        count[p0:p1], first[p0:p1], inner[p0:p1] = scene_outputs(inside, vol)
        held[b0:b1] = inside.sum(0)
    return count, first, inner, held


# ---- exact containment ------------------------------------------------------------------------------------------------------------------------
def exact_gaps(p, box, margin=0.0):
    """one point (3 floats) against one box (15 doubles) in fractions over the doubles the arrays hold -> [|l_k| - h_k for k = 0, 1, 2],
    exact: the point is inside iff every gap is <= 0"""
    f = [Fraction(float(v)) for v in box]
    d = [Fraction(float(p[i])) - f[i] for i in range(3)]
    gaps = []
    for k in range(3):
        l = f[6 + 3 * k] * d[0] + f[7 + 3 * k] * d[1] + f[8 + 3 * k] * d[2]
        gaps.append(abs(l) - (f[3 + k] / 2 + Fraction(float(margin))))
    return gaps


def random_scene(seed, n=2000, k=17):
    """the input of the check against exact containment: float32 points uniform in [0,2)^3, boxes with float32-valued centres in that
    cube and sizes uniform in 0.05 .. 1.55; even boxes get a random yaw, odd boxes a QR frame of determinant +1"""
    rng = np.random.RandomState(seed)
    xyz = (rng.rand(n, 3) * 2.0).astype(F32)
    c = (rng.rand(k, 3) * 2.0).astype(F32).astype(F64)
    s = 0.05 + 1.5 * rng.rand(k, 3)
    boxes = np.zeros((k, 15))
    for j in range(k):
        if j % 2 == 0:
            R = yaw_frame(rng.rand() * 2.0 * math.pi)
        else:
            R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if np.linalg.det(R) < 0.0:
                R[2] = -R[2]
        boxes[j] = row(*c[j], *s[j], R=R)
    return xyz, boxes


# ---- the owner and the segment rules, in loops -----------------------------------------------------------------------------------------------
def vertex_owner(count, first, inner, k, overlap="skip"):
    out = []
    for c, f, i in zip(count, first, inner):
        if c == 0:
            out.append(0)
        elif c == 1:
            out.append(1 + int(f))
        else:
            out.append(k + 1 if overlap == "skip" else 1 + int(i))
    return out


def vote(seg, owner):
    """the rows a vote over (segment, code) gives, ascending segment id -> (row_ids, winner, winner_count, row_count, tied) as lists"""
    rows = {}
    for s, o in zip(seg, owner):
        rows.setdefault(int(s), {})
        rows[int(s)][int(o)] = rows[int(s)].get(int(o), 0) + 1
    out = ([], [], [], [], [])
    for s in sorted(rows):
        top = max(rows[s].values())
        winners = sorted(c for c, v in rows[s].items() if v == top)
        for column, value in zip(out, (s, winners[0], top, sum(rows[s].values()), int(len(winners) > 1))):
            column.append(value)
    return out


def segment_boxes(seg, owner, k, purity=1.0):
    """-> {segment id: (box or -1, votes of the winner, size)}: the winner is the code most vertices hold, the lowest code among equals;
    the segment takes box w - 1 when the winner w is a box's code, no other code has as many votes, and votes >= purity * size"""
    rows = {}
    for s, o in zip(seg, owner):
        rows.setdefault(int(s), {})
        rows[int(s)][int(o)] = rows[int(s)].get(int(o), 0) + 1
    out = {}
    for s, votes in rows.items():
        size = sum(votes.values())
        top = max(votes.values())
        winners = sorted(c for c, v in votes.items() if v == top)
        w = winners[0]
        ok = 1 <= w <= k and len(winners) == 1 and float(top) >= purity * float(size)
        out[s] = (w - 1 if ok else -1, top, size)
    return out


def weak_labels(seg, owner, k, ids, sem, purity=1.0):
    """-> (ins, sem) lists: every vertex of a segment that took box b gets ids[b] / sem[b], every other vertex -1"""
    table = segment_boxes(seg, owner, k, purity)
    ins_out, sem_out = [], []
    for s in seg:
        b = table[int(s)][0]
        ins_out.append(int(ids[b]) if b >= 0 else -1)
        sem_out.append(int(sem[b]) if b >= 0 else -1)
    return ins_out, sem_out
