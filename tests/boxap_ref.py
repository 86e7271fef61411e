"""Box IoU and detection AP restated: the operation sequence of include/seggroup_hip.h in NumPy float64, one statement per
operation, over P pairs at once (a predicate of the sequence is an `np.where`), and the scoring rule of seggroup_amd/boxap.py in plain
Python loops.  It never calls the library.  `exact_iou` is the truth the restatement is measured against: the same boxes, as the four
corners centre +/- (sx/2)(c, s) +/- (sy/2)(-s, c) over the doubles they hold, clipped in fractions.Fraction -- nothing rounds."""
from fractions import Fraction

import numpy as np

F64 = np.float64
SLOTS = 8


def _put(u, v, m, sel, x, y):
    """slot m <- (x, y) where `sel`; an append past slot 7 is dropped"""
    for j in range(SLOTS):
        hit = sel & (m == j)
        u[j] = np.where(hit, x, u[j])
        v[j] = np.where(hit, y, v[j])


def _dist(side, u, v, h):
    return h - u if side == 0 else u + h if side == 1 else h - v if side == 2 else v + h


def _clip_side(side, max_in, iu, iv, n, h):
    zero = np.zeros_like(h)
    ou, ov = [zero.copy() for _ in range(SLOTS)], [zero.copy() for _ in range(SLOTS)]
    m = np.zeros(h.shape, np.int64)
    pu, pv = iu[0], iv[0]
    for j in range(1, max_in):
        last = n - 1 == j
        pu = np.where(last, iu[j], pu)
        pv = np.where(last, iv[j], pv)
    dp = _dist(side, pu, pv, h)
    for i in range(max_in):
        live = i < n
        qu, qv = iu[i], iv[i]
        dq = _dist(side, qu, qv, h)
        in_p, in_q = dp >= 0.0, dq >= 0.0
        cross = live & (in_p != in_q)
        den = dp - dq
        t = dp / np.where(cross, den, 1.0)
        if side < 2:
            xu = h if side == 0 else -h
            dv = qv - pv
            tv = t * dv
            xv = pv + tv
        else:
            du = qu - pu
            tu = t * du
            xu = pu + tu
            xv = h if side == 2 else -h
        _put(ou, ov, m, cross, xu, xv)
        m = m + cross
        keep = live & in_q
        _put(ou, ov, m, keep, qu, qv)
        m = m + keep
        pu = np.where(live, qu, pu)
        pv = np.where(live, qv, pv)
        dp = np.where(live, dq, dp)
    return ou, ov, np.minimum(m, SLOTS)


def pair_iou(a, b):
    """IoU of rows a [P,8] with rows b [P,8] -> float64 [P], the header's sequence"""
    a, b = np.asarray(a, F64).reshape(-1, 8), np.asarray(b, F64).reshape(-1, 8)
    ax, ay, az, asx, asy, asz, ac, as_ = (a[:, k] for k in range(8))
    bx, by, bz, bsx, bsy, bsz, bc, bs = (b[:, k] for k in range(8))
    with np.errstate(all="ignore"):
        dx = ax - bx
        dy = ay - by
        hax = 0.5 * asx
        hay = 0.5 * asy
        hbx = 0.5 * bsx
        hby = 0.5 * bsy
        ex = hax * ac
        ey = hax * as_
        fx = hay * as_
        fy = hay * ac
        xm, xp, ym, yp = dx - ex, dx + ex, dy - ey, dy + ey
        wx = [xm + fx, xp + fx, xp - fx, xm - fx]
        wy = [ym - fy, yp - fy, yp + fy, ym + fy]
        zero = np.zeros_like(dx)
        pu, pv = [zero.copy() for _ in range(SLOTS)], [zero.copy() for _ in range(SLOTS)]
        for k in range(4):
            t0 = bc * wx[k]
            t1 = bs * wy[k]
            pu[k] = t0 + t1
            t2 = bc * wy[k]
            t3 = bs * wx[k]
            pv[k] = t2 - t3
        n = np.full(dx.shape, 4, np.int64)
        pu, pv, n = _clip_side(0, 4, pu, pv, n, hbx)
        pu, pv, n = _clip_side(1, 5, pu, pv, n, hbx)
        pu, pv, n = _clip_side(2, 6, pu, pv, n, hby)
        pu, pv, n = _clip_side(3, 7, pu, pv, n, hby)
        acc = zero.copy()
        for i in range(1, SLOTS - 1):
            e0 = pu[i] - pu[0]
            e1 = pv[i] - pv[0]
            g0 = pu[i + 1] - pu[0]
            g1 = pv[i + 1] - pv[0]
            c0 = e0 * g1
            c1 = e1 * g0
            cr = c0 - c1
            acc = np.where(i + 1 < n, acc + cr, acc)
        area = 0.5 * acc
        area = np.where(area > 0.0, area, 0.0)
        haz = 0.5 * asz
        hbz = 0.5 * bsz
        top = np.minimum(az + haz, bz + hbz)
        bottom = np.maximum(az - haz, bz - hbz)
        h = top - bottom
        h = np.where(h > 0.0, h, 0.0)
        inter = area * h
        va = (asx * asy) * asz
        vb = (bsx * bsy) * bsz
        uni = (va + vb) - inter
        pos = uni > 0.0
        return np.where(pos, inter / np.where(pos, uni, 1.0), 0.0), n


def offsets(off, k):
    return np.array([0, k], np.int64) if off is None else np.asarray(off, np.int64)


def box_iou(a, b, off_a=None, off_b=None):
    """-> the list of [Ka_b, Kb_b] blocks, one per scene"""
    a, b = np.asarray(a, F64).reshape(-1, 8), np.asarray(b, F64).reshape(-1, 8)
    oa, ob = offsets(off_a, a.shape[0]), offsets(off_b, b.shape[0])
    out = []
    for s in range(oa.shape[0] - 1):
        sa, sb = a[oa[s]:oa[s + 1]], b[ob[s]:ob[s + 1]]
        ka, kb = sa.shape[0], sb.shape[0]
        if ka * kb == 0:
            out.append(np.zeros((ka, kb)))
            continue
        out.append(pair_iou(np.repeat(sa, kb, 0), np.tile(sb, (ka, 1)))[0].reshape(ka, kb))
    return out


def box_best(a, b, cls_a=None, cls_b=None, off_a=None, off_b=None):
    """-> (best int32 [Ka], iou float64 [Ka]): the highest IoU of the scene's B boxes (of the same class), the lowest index among equals;
    an IoU of 0 is not a partner"""
    a = np.asarray(a, F64).reshape(-1, 8)
    oa = offsets(off_a, a.shape[0])
    best, top = np.full(a.shape[0], -1, np.int32), np.zeros(a.shape[0])
    ob = offsets(off_b, np.asarray(b).reshape(-1, 8).shape[0])
    for s, block in enumerate(box_iou(a, b, off_a, off_b)):
        for r in range(block.shape[0]):
            i = int(oa[s]) + r
            for j in range(block.shape[1]):
                if cls_a is not None and int(cls_a[i]) != int(cls_b[int(ob[s]) + j]):
                    continue
                if block[r, j] > top[i]:
                    best[i], top[i] = j, block[r, j]
    return best, top


# ---- the truth --------------------------------------------------------------------------------------------------------------------------
def _corners(box):
    cx, cy, _, sx, sy, _, c, s = (Fraction(float(v)) for v in box)
    hx, hy = sx / 2, sy / 2
    return [(cx + su * hx * c - sv * hy * s, cy + su * hx * s + sv * hy * c) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def _area(poly):
    return sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly))) / 2 if poly else Fraction(0)


def exact_iou(a, b):
    """-> (the IoU as a Fraction, the vertices of the clipped footprint)"""
    poly, clip = _corners(a), _corners(b)
    for k in range(4):
        (x0, y0), (x1, y1) = clip[k], clip[(k + 1) % 4]
        d = [(x1 - x0) * (y - y0) - (y1 - y0) * (x - x0) for x, y in poly]          # >= 0 on the inner side of a counter-clockwise edge
        out = []
        for i in range(len(poly)):
            p, q, dp, dq = poly[i - 1], poly[i], d[i - 1], d[i]
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
            if dq >= 0:
                out.append(q)
        poly = out
    az, asz, bz, bsz = (Fraction(float(v)) for v in (a[2], a[5], b[2], b[5]))
    h = max(Fraction(0), min(az + asz / 2, bz + bsz / 2) - max(az - asz / 2, bz - bsz / 2))
    inter = abs(_area(poly)) * h
    uni = _area(_corners(a)) * asz + _area(_corners(b)) * bsz - inter
    return (inter / uni if uni > 0 else Fraction(0)), len(poly)


def row(cx, cy, cz, sx, sy, sz, yaw=0.0):
    """a box row from a yaw in radians; multiples of a quarter turn get exact (c, s)"""
    q = yaw / (np.pi / 2)
    if q == round(q):
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(round(q)) % 4]
    else:
        c, s = float(np.cos(yaw)), float(np.sin(yaw))
    return np.array([cx, cy, cz, sx, sy, sz, c, s], F64)


def random_pairs(seed, n):
    """the pairs of the issue: float32-valued centres in a 2 m cube, sizes 0.05 .. 1.55, any yaw with a share at multiples of 45
    degrees, a share of identical and of half-shifted pairs -> (a [n,8], b [n,8])"""
    rng = np.random.RandomState(seed)

    def boxes():
        c = (rng.rand(n, 3) * 2.0).astype(np.float32).astype(F64)
        s = 0.05 + 1.5 * rng.rand(n, 3)
        yaw = rng.rand(n) * 2.0 * np.pi
        grid = rng.rand(n) < 0.25
        yaw = np.where(grid, rng.randint(0, 8, n) * (np.pi / 4), yaw)
        return np.concatenate([c, s, np.cos(yaw)[:, None], np.sin(yaw)[:, None]], 1)
    a, b = boxes(), boxes()
    kind = rng.rand(n)
    same, half = kind < 0.1, (kind >= 0.1) & (kind < 0.2)
    b[same] = a[same]
    b[half] = a[half]
    b[half, 0] = a[half, 0] + 0.5 * a[half, 3]                  # along world x: half a side only for an axis-aligned box
    return a, b


# ---- the scoring rule, in loops ------------------------------------------------------------------------------------------------------------
def match(best, iou, cls, scene_of_pred, score=None, thresholds=(0.25, 0.5)):
    """-> tp[t][k] booleans.  Predictions by descending score, scene then index breaking ties; a prediction is a true positive when its
    best box has IoU > t and no earlier prediction took that box."""
    k = len(best)
    sc = [1.0] * k if score is None else [float(v) for v in score]
    order = sorted(range(k), key=lambda i: (-sc[i], int(scene_of_pred[i]), i))
    out = []
    for t in thresholds:
        taken, tp = set(), [False] * k
        for i in order:
            if int(best[i]) < 0 or not float(iou[i]) > t:
                continue
            key = (int(scene_of_pred[i]), int(cls[i]), int(best[i]))
            if key in taken:
                continue
            taken.add(key)
            tp[i] = True
        out.append(tp)
    return out


def average_precision(tp, score, n_gt):
    """one class, one threshold: a point per distinct score, the area under the monotone precision envelope -> (ap, recall)"""
    if n_gt == 0:
        return float("nan"), float("nan")
    if len(tp) == 0:
        return 0.0, 0.0
    order = sorted(range(len(tp)), key=lambda i: -float(score[i]))
    pts, ntp, nfp = [], 0, 0
    for pos, i in enumerate(order):
        ntp += 1 if tp[i] else 0
        nfp += 0 if tp[i] else 1
        if pos + 1 == len(order) or float(score[order[pos + 1]]) != float(score[i]):
            pts.append((ntp / n_gt, ntp / (ntp + nfp)))
    ap, above, prev = 0.0, 0.0, None
    env = [0.0] * len(pts)
    for j in range(len(pts) - 1, -1, -1):
        above = max(above, pts[j][1])
        env[j] = above
    prev = 0.0
    for j, (r, _) in enumerate(pts):
        ap = ap + (r - prev) * env[j]
        prev = r
    return ap, pts[-1][0]


def evaluate(best, iou, cls, scene_of_pred, n_gt, score=None, thresholds=(0.25, 0.5)):
    """n_gt: {class: ground-truth boxes over all scenes} -> {threshold: {class: dict(ap, recall, pred, gt, tp)}, and "map"}"""
    tps = match(best, iou, cls, scene_of_pred, score, thresholds)
    k = len(best)
    sc = [1.0] * k if score is None else [float(v) for v in score]
    classes = sorted(set(int(c) for c in cls) | set(int(c) for c in n_gt))
    out = {}
    for t, tp in zip(thresholds, tps):
        per, aps = {}, []
        for c in classes:
            idx = [i for i in range(k) if int(cls[i]) == c]
            g = int(n_gt.get(c, 0))
            ap, rec = average_precision([tp[i] for i in idx], [sc[i] for i in idx], g)
            per[c] = dict(ap=ap, recall=rec, pred=len(idx), gt=g, tp=sum(1 for i in idx if tp[i]))
            if g > 0:
                aps.append(ap)
        out[t] = dict(classes=per, map=(sum(aps) / len(aps) if aps else float("nan")))
    return out
