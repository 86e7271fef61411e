"""Plain NumPy statements of the training step's cluster-level operators (csrc/kernels_train.hip), and the seeded edge cases
tests/test_gpu_train_edges.py runs them on ("ties in the backward maxima").  Everything is stated in float64: the classifier
tail and its backward, the backward of the group max, of the point -> cluster max and of the GCN layer, the stand-alone cross entropy and
the two optimizers.  The derivatives are written out (each is shorter than its kernel); tests/test_train_ops_ref.py holds them against
torch float64 autograd of oracle/train_ref.py.  A max or a ReLU gate sits at a discontinuity, so every generator asserts that its case is
one where the float64 statement itself is unambiguous (`top_gap`, `GAP`).  Nothing here touches a GPU."""
import numpy as np

import ops_ref as R

F32 = np.float32
GAP = 1e-3                          # smallest distance of a decision from its discontinuity, outside the ties built in on purpose
Y_GAP = 1e-6                        # ... of the tail's LeakyReLU input from 0 (the kernel's h is a float32: 6e-8 relative)
H, CLS, D5 = 128, 40, 256           # classifier: hidden width, classes, width of Feat_5
SMOOTH = 0.2                        # label smoothing (util.py:18)
BN_EPS = 1e-5
PAIR_EPS = 1e-6


# ---- statements -------------------------------------------------------------------------------------------------------------------------
def first_argmax(vals):
    """position of the first maximal row of every column, BY VALUE: both zeros are one value (np.argmax compares with <, like torch.max)"""
    return np.argmax(np.asarray(vals, np.float64), axis=0)


def top_gap(vals):
    """per column, the distance between the two largest DISTINCT values (inf where there is no second one)"""
    v = np.asarray(vals, np.float64)
    m = v.max(axis=0)
    second = np.where(v < m, v, -np.inf).max(axis=0)
    with np.errstate(invalid="ignore"):
        gap = m - second
    return np.where(np.isfinite(second) & np.isfinite(m), gap, np.inf)


def _targets(K, C, gold, smoothing):
    t = np.full((K, C), SMOOTH / (C - 1) if smoothing else 0.0)
    t[np.arange(K), gold] = 1.0 - SMOOTH if smoothing else 1.0
    return t


def _log_softmax(logits):
    z = logits - logits.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def tail(feat5, group, gold, keep, cls, scale=None):
    """sg_train_tail_forward / _backward (model.py:900-932, Classifier 154-166, util.py:12-29): Feat_6 = max over the clusters of an instance
    (first maximal cluster), linear1, BatchNorm1d on batch statistics, LeakyReLU(0.2), the keep mask, linear2, smoothed cross entropy
    (sum).  -> dict(feat6, arg, logits, loss_sum, mean, var, y) and, for loss = scale * loss_sum, the six gradients."""
    f5 = np.asarray(feat5, np.float64)
    group, gold = np.asarray(group, np.int64), np.asarray(gold, np.int64)
    w1, gamma, beta, w2, b2 = (np.asarray(cls[k], np.float64) for k in ("w1", "gamma", "beta", "w2", "b2"))
    K = gold.size
    arg = np.empty((K, D5), np.int64)
    for k in range(K):
        rows = np.nonzero(group == k)[0]
        arg[k] = rows[first_argmax(f5[rows])]
    f6 = f5[arg, np.arange(D5)]
    h = f6 @ w1.T
    mean, var = h.mean(axis=0), h.var(axis=0)
    inv = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (h - mean) * inv
    y = xhat * gamma + beta
    mask = np.ones_like(y) if keep is None else np.asarray(keep, np.float64)
    z = np.where(y > 0, y, 0.2 * y) * mask
    logits = z @ w2.T + b2
    logp = _log_softmax(logits)
    t = _targets(K, CLS, gold, True)
    out = dict(feat6=f6, arg=arg, logits=logits, loss_sum=float(-(t * logp).sum()), mean=mean, var=var, y=y)
    if scale is None:
        return out
    dlog = scale * (np.exp(logp) - t)
    dy = (dlog @ w2) * mask * np.where(y > 0, 1.0, 0.2)
    dh = gamma * inv * (dy - dy.mean(axis=0) - xhat * (dy * xhat).mean(axis=0))
    gf5 = np.zeros_like(f5)
    gf5[arg, np.arange(D5)] = dh @ w1                     # every (instance, channel) has its own winner row
    out.update(gw1=dh.T @ f6, ggamma=(dy * xhat).sum(axis=0), gbeta=dy.sum(axis=0), gw2=dlog.T @ z, gb2=dlog.sum(axis=0), gfeat5=gf5, dh=dh)
    return out


def group_max_backward(rows, goff, gidx, gout):
    """sg_group_max_rows_backward -> (grad [R,D] float32, written [R] bool).  The gradient of a group's maximum goes to the row at its first
    maximal POSITION, by value; every other row of the group gets 0; an empty group writes nothing; a row in no group is not written.
    A row id repeated inside a group receives the gradient iff one of its positions is that first maximal one (autograd of
    x[ids].max(0)).  The groups of one call share no row."""
    rows = np.asarray(rows, F32)
    grad = np.zeros(rows.shape, F32)
    written = np.zeros(rows.shape[0], bool)
    for g in range(len(goff) - 1):
        ids = np.asarray(gidx[goff[g]:goff[g + 1]], np.int64)
        if ids.size == 0:
            continue
        assert not written[ids].any(), "a row in two groups: the result would depend on the order of the groups"
        written[ids] = True
        grad[ids[first_argmax(rows[ids])], np.arange(rows.shape[1])] = np.asarray(gout, F32)[g]
    return grad, written


def segment_max_backward(rows, cl_off, gout):
    """sg_segment_max_backward -> grad [N,D] float32: cluster c = rows [cl_off[c], cl_off[c+1]); its gradient goes to its first maximal
    row by value (both zeros are one value), every other row is 0, an empty cluster sends nothing."""
    rows = np.asarray(rows, F32)
    grad = np.zeros(rows.shape, F32)
    for c in range(len(cl_off) - 1):
        lo, hi = int(cl_off[c]), int(cl_off[c + 1])
        if hi > lo:
            grad[lo + first_argmax(rows[lo:hi]), np.arange(rows.shape[1])] = np.asarray(gout, F32)[c]
    return grad


def gcn_forward(x, adj, w, alpha):
    """-> (A row-normalised [S,S], agg = A x, pre = agg W^T) of the dense formulation (model.py:262-274, 305-309, 141-151)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    adj = np.asarray(adj, np.int64).reshape(-1, 2)
    A = np.eye(x.shape[0])
    if adj.shape[0]:
        d = x[adj[:, 0]] - x[adj[:, 1]] + PAIR_EPS
        s = np.exp(-np.sqrt((d * d).sum(axis=1)) * alpha)
        A[adj[:, 0], adj[:, 1]] = s
        A[adj[:, 1], adj[:, 0]] = s
    A = A / A.sum(axis=1, keepdims=True)
    agg = A @ x
    return A, agg, agg @ w.T


def gcn_backward(x, adj, w, alpha, gout):
    """sg_gcn_backward -> (gx [S,D], gw [D,D], pre): out = relu(A x W^T) with A = rownorm(I + sym(exp(-alpha ||x_a - x_b + 1e-6||))),
    differentiated through the similarity weights and the row normalisation.  Edges are distinct unordered pairs, no self-edge."""
    x, w, gout = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(gout, np.float64)
    adj = np.asarray(adj, np.int64).reshape(-1, 2)
    A, agg, pre = gcn_forward(x, adj, w, alpha)
    G = gout * (pre > 0)
    gagg = G @ w
    gx = A.T @ gagg
    if adj.shape[0]:
        a, b = adj[:, 0], adj[:, 1]
        d = x[a] - x[b] + PAIR_EPS
        dist = np.sqrt((d * d).sum(axis=1))
        s = np.exp(-dist * alpha)
        r = 1.0 + np.bincount(np.concatenate([a, b]), np.concatenate([s, s]), x.shape[0])       # row sums before the normalisation
        gs = (gagg[a] * (x[b] - agg[a])).sum(axis=1) / r[a] + (gagg[b] * (x[a] - agg[b])).sum(axis=1) / r[b]
        step = (-alpha * s * gs / dist)[:, None] * d
        np.add.at(gx, a, step)
        np.add.at(gx, b, -step)
    return gx, G.T @ agg, pre


def cross_entropy(logits, gold, smoothing, scale=1.0):
    """sg_cross_entropy_forward / _backward (util.py:12-29) -> (loss sum, softmax [K,C], glogits = scale * (softmax - target))"""
    lg = np.asarray(logits, np.float64)
    K, C = lg.shape
    logp = _log_softmax(lg)
    t = _targets(K, C, np.asarray(gold, np.int64), smoothing)
    prob = np.exp(logp)
    return float(-(t * logp).sum()), prob, scale * (prob - t)


def sgd_step(p, g, buf, lr, momentum, wd, first):
    """torch.optim.SGD (train.py:96; dampening 0, no Nesterov) -> (p, buf)"""
    g = g + wd * p
    buf = g if first else momentum * buf + g
    return p - lr * buf, buf


def adam_step(p, g, m, v, lr, wd, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (train.py:98; L2 weight decay added to the gradient), step = 1, 2, ... -> (p, m, v)"""
    g = g + wd * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - beta2 ** step) + eps
    return p - lr / (1.0 - beta1 ** step) * m / denom, m, v


# ---- seeded cases -------------------------------------------------------------------------------------------------------------------------
def _grid(rng, shape):
    """normal values rounded to multiples of 1/64: two distinct values are at least 0.0156 > GAP apart, and equal ones are exact ties"""
    return (np.round(rng.normal(size=shape) * 64.0) / 64.0).astype(F32)


TAIL_K = (2, 3, 256, 257)
TAIL_VARIANTS = ("C_equals_K", "one_big_instance", "duplicate_clusters", "keep_null", "keep_zero_row", "gamma_neg_zero", "w1_row7_zero",
                 "gold_all_equal", "gold_0_39", "w2_x1000")
TAIL_CASES = tuple("K%d" % k for k in TAIL_K) + TAIL_VARIANTS
TAIL_AMPLIFYING = ("K2", "K3", "w1_row7_zero", "w2_x1000")          # float32 rounding amplified: the bound is measured (tail_fp32)
TAIL_DROPPED, TAIL_BIG, TAIL_DUP = 3, 4, 2                           # the instance whose keep row is 0 / that owns most clusters / of duplicates


def tail_case(name, seed=0):
    """-> dict(feat5 [C,256], group [C], gold [K], keep [K,128] or None, cls {w1, gamma, beta, w2, b2}, scale).  K = 2, 3, 256, 257 with
    C = K + 40; the variants are K = 9, C = 49 unless they say otherwise.  Every instance has a cluster."""
    rng = np.random.default_rng([61, TAIL_CASES.index(name), seed])
    K = int(name[1:]) if name[1:].isdigit() else 9
    C = K if name == "C_equals_K" else K + 40
    group = np.concatenate([np.arange(K), rng.integers(0, K, C - K)])
    if name == "one_big_instance":
        group[K:] = TAIL_BIG
    group = rng.permutation(group).astype(np.int32)
    feat5 = _grid(rng, (C, D5))
    if name == "duplicate_clusters":
        rows = np.nonzero(group == TAIL_DUP)[0]
        assert rows.size >= 3
        feat5[rows] = feat5[rows[0]]
    gold = rng.integers(0, CLS, K).astype(np.int32)
    if name == "gold_all_equal":
        gold[:] = 17
    elif name == "gold_0_39":
        gold = np.where(np.arange(K) % 2 == 0, 0, CLS - 1).astype(np.int32)
    keep = (rng.random((K, H)) < 0.5).astype(F32) * F32(2.0)
    if name == "keep_null":
        keep = None
    elif name == "keep_zero_row":
        keep[TAIL_DROPPED] = 0
    cls = dict(w1=(rng.normal(size=(H, D5)) / 16.0).astype(F32), gamma=(rng.normal(size=H) * 0.3 + 1.0).astype(F32),
               beta=(rng.normal(size=H) * 0.2).astype(F32), w2=(rng.normal(size=(CLS, H)) / 8.0).astype(F32), b2=(rng.normal(size=CLS) * 0.1).astype(F32))
    if name == "gamma_neg_zero":
        cls["gamma"][5], cls["gamma"][11] = F32(-0.7), F32(0.0)
    elif name == "w1_row7_zero":
        cls["w1"][7] = 0
    elif name == "w2_x1000":
        cls["w2"] *= F32(1e3)
    case = dict(feat5=feat5, group=group, gold=gold, keep=keep, cls=cls, scale=1.0 / K)
    ok, why = tail_valid(case)
    assert ok, f"tail case {name}: {why}"
    return case


def tail_valid(case):
    """the float64 statement is unambiguous: every instance's maximum is >= GAP above the next distinct value in every channel, and no
    LeakyReLU input is within Y_GAP of 0"""
    K = case["gold"].size
    if sorted(np.unique(case["group"]).tolist()) != list(range(K)):
        return False, "an instance without a cluster"
    gap = min(float(top_gap(case["feat5"][case["group"] == k]).min()) for k in range(K))
    y = np.abs(tail(case["feat5"], case["group"], case["gold"], case["keep"], case["cls"])["y"]).min()
    return (gap >= GAP and y >= Y_GAP), f"top gap {gap:.3g}, min |y| {y:.3g}"


def tail_torch(case, dtype):
    """the reference's own formulation (oracle/train_ref.tail) under torch autograd in `dtype` -> dict like tail()'s, gradients included"""
    import torch
    from oracle import train_ref
    names = {"w1": "classifier.linear1.weight", "gamma": "classifier.bn1.weight", "beta": "classifier.bn1.bias", "w2": "classifier.linear2.weight",
             "b2": "classifier.linear2.bias"}
    P = {names[k]: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in case["cls"].items()}
    f5 = torch.tensor(case["feat5"], dtype=dtype, requires_grad=True)
    loss, K = train_ref.tail(f5, case["group"], case["gold"][case["group"]], P, case["keep"])
    (loss * case["scale"]).backward()
    out = {"g" + k: P[names[k]].grad.numpy().astype(np.float64) for k in names}
    out.update(gfeat5=f5.grad.numpy().astype(np.float64), loss_sum=float(loss.detach()))
    return out


GROUPB_SIZES = R.GROUP_SIZES + (6, 2, 2, 5)          # ... + identical rows, {-0.0, +0.0}, {+0.0, -0.0}, all -inf (in the channels % 3 == 0)
GROUPB_D = R.GROUP_D + (192,)                        # 192: the trainer's own layout (trainer.cpp:197)


def group_backward_case(D, seed=0):
    """-> dict(rows [R, row_stride], goff, gidx, gout [G, out_stride], D, row_stride, out_stride, grow_stride).  The groups of ops_ref's
    GROUP_SIZES (empty ones, 1, 3/4/5/8/9, a hub of 1,000 positions over 30 rows), then six identical rows, the two zeros in each order,
    and five rows that are -inf in every third channel; disjoint, in a shuffled row order, with four rows in no group.  The columns past
    D hold 1e30.  D = 192 is the trainer's layout: row_stride = grow_stride = 192, gout the first 192 columns of a 256-wide buffer;
    otherwise row_stride = D + 5, out_stride = D + 7, grow_stride = D + 3."""
    rng = np.random.default_rng([67, D, seed])
    row_stride, out_stride, grow_stride = (192, 256, 192) if D == 192 else (D + 5, D + 7, D + 3)
    groups, used = [], 0
    for n in GROUPB_SIZES:
        own = 30 if n > 100 else n
        ids = np.arange(used, used + own)
        groups.append(np.concatenate([ids, rng.choice(ids, n - own)]) if n > own else ids)
        used += own
    R_ = used + 4
    perm = rng.permutation(R_)
    groups = [perm[rng.permutation(g)] for g in groups]
    rows = np.full((R_, row_stride), 1e30, F32)
    rows[:, :D] = _grid(rng, (R_, D))
    base = len(R.GROUP_SIZES)
    rows[groups[base], :D] = rows[groups[base][0], :D]
    rows[groups[base + 1], :D] = np.array([-0.0, 0.0], F32)[:, None]
    rows[groups[base + 2], :D] = np.array([0.0, -0.0], F32)[:, None]
    rows[groups[base + 3], 0:D:3] = -np.inf
    goff = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=goff[1:])
    gout = np.full((len(groups), out_stride), 1e30, F32)
    gout[:, :D] = rng.normal(size=(len(groups), D))
    case = dict(rows=rows, goff=goff, gidx=np.concatenate(groups).astype(np.int32), gout=gout, D=D, row_stride=row_stride, out_stride=out_stride,
                grow_stride=grow_stride)
    assert group_backward_gap(case) >= GAP
    return case


def group_backward_gap(case):
    goff, gidx, D = case["goff"], case["gidx"], case["D"]
    return min(float(top_gap(case["rows"][gidx[goff[g]:goff[g + 1]], :D]).min()) for g in range(len(goff) - 1) if goff[g + 1] > goff[g])


SEGB_BUILT_TIES = ("value_sets", "value_sets_first_block")       # ops_ref's subnormals, zeros and infinities: ties and gaps built on purpose
SEGB_SEED = 10                                                   # the first seed at which ops_ref's random cases keep GAP in every (cluster, channel)


def segment_backward_cases(seed=SEGB_SEED):
    """name -> dict(rows [N,D], cl_off [C+1], gout [C, out_stride], D, col0, out_stride): ops_ref.segment_max_cases() with cl_off derived
    from the ascending ids (a gap in the ids is an empty cluster), the gaps case again behind two empty clusters, equal maxima in two
    different 64-row blocks of one cluster, D = 1 and D = 70, the trainer's layout (gout at column 128 of a 192-wide buffer,
    trainer.cpp:209), and C = 0 / N = 0."""
    rng = np.random.default_rng([71, seed])
    cases = {}

    def add(name, rows, cl_off, col0=0, out_stride=None):
        rows = np.ascontiguousarray(rows, F32)
        D = rows.shape[1]
        out_stride = D + 6 if out_stride is None else out_stride
        gout = np.full((max(len(cl_off) - 1, 1), out_stride), 1e30, F32)
        gout[:, col0:col0 + D] = rng.normal(size=(gout.shape[0], D))
        cases[name] = dict(rows=rows, cl_off=np.asarray(cl_off, np.int32), gout=gout, D=D, col0=col0, out_stride=out_stride)

    for name, (rows, cl, C_) in sorted(R.segment_max_cases(seed).items()):
        add(name, rows, np.searchsorted(cl, np.arange(C_ + 1)))
    rows, cl, C_ = R.segment_max_cases(seed)["gaps"]
    add("gaps_behind_empty_front", rows, np.searchsorted(cl + 2, np.arange(C_ + 3)))
    tied = _grid(rng, (200, 64)) - F32(8.0)
    tied[[70, 150]] = 0.5                                                   # blocks 1 and 2: row 70 wins the even channels
    tied[[150, 10], 1::2] = 0.75                                            # blocks 2 and 0: row 10 wins the odd ones
    add("equal_maxima_in_two_blocks", tied, [0, 200])
    off = np.array([0, 1, 1, 66, 130, 130, 141], np.int32)
    add("D1", _grid(rng, (141, 1)), off)
    add("D70", _grid(rng, (141, 70)), off)
    add("trainer_layout", _grid(rng, (141, 64)), off, col0=128, out_stride=192)
    add("C0", _grid(rng, (5, 64)), [0])
    add("N0", np.zeros((0, 64), F32), [0, 0, 0])
    for name, c in cases.items():
        assert c["cl_off"][0] == 0 and c["cl_off"][-1] == (c["rows"].shape[0] if len(c["cl_off"]) > 1 else 0) and np.all(np.diff(c["cl_off"]) >= 0), name
        if name not in SEGB_BUILT_TIES:
            assert segment_backward_gap(c) >= GAP, name
    return cases


def segment_backward_gap(case):
    off = case["cl_off"]
    return min([float(top_gap(case["rows"][off[c]:off[c + 1]]).min()) for c in range(len(off) - 1) if off[c + 1] > off[c]] + [np.inf])


GCN_CASES = ("S1", "S2", "hubs_D1", "hubs_D192", "hubs_D256")
GCN_ALPHA = 0.125
GCN_HUBS = (300, 257)                                # degrees: the e += 256 trip of k_gcn_bwd_rows, taken by 44 edges and by one


def _sym_csr(adj, S):
    """the symmetric CSR sg_gcn_backward takes: per row the neighbours and the edge ids, in edge order"""
    rowptr = np.zeros(S + 1, np.int32)
    for c in (0, 1):
        np.add.at(rowptr, adj[:, c] + 1, 1)
    np.cumsum(rowptr, out=rowptr)
    fill = rowptr[:-1].copy()
    col, eid = np.zeros(2 * len(adj), np.int32), np.zeros(2 * len(adj), np.int32)
    for e, (u, v) in enumerate(adj):
        col[fill[u]] = v; eid[fill[u]] = e; fill[u] += 1
        col[fill[v]] = u; eid[fill[v]] = e; fill[v] += 1
    return rowptr, col, eid


def gcn_case(name, seed=0):
    """-> dict(x [S,D], adj [E,2] int32, rowptr, col, eid, w [D,D], gout [S,D], alpha, dead, pair).  S1: one node, no edge.  S2: two nodes,
    one edge.  hubs_D*: node 0 of degree 300, node 1 of degree 257 (they share leaves and an edge), some leaf-leaf edges, node `dead`
    isolated with W x < 0 in every output (its gout is gated to 0 everywhere), another node isolated, and the edge `pair` joining two
    bitwise-equal rows (dist = sqrt(D) 1e-6).  Rows whose pre-activation comes within GAP of 0 in the float64 statement are drawn again
    (in a fixed order, from the case's own stream) until none does."""
    rng = np.random.default_rng([73, GCN_CASES.index(name), seed])
    if name in ("S1", "S2"):
        S, D = int(name[1]), 192
        adj = np.array([[1, 0]] if S == 2 else [], np.int32).reshape(-1, 2)
        dead, pair, fixed = -1, (-1, -1), []
    else:
        D, S = int(name.split("D")[1]), 400
        dead, iso, pair = S - 1, S - 2, (S - 4, S - 3)
        leaves = np.arange(2, S - 4)
        edges = {(0, 1), pair}
        edges |= {(0, int(j)) for j in rng.choice(leaves, GCN_HUBS[0] - 1, replace=False)}
        edges |= {(int(j), 1) for j in rng.choice(leaves, GCN_HUBS[1] - 1, replace=False)}            # hub 1 is the SECOND endpoint
        while len(edges) < GCN_HUBS[0] + GCN_HUBS[1] + 60:
            a, b = (int(v) for v in rng.choice(leaves, 2, replace=False))
            if (b, a) not in edges:
                edges.add((a, b))
        adj = np.array(sorted(edges), np.int32)
        adj = adj[rng.permutation(len(adj))]
        fixed = [dead]
    w = (rng.normal(size=(D, D)) / np.sqrt(D)).astype(F32)
    xs = 0.3 if D == 1 else 1.0 if S <= 2 else 1.5             # hubs: similarities of 0.03, so that a hub's mean keeps a pre-activation of size 0.2
    x = (rng.normal(size=(S, D)) * xs).astype(F32)
    if dead >= 0:
        x[dead] = np.linalg.solve(w.astype(np.float64), -np.ones(D))                                   # isolated: agg = x, pre = W x = -1
        x[pair[1]] = x[pair[0]]
    for _ in range(200):
        pre = gcn_forward(x, adj, w, GCN_ALPHA)[2]
        bad = [i for i in np.nonzero((np.abs(pre) < GAP).any(axis=1))[0] if i not in fixed]
        if not bad:
            break
        for i in bad:
            x[i] = rng.normal(size=D) * xs
            if i in pair:
                x[pair[0]] = x[pair[1]] = x[i]
    rowptr, col, eid = _sym_csr(adj, S)
    gout = rng.normal(size=(S, D)).astype(F32)
    case = dict(x=x, adj=adj, rowptr=rowptr, col=col, eid=eid, w=w, gout=gout, alpha=GCN_ALPHA, dead=dead, pair=pair)
    assert gcn_gap(case) >= GAP, f"gcn case {name}: a pre-activation within {gcn_gap(case):.3g} of 0"
    return case


def gcn_gap(case):
    return float(np.abs(gcn_forward(case["x"], case["adj"], case["w"], case["alpha"])[2]).min())


def gcn_torch(case, dtype):
    """the reference's dense formulation (oracle/train_ref.gcn) under torch autograd in `dtype` -> (gx, gw) float64"""
    import torch
    from oracle import train_ref
    x = torch.tensor(case["x"], dtype=dtype, requires_grad=True)
    w = torch.tensor(case["w"], dtype=dtype, requires_grad=True)
    train_ref.gcn(x, case["adj"], w, case["alpha"]).backward(torch.tensor(case["gout"], dtype=dtype))
    return x.grad.numpy().astype(np.float64), w.grad.numpy().astype(np.float64)


CE_K = (1, 255, 256, 257)
CE_C = (2, 40, 41)
CE_SCALES = (1.0, 1e4)
CE_GRID_STRIDE = (6554, 40)                          # K C = 262,160 = 1024 x 256 + 16: the backward's grid-stride loop takes a second trip


def cross_entropy_case(K, C, logit_scale=1.0, seed=0):
    """-> (logits [K,C] float32, gold [K] int32): gold holds 0 and C - 1 (K = 1: C - 1)"""
    rng = np.random.default_rng([79, K, C, seed])
    logits = (rng.normal(size=(K, C)) * 3.0 * logit_scale).astype(F32)
    gold = rng.integers(0, C, K).astype(np.int32)
    gold[0] = 0
    gold[-1] = C - 1
    return logits, gold


OPT_N = (1, 255, 257, 1024 * 256 + 259)
OPT_STEPS = 5
OPT_LATE_STEP = 100000
SGD_ARGS = dict(lr=0.1, momentum=0.9, wd=1e-4)       # train.py:96 (lr 0.001 * 100)
ADAM_ARGS = dict(lr=0.001, wd=1e-4)                  # train.py:98


def optimizer_case(n, seed=0):
    """-> (p0 [n], grads [OPT_STEPS + 1, n]) float32; for n > 1 the last element is a weight of 0 whose gradient is always 0"""
    rng = np.random.default_rng([83, n, seed])
    p0 = rng.normal(size=n).astype(F32)
    grads = (rng.normal(size=(OPT_STEPS + 1, n)) * 0.1).astype(F32)
    if n > 1:
        p0[-1] = 0
        grads[:, -1] = 0
    return p0, grads


def optimizer_runs(p0, grads, use_sgd, dtype):
    """the parameter vector after each of OPT_STEPS steps (and, Adam, after one more taken as step OPT_LATE_STEP): the statement in float64
    (dtype = None) or torch.optim in `dtype` on the CPU"""
    out = []
    if dtype is None:
        p = p0.astype(np.float64)
        a, b = np.zeros_like(p), np.zeros_like(p)
        for i in range(OPT_STEPS + (0 if use_sgd else 1)):
            g = grads[i].astype(np.float64)
            if use_sgd:
                p, a = sgd_step(p, g, a, first=i == 0, **SGD_ARGS)
            else:
                p, a, b = adam_step(p, g, a, b, step=i + 1 if i < OPT_STEPS else OPT_LATE_STEP, **ADAM_ARGS)
            out.append(p.copy())
        return out
    import torch
    ref = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
    opt = torch.optim.SGD([ref], lr=SGD_ARGS["lr"], momentum=SGD_ARGS["momentum"], weight_decay=SGD_ARGS["wd"]) if use_sgd else \
        torch.optim.Adam([ref], lr=ADAM_ARGS["lr"], weight_decay=ADAM_ARGS["wd"])
    for i in range(OPT_STEPS + (0 if use_sgd else 1)):
        if i == OPT_STEPS:
            opt.state[ref]["step"] = torch.tensor(float(OPT_LATE_STEP - 1))
        ref.grad = torch.tensor(grads[i], dtype=dtype)
        opt.step()
        out.append(ref.detach().numpy().astype(np.float64).copy())
    return out
