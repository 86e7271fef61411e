"""Plain NumPy statements of the scene path's small operators, and the seeded edge cases tests/test_gpu_ops_edges.py runs them on
("signed zero in the float max"; section 6).  Float operators are stated in float64; where oracle/cpu_ref.py already is the
statement (mlp1_forward, edge_distance, group_max, evaluate, centre_per_cluster) it is reused and only what it lacks is added here:
untouched clusters, empty groups, refused edges, out-of-range gathers, strides.  Nothing here touches a GPU."""
import numpy as np

from oracle import cpu_ref as O

F32 = np.float32
NEG_INF = F32(-np.inf)
SUB = F32(1e-41)                    # a float32 subnormal (the smallest normal is 1.18e-38)


# ---- statements -------------------------------------------------------------------------------------------------------------------------
def segment_max(rows, cluster_of_pos, C):
    """sg_segment_max: out[c] = maximum BY VALUE of the rows of cluster c, -inf where the cluster has no row.  Both zeros are one value:
    compare with ==, never by bits."""
    rows = np.asarray(rows, F32)
    out = np.full((C, rows.shape[1]), NEG_INF, F32)
    np.maximum.at(out, np.asarray(cluster_of_pos, np.int64), rows)
    return out


def group_max(rows, goff, gidx):
    """sg_group_max_rows over a CSR of row ids: an empty group gives -inf."""
    out = np.full((len(goff) - 1, rows.shape[1]), NEG_INF, F32)
    for g in range(len(goff) - 1):
        if goff[g + 1] > goff[g]:
            out[g] = rows[gidx[goff[g]:goff[g + 1]]].max(axis=0)
    return out


def group_mean(rows, goff, gidx):
    """sg_group_mean_rows in float64: an empty group gives NaN (torch.mean of nothing)."""
    out = np.full((len(goff) - 1, rows.shape[1]), np.nan, np.float64)
    with np.errstate(invalid="ignore"):
        for g in range(len(goff) - 1):
            if goff[g + 1] > goff[g]:
                out[g] = rows[gidx[goff[g]:goff[g + 1]]].astype(np.float64).sum(axis=0) / float(goff[g + 1] - goff[g])
    return out


def edge_distance(feat, adj):
    """sg_edge_distance in float64, NOT rounded: || F[a] - F[b] + 1e-6 ||_2 (cpu_ref.edge_distance is this rounded to float32)."""
    adj = np.asarray(adj, np.int64).reshape(-1, 2)
    f = np.asarray(feat, np.float64)
    d = f[adj[:, 0]] - f[adj[:, 1]] + O.PAIR_EPS
    return np.sqrt((d * d).sum(axis=1))


def contract(adj, seg_of_point, N, S):
    """sg_contract_point_edges: the sorted unique set of (min, max) segment pairs; an edge with an endpoint outside [0, N), a segment id
    < 0 or both ends in one segment is dropped.  (Segment ids >= S are outside the operator's contract: no case holds one.)"""
    adj = np.asarray(adj, np.int64).reshape(-1, 2)
    seg = np.asarray(seg_of_point, np.int64)
    assert seg.size == 0 or seg.max() < S
    ok = (adj >= 0).all(axis=1) & (adj < N).all(axis=1)
    a, b = seg[adj[ok, 0]], seg[adj[ok, 1]]
    keep = (a >= 0) & (b >= 0) & (a != b)
    pairs = np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], axis=1)
    if pairs.shape[0] == 0:
        return np.zeros((0, 2), np.int32)
    return np.unique(pairs, axis=0).astype(np.int32)


def export(unmap, seg_of_point, N, tables):
    """sg_export_labels: out[t][v] = tables[t][seg[unmap[v]]], and -1 where unmap[v] is outside [0, N) or the segment outside [0, S)."""
    unmap, seg, tables = np.asarray(unmap, np.int64), np.asarray(seg_of_point, np.int64), np.asarray(tables, np.int32)
    S = tables.shape[1]
    p_ok = (unmap >= 0) & (unmap < N)
    s = np.where(p_ok, seg[np.where(p_ok, unmap, 0)], -1)
    s_ok = (s >= 0) & (s < S)
    return np.where(s_ok[None, :], tables[:, np.where(s_ok, s, 0)], np.int32(-1)).astype(np.int32)


def centre(data, members, off):
    """sg_center_clusters' centred coordinates in float64, in MEMBER order: XYZ - mean XYZ of the position's cluster."""
    xyz = np.asarray(data, F32)[members, :3].astype(np.float64)
    out = np.empty_like(xyz)
    for c in range(len(off) - 1):
        out[off[c]:off[c + 1]] = xyz[off[c]:off[c + 1]] - xyz[off[c]:off[c + 1]].mean(axis=0)
    return out


def xyzw(data, members):
    """the kNN operand [X, Y, Z, fl(fl(X2 + Y2) + Z2)] with separately rounded squares, bit for bit"""
    p = np.asarray(data, F32)[members, :3]
    xx = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    return np.concatenate([p, xx[:, None]], axis=1).astype(F32)


def evaluate(gt, sem_pred, ins_pred, max_ins):
    """sg_evaluate: cpu_ref.evaluate, with predicted instance ids >= max_ins left out of the per-instance IoU (they still count in the
    accuracies, which compare the raw ids)."""
    iou_sem, _, acc = O.evaluate(gt, sem_pred, ins_pred)
    ins_pred = np.asarray(ins_pred)
    _, iou_ins, _ = O.evaluate(gt, sem_pred, np.where(ins_pred >= max_ins, -1, ins_pred))
    return iou_sem, iou_ins, acc


def mlp1_fp32(samples, W, idx):
    """MLP1 the way the reference formulates it, in float32 with torch on the CPU: 1x1 convolution, BatchNorm on batch statistics,
    LeakyReLU(0.2), max over the 10 neighbours, [max | mean] over the 64 samples.  `idx` [C,64,10] are the neighbours (the oracle's: the tie
    rule is the build's).  Its distance from the float64 statement is what float32 costs ANY formulation on that input."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(samples, F32))                       # [C,64,6]
    i = torch.from_numpy(np.ascontiguousarray(idx, np.int64))
    C = x.shape[0]
    nb = torch.gather(x[:, None].expand(C, 64, 64, 6), 2, i[..., None].expand(C, 64, 10, 6)).clone()       # [C,64,10,6]
    nb[..., :3] = (nb[..., :3] - nb[..., :3].mean(dim=2, keepdim=True)) * 10
    f = nb.permute(0, 3, 1, 2).contiguous()                                       # [C,6,64,10]
    w = torch.from_numpy(np.ascontiguousarray(W["mlp_1.conv1.0.weight"], F32)).reshape(64, 6, 1, 1)
    y = F.conv2d(f, w)
    y = F.batch_norm(y, None, None, torch.from_numpy(np.ascontiguousarray(W["mlp_1.bn1.weight"], F32)),
                     torch.from_numpy(np.ascontiguousarray(W["mlp_1.bn1.bias"], F32)), training=True, eps=O.BN_EPS)
    y = F.leaky_relu(y, 0.2).max(dim=-1)[0]
    return torch.cat([y.max(dim=-1)[0], y.mean(dim=-1)], dim=-1).numpy()


# ---- the float max: two integer atomics on the value's bits -----------------------------------------------------------------------------
def float_max_atomic(stored, v, split="sign bit"):
    """What one atomic_max_float(addr, v) leaves at an address holding `stored` (csrc/kernels_graph.hip): a signed max of the bits where v
    takes the non-negative path, an unsigned min where it takes the negative one.  split = "sign bit" is the rule of the library,
    "v >= 0" the earlier one, which sent -0.0 (bits of INT_MIN) down the signed path."""
    sb, vb = np.array([stored], F32).view(np.int32)[0], np.array([v], F32).view(np.int32)[0]
    positive_path = (vb >= 0) if split == "sign bit" else bool(F32(v) >= 0)
    if positive_path:
        r = np.int32(max(int(sb), int(vb)))
    else:
        r = np.array([min(int(sb) & 0xffffffff, int(vb) & 0xffffffff)], np.uint32).view(np.int32)[0]
    return np.array([r], np.int32).view(F32)[0]


ORDER_VALUES = [NEG_INF, F32(-1.0), -SUB, F32(-0.0), F32(0.0), SUB, F32(1.0), F32(np.inf)]


# ---- seeded cases ---------------------------------------------------------------------------------------------------------------------
MLP1_C = (1, 31, 32, 33, 97)
MLP1_WEIGHTS = ("as_is", "neg_gamma", "zero_gamma")
MLP1_DATA = ("far_900", "grey", "five_points", "all_identical")


def mlp1_samples(C, variant="plain", seed=0):
    """[C,64,6] float32: xyz in a 0.3 m box per cluster, rgb in [0, 1]."""
    rng = np.random.default_rng([11, C, seed])
    s = np.empty((C, 64, 6), F32)
    origin = rng.uniform(-1.0, 1.0, (C, 1, 3))
    s[..., :3] = origin + rng.uniform(0.0, 0.3, (C, 64, 3))
    s[..., 3:] = rng.uniform(0.0, 1.0, (C, 64, 3))
    if variant == "far_900":
        s[..., :3] += F32(900.0)
    elif variant == "grey":
        s[..., 3:] = 0
    elif variant == "five_points":
        s = np.tile(s[:, :5], (1, 13, 1))[:, :64].copy()
    elif variant == "all_identical":
        s[:] = s[0, 0]
    else:
        assert variant == "plain", variant
    return s


def mlp1_weights(W, variant):
    """a copy of the MLP1 entries of a weight set: as is, gamma with every 7th entry negated, gamma[9] = 0"""
    w = {k: np.array(W[k], F32) for k in ("mlp_1.conv1.0.weight", "mlp_1.bn1.weight", "mlp_1.bn1.bias")}
    if variant == "neg_gamma":
        w["mlp_1.bn1.weight"][::7] *= F32(-1.0)
    elif variant == "zero_gamma":
        w["mlp_1.bn1.weight"][9] = 0
    else:
        assert variant == "as_is", variant
    return w


def _value_columns(rng, n, far_block):
    """[n,64] rows whose channel k holds value set k % 10; where one value must beat the rest it sits in the rows `far_block` alone, so
    that (n spanning several 64-row blocks) it reaches the output through an atomic of its own"""
    v = np.empty((n, 64), F32)
    here = np.zeros(n, bool)
    here[far_block] = True
    for k in range(64):
        s = k % 10
        if s == 0:
            col = rng.uniform(-5.0, -0.1, n)                                   # all negative
        elif s == 1:
            col = rng.normal(size=n)                                           # a mix of signs
        elif s == 2:
            col = np.where(here, -0.0, -1.0)                                   # {-1.0, -0.0}
        elif s == 3:
            col = np.full(n, -0.0)                                             # {-0.0} alone
        elif s == 4:
            col = np.where(here, 0.0, -0.0)                                    # {-0.0, +0.0}
        elif s == 5:
            col = np.full(n, -np.inf)                                          # -inf rows alone
        elif s == 6:
            col = np.where(here, np.inf, rng.normal(size=n))                   # +inf
        elif s == 7:
            col = np.where(here, -SUB, -SUB * F32(50))                         # negative subnormals
        elif s == 8:
            col = np.where(here, SUB, np.where(np.arange(n) % 2 == 0, -SUB, -1.0))      # a positive subnormal above negatives
        else:
            col = np.where(here, -3.0, -np.inf)                                # -inf beside one finite negative
        v[:, k] = col
    return v


def segment_max_cases(seed=0):
    """name -> (rows [N,64], cluster_of_pos [N] non-decreasing, C)"""
    rng = np.random.default_rng([23, seed])
    cases = {}
    for n in (1, 63, 64, 65, 200):
        cases["one_cluster_%d" % n] = (rng.normal(size=(n, 64)).astype(F32), np.zeros(n, np.int32), 1)
    cases["singletons_130"] = (rng.normal(size=(130, 64)).astype(F32), np.arange(130, dtype=np.int32), 130)
    cases["boundary_at_row_64"] = (rng.normal(size=(128, 64)).astype(F32), np.repeat(np.arange(2), 64).astype(np.int32), 2)
    ids = np.repeat(np.arange(0, 3 * 35, 3), 2).astype(np.int32)              # 0,0,3,3,6,6,...: clusters 1,2,4,5,... and the last stay -inf
    cases["gaps"] = (rng.normal(size=(ids.size, 64)).astype(F32), ids, int(ids[-1]) + 2)
    # a cluster of four blocks and one of a single block, every value set in both; the deciding rows in the third block / in the middle
    four = _value_columns(rng, 256, slice(128 + 5, 128 + 9))
    one = _value_columns(rng, 64, slice(30, 33))
    cases["value_sets"] = (np.concatenate([four, one]), np.concatenate([np.zeros(256), np.ones(64)]).astype(np.int32), 2)
    # the same sets with the deciding rows in the FIRST block: whatever the arrival order of the atomics, one of the two cases has the
    # deciding value arrive at a cell that already holds another
    cases["value_sets_first_block"] = (_value_columns(rng, 256, slice(3, 6)), np.zeros(256, np.int32), 1)
    return cases


GROUP_D = (1, 64, 65, 256, 257, 300)
GROUP_FINITE_ROWS = 28                               # rows below it (but row 7) hold no -inf
GROUP_SIZES = (1, 0, 3, 4, 5, 8, 9, 1000, 0)        # one call; 1000 = a hub with repeated row ids; an empty group first-but-one and last


def group_case(D, seed=0):
    """-> rows [R, D + 5] (the 5 columns past D hold 1e30: a read past D shows), goff, gidx.  Row 7 is -inf in every column and only the
    group of one holds it; rows GROUP_FINITE_ROWS.. carry scattered -inf entries and only the small groups draw from them; the hub of
    1,000 draws (repeated ids) from the rows below, none of them -inf, so that its mean is a finite sum of 1,000 terms"""
    rng = np.random.default_rng([37, D, seed])
    R = 40
    rows = np.full((R, D + 5), 1e30, F32)
    rows[:, :D] = rng.normal(size=(R, D))
    tail = rows[GROUP_FINITE_ROWS:, :D]
    tail[rng.random(tail.shape) < 0.15] = -np.inf
    rows[7, :D] = -np.inf
    finite = np.setdiff1d(np.arange(GROUP_FINITE_ROWS), [7])
    anyrow = np.setdiff1d(np.arange(R), [7])
    groups = []
    for n in GROUP_SIZES:
        groups.append(rng.choice(finite, n, replace=True) if n > R else rng.choice(anyrow, n, replace=False))
    groups[0] = np.array([7])
    goff = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=goff[1:])
    return rows, goff, np.concatenate(groups).astype(np.int32)


EDGE_D = (1, 63, 64, 65, 127, 128, 129, 320)
EDGE_E = (1, 5, 1503)


def edge_case(D, E, scale=1.0, seed=0):
    """-> feat [S, D + 3] (1e30 past D), adj [E,2] int32; edge 0 is a self-edge"""
    rng = np.random.default_rng([41, D, E, seed])
    S = 50
    feat = np.full((S, D + 3), 1e30, F32)
    feat[:, :D] = rng.normal(size=(S, D)) * scale
    adj = rng.integers(0, S, (E, 2)).astype(np.int32)
    adj[0] = (5, 5)
    return feat, adj


CONTRACT_S = (1, 2, 181, 2900)


def contract_case(S, seed=0):
    """-> adj [E,2] int64, seg_of_point [N] int32 (every segment has a point; some points have none: -1), N.  Edges: random ones, some
    with an endpoint -1 or N, duplicates in both orders, and every pair of the 40 highest segments (the last words of the bitmap).  S = 1 has no pair and
    S = 2 one: a capacity below the count is 0 there, so "the rows up to the capacity are right" is exercised by S = 181 and 2,900 alone."""
    rng = np.random.default_rng([43, S, seed])
    N = 2 * S + 50
    seg = np.concatenate([np.arange(S), rng.integers(0, S, N - S)]).astype(np.int32)
    seg[rng.choice(np.arange(S, N), 20, replace=False)] = -1
    E = 20000 if S == 2900 else 400
    adj = rng.integers(0, N, (E, 2)).astype(np.int64)
    adj[3] = (-1, 4)
    adj[4] = (5, N)
    adj[5] = (N, -1)
    adj[6] = (0, 0)
    adj[10:20] = adj[30:40][:, ::-1]                                          # duplicates in the other order
    adj[20:30] = adj[30:40]                                                   # ... and in the same
    top = np.arange(max(S - 40, 0), S)
    a, b = np.meshgrid(top, top)
    adj = np.concatenate([adj, np.stack([a.reshape(-1), b.reshape(-1)], 1).astype(np.int64)])      # point s is in segment s
    return adj, seg, N


CENTRE_SIZES = (1, 255, 256, 257, 3000)


def centre_case(offset=0.0, seed=0):
    """-> data [N,6], members (a permutation of the points), cluster offsets, and the <= 256-position tiles of every cluster"""
    rng = np.random.default_rng([47, seed])
    N = sum(CENTRE_SIZES)
    data = rng.uniform(-1.0, 1.0, (N, 6)).astype(F32)
    data[:, :3] = data[:, :3] * F32(2.0) + F32(offset)
    members = rng.permutation(N).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(CENTRE_SIZES)]).astype(np.int32)
    tc, lo, hi, cto = [], [], [], [0]
    for c in range(len(CENTRE_SIZES)):
        for s in range(off[c], off[c + 1], 256):
            tc.append(c); lo.append(s); hi.append(min(s + 256, off[c + 1]))
        cto.append(len(tc))
    return data, members, off, tuple(np.array(x, np.int32) for x in (tc, lo, hi, cto))


EXPORT_V = (0, 1, 255, 257)


def export_case(V, seed=0):
    """-> unmap [V], seg_of_point [N], N, tables [T,S]; unmap holds -1 and N, seg holds -1 and S (where V has room for them)"""
    rng = np.random.default_rng([53, V, seed])
    N, S, T = 100, 7, 3
    seg = rng.integers(0, S, N).astype(np.int32)
    seg[10], seg[11] = -1, S
    unmap = rng.integers(0, N, V).astype(np.int32)
    if V >= 8:
        unmap[1], unmap[2], unmap[3], unmap[4] = -1, N, 10, 11
    tables = rng.integers(-1, 50, (T, S)).astype(np.int32)
    return unmap, seg, N, tables


EVAL_MAX_INS = (1, 2048, 2049, 5000)


def eval_case(V, max_ins, kind="mixed", seed=0):
    """-> gt [V,2] int32, sem_pred [V], ins_pred [V].  Predicted instance ids are spread over [0, max_ins) and some lie at and above it; the
    highest id below max_ins is present and the semantic prediction at its first valid vertex is -1 (Python's negative index wraps to class
    38); semantic predictions hold 0, 41 and -1 -- 41 never at the first valid vertex of an instance, where the reference itself raises
    an IndexError.  kind = "all_invalid": every ground-truth class is 0."""
    rng = np.random.default_rng([59, V, max_ins, seed])
    gt = np.zeros((V, 2), np.int32)
    gt[:, 0] = rng.integers(0, 41, V)
    ins = rng.integers(0, max_ins, V).astype(np.int32)                                             # the whole range
    over = rng.random(V) < 0.1
    ins[over] = max_ins + rng.integers(0, 9, int(over.sum()))                                      # ids >= max_ins: ignored
    ins[rng.random(V) < 0.1] = -1
    if V:
        ins[V // 2] = max_ins - 1
    gt[:, 1] = np.where(rng.random(V) < 0.6, ins, rng.integers(0, max_ins + 3, V))
    sem = rng.integers(-1, 42, V).astype(np.int32)                                                 # -1, 0 and 41 among them
    if kind == "all_invalid":
        gt[:, 0] = 0
    else:
        assert kind == "mixed", kind
    valid = np.nonzero(gt[:, 0] != 0)[0]
    if V and kind == "mixed":
        gt[V // 2, 0] = max(int(gt[V // 2, 0]), 1)
        valid = np.nonzero(gt[:, 0] != 0)[0]
    seen = set()
    for v in valid:                                                                                # first valid vertex of every instance
        i = int(ins[v])
        if i < 0 or i in seen:
            continue
        seen.add(i)
        if sem[v] == 41:
            sem[v] = 40
    if V and kind == "mixed":
        first = valid[ins[valid] == max_ins - 1][0]
        sem[first] = -1
    return gt, sem, ins
