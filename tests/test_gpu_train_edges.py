"""Edge shapes of the training step's cluster-level operators on the GPU ("ties in the backward maxima"): everything in
csrc/kernels_train.hip -- sg_train_tail_forward / _backward, sg_group_max_rows_backward, sg_segment_max_backward, sg_gcn_backward,
sg_cross_entropy_forward / _backward, sg_optimizer_sgd / _adam -- against the plain float64 statements of tests/train_ops_ref.py, through
the C entry points, at the sizes where the kernels change path: K = 2 and 3 instances, K on either side of the 256 threads that walk the
instances, groups that are empty, hubs with repeated row ids, rows of 257 and 300 neighbours, D past one block, more elements than one
grid, the strides and column offsets the trainer passes, both zeros, duplicates and -inf in the maxima.  Every output is written into a
larger buffer filled with a sentinel, which must survive outside the rows and columns the operator owns; workspaces have exactly the
size asked for, in front of guard bytes.  The two backward maxima only route values: their whole output is bit-equal to the statement.
Floats: 1e-4 of max(1, the tensor's largest entry) against the float64 statement is the ceiling (north_star); where a case amplifies
float32 rounding the bound is max(1e-4, 2 x the distance of the reference's own formulation run in float32 on the CPU), as in
test_gpu_ops_edges.test_mlp1_data_variants.  Observed figures (MI355X) are in each test's docstring."""
import ctypes as C

import numpy as np
import pytest

import train_ops_ref as T
from test_gpu_ops_edges import SENT, TOL, _exact_ws, _framed, _guard_intact, _inside, _up

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(sg_lib):
    import torch
    from seggroup_amd import hip
    hip.require_device()
    return sg_lib, torch, hip


def _rel(got, want):
    """max |got - want| relative to max(1, the largest entry of want), as tests/test_gpu_train.py measures"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


# ---- classifier tail ------------------------------------------------------------------------------------------------------------------------
TAIL_GRADS = ("gw1", "ggamma", "gbeta", "gw2", "gb2", "gfeat5")


@pytest.mark.parametrize("name", T.TAIL_CASES)
def test_tail_edges(env, name):
    """K = 2 (BatchNorm1d over two rows), 3, 256 and 257 (the second trip of k_tail_classifier's instance loop) with C = K + 40; C == K;
    one instance owning all but K - 1 clusters; an instance of bitwise duplicate clusters (the first wins every channel); no keep mask;
    a keep row of zeros (that instance's logits are b2, exactly); gamma with a negative and a zero entry; row 7 of w1 zero (h[:, 7] = 0:
    batch mean and ggamma[7] exactly 0, variance 0; dh[:, 7] and gw1[7] are gamma / sqrt(eps) (dy - mean dy), not 0); every gold equal;
    gold in {0, 39}; w2 x 1000 (saturated softmax, most probabilities 0, the loss finite).  Exact: Feat_6 and its argmax rows as left in
    the workspace (its first two blocks), loss[1] == K, the rows of gfeat5 that won nothing.  Floats: 1e-4; for K2, K3, w1_row7_zero and
    w2_x1000 max(1e-4, 2 x oracle/train_ref.tail under torch float32 autograd on the CPU).
    Observed on MI355X, largest relative error over loss and the six gradients: K2 2.3e-6 (the float32 reference formulation: 6.2e-5, so
    the bound is 1.24e-4), K3 7.6e-7 (3.5e-6), w1_row7_zero 6.3e-8 (2.7e-7), w2_x1000 1.3e-7 (9.5e-7), every other case at most 8.3e-8;
    logits and batch statistics at most 2.3e-7.  But for K2 the
    bound is 1e-4 in every case."""
    lib, torch, hip = env
    case = T.tail_case(name)
    K, C_ = case["gold"].size, case["group"].size
    want = T.tail(case["feat5"], case["group"], case["gold"], case["keep"], case["cls"], case["scale"])
    d_feat5, d_group, d_gold = _up(torch, case["feat5"]), _up(torch, case["group"]), _up(torch, case["gold"])
    d_keep = None if case["keep"] is None else _up(torch, case["keep"])
    d_cls = {k: _up(torch, v) for k, v in case["cls"].items()}
    cls = hip.Classifier(**{k: v.data_ptr() for k, v in d_cls.items()})
    ws, nbytes = _exact_ws(torch, lib.sg_train_tail_ws_bytes(C_, K))
    b_logits, p_logits = _framed(torch, K, T.CLS, torch.float32, float(SENT))
    b_loss, p_loss = _framed(torch, 1, 2, torch.float32, float(SENT))
    hip.check(lib.sg_train_tail_forward(d_feat5.data_ptr(), C_, d_group.data_ptr(), K, d_gold.data_ptr(), hip.ptr(d_keep), C.byref(cls), p_logits, p_loss,
                                        ws.data_ptr(), nbytes, None))
    b_bn, p_bn = _framed(torch, 1, 2 * T.H, torch.float32, float(SENT))
    hip.check(lib.sg_train_tail_bn_stats(ws.data_ptr(), nbytes, K, p_bn, None))
    shapes = dict(gw1=(T.H, T.D5), ggamma=(1, T.H), gbeta=(1, T.H), gw2=(T.CLS, T.H), gb2=(1, T.CLS), gfeat5=(C_, T.D5))
    frames = {k: _framed(torch, r, c, torch.float32, float(SENT)) for k, (r, c) in shapes.items()}
    hip.check(lib.sg_train_tail_backward(C_, K, d_gold.data_ptr(), hip.ptr(d_keep), C.byref(cls), C.c_float(case["scale"]),
                                         *[frames[k][1] for k in TAIL_GRADS], ws.data_ptr(), nbytes, None))
    got = {k: _inside(frames[k][0], *shapes[k], SENT, "sg_train_tail_backward " + k).reshape(np.shape(want[k])) for k in TAIL_GRADS}
    _guard_intact(ws, nbytes, "sg_train_tail_*")
    logits = _inside(b_logits, K, T.CLS, SENT, "sg_train_tail_forward logits")
    loss = _inside(b_loss, 1, 2, SENT, "sg_train_tail_forward loss")[0]
    bn = _inside(b_bn, 1, 2 * T.H, SENT, "sg_train_tail_bn_stats")[0]
    head = ws[:2 * K * T.D5 * 4].cpu().numpy()                  # the workspace begins with Feat_6 [K,256] float32 and its argmax rows [K,256] int32
    feat6, arg = head[:K * T.D5 * 4].view(np.float32).reshape(K, T.D5), head[K * T.D5 * 4:].view(np.int32).reshape(K, T.D5)
    # exact
    assert np.array_equal(arg, want["arg"]), f"{name}: argmax rows differ at (instance, channel) {np.argwhere(arg != want['arg'])[:1].tolist()}"
    assert np.array_equal(feat6, want["feat6"].astype(np.float32))
    assert loss[1] == K
    winners = np.zeros((C_, T.D5), bool)
    winners[want["arg"], np.arange(T.D5)] = True
    assert np.all(got["gfeat5"][~winners] == 0), "a row of Feat_5 that won no (instance, channel) has gradient 0, exactly"
    if name == "keep_zero_row":
        assert np.array_equal(logits[T.TAIL_DROPPED], case["cls"]["b2"]), "every hidden unit dropped: the logits are b2, exactly"
    if name == "w1_row7_zero":
        assert got["ggamma"][7] == 0 and bn[7] == 0 and bn[T.H + 7] <= 1e-10, "h[:, 7] = 0: xhat, the batch mean and ggamma[7] are exactly 0"
    if name == "gamma_neg_zero":
        assert np.all(got["gw1"][11] == 0), "gamma[11] = 0: nothing flows back through channel 11"
    # floats
    assert np.isfinite(loss).all() and np.isfinite(logits).all() and all(np.isfinite(v).all() for v in got.values())
    fwd = {"logits": _rel(logits, want["logits"]), "batch mean": _rel(bn[:T.H], want["mean"]), "batch variance": _rel(bn[T.H:], want["var"])}
    assert max(fwd.values()) < TOL, fwd
    err = {k: _rel(got[k], want[k]) for k in TAIL_GRADS}
    err["loss"] = _rel(loss[:1], [want["loss_sum"]])
    bound, ref_err = TOL, float("nan")
    if name in T.TAIL_AMPLIFYING:
        ref = T.tail_torch(case, torch.float32)
        ref_err = max(_rel(ref[k], want[k]) for k in TAIL_GRADS + ("loss_sum",))
        bound = max(TOL, 2.0 * ref_err)
    print(f"tail {name}: max rel |HIP - f64| = {max(err.values()):.3g} ({max(err, key=err.get)}), forward {max(fwd.values()):.3g}, "
          f"float32 reference formulation - f64 = {ref_err:.3g}, bound = {bound:.3g}")
    assert max(err.values()) < bound, (err, ref_err, bound)


# ---- group max backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.GROUPB_D)
def test_group_max_backward_edges(env, D):
    """row_stride = D + 5, out_stride = D + 7, grow_stride = D + 3 (D = 192: the trainer's 192 / 256 / 192); D on either side of the 256
    threads of a block; one call with groups of 0, 1, 3, 4, 5, 8, 9 rows, a hub of 1,000 positions over 30 row ids (the winner's id is
    listed again after the winning position: a later position must not clear it), six identical rows, {-0.0, +0.0} in each order (the
    first row wins: both zeros are one value), five rows that are -inf in every third channel (the first row wins), and four rows in no
    group, which are not written.  Pure routing: bit-equal to the statement, the sentinel intact in the stride padding."""
    lib, torch, hip = env
    c = T.group_backward_case(D)
    rows, goff, gidx, gout = c["rows"], c["goff"], c["gidx"], c["gout"]
    R_, G = rows.shape[0], goff.size - 1
    want, written = T.group_max_backward(rows[:, :D], goff, gidx, gout[:, :D])
    d_rows, d_goff, d_gidx, d_gout = _up(torch, rows), _up(torch, goff), _up(torch, gidx), _up(torch, gout)
    buf, p_out = _framed(torch, R_, c["grow_stride"], torch.float32, float(SENT))
    hip.check(lib.sg_group_max_rows_backward(d_rows.data_ptr(), c["row_stride"], D, d_goff.data_ptr(), d_gidx.data_ptr(), G, d_gout.data_ptr(),
                                             c["out_stride"], p_out, c["grow_stride"], None))
    got = _inside(buf, R_, D, SENT, "sg_group_max_rows_backward")
    assert np.all(got[~written] == SENT), "a row in no group was written"
    bad = np.argwhere((got != want) & written[:, None])
    owner = np.zeros(R_, np.int64)
    owner[gidx] = np.repeat(np.arange(G), np.diff(goff))
    assert bad.size == 0, f"D={D}: {bad.shape[0]} entries differ, in groups {np.unique(owner[bad[:, 0]]).tolist()} (sizes {np.diff(goff).tolist()})"


# ---- segment max backward ---------------------------------------------------------------------------------------------------------------------
_segb_cases = T.segment_backward_cases()


@pytest.mark.parametrize("name", sorted(_segb_cases))
def test_segment_max_backward_edges(env, name):
    """the cases of test_segment_max_edges with offsets derived from their ids (empty clusters in front, inside and at the end; 1 / 63 /
    64 / 65 / 200 rows, 130 singletons, a boundary at row 64; {-0.0, +0.0} with the -0.0 row first: it wins, both zeros are one value;
    infinities, subnormals), equal maxima in two different 64-row blocks of one cluster (the first row wins whatever the arrival order
    of the atomics), D = 1 and 70, gout at column 128 of a 192-wide buffer (the trainer's), C = 0 and N = 0 (nothing written).  Pure
    routing: bit-equal to the statement; the workspace is exactly sg_segment_max_backward_ws_bytes."""
    lib, torch, hip = env
    c = _segb_cases[name]
    rows, off, D = c["rows"], c["cl_off"], c["D"]
    N, C_ = rows.shape[0], off.size - 1
    want = T.segment_max_backward(rows, off, c["gout"][:, c["col0"]:c["col0"] + D])
    d_rows, d_off, d_gout = _up(torch, rows), _up(torch, off), _up(torch, c["gout"])
    buf, p_out = _framed(torch, N, D, torch.float32, float(SENT))
    ws, nbytes = _exact_ws(torch, lib.sg_segment_max_backward_ws_bytes(C_, D))
    hip.check(lib.sg_segment_max_backward(d_rows.data_ptr(), N, D, d_off.data_ptr(), C_, d_gout.data_ptr() + 4 * c["col0"], c["out_stride"], p_out,
                                          ws.data_ptr(), nbytes, None))
    got = _inside(buf, N, D, SENT, "sg_segment_max_backward")
    _guard_intact(ws, nbytes, "sg_segment_max_backward")
    if C_ == 0 or N == 0:
        assert np.all(got == SENT), "no cluster or no row: nothing is written"
        return
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{name}: {bad.shape[0]} of {got.size} differ, first (row, channel) {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


# ---- GCN backward -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.GCN_CASES)
def test_gcn_backward_edges(env, name):
    """S = 1 without an edge, S = 2 with one, and at D = 1, 192 and 256 a graph of 400 nodes with a row of 300 neighbours and one of 257
    (the second trip of k_gcn_bwd_rows' edge loop, taken by 44 edges and by a single one), isolated nodes, a node dead in every output
    (its gout is gated away: gx of that row is exactly 0) and an edge between two bitwise-equal rows (dist = sqrt(D) 1e-6, coefficient
    1 / dist).  Every pre-activation of the float64 statement is at least 1e-3 from 0.  Bound: 1e-4 for S1 / S2; for the hub graphs
    max(1e-4, 2 x oracle/train_ref.gcn under torch float32 autograd on the CPU).
    Observed on MI355X, relative error of gx / gw: S1 3.2e-8 / 3.3e-8, S2 8.4e-8 / 5.8e-8, hubs_D1 2.2e-8 / 7.0e-8 (the float32 reference
    formulation: 3.4e-7), hubs_D192 1.0e-7 / 5.1e-8 (4.6e-7), hubs_D256 1.1e-7 / 5.1e-8 (3.7e-7); the bound is 1e-4 in every case."""
    lib, torch, hip = env
    c = T.gcn_case(name)
    S, D = c["x"].shape
    E = c["adj"].shape[0]
    wx, ww, _ = T.gcn_backward(c["x"], c["adj"], c["w"], c["alpha"], c["gout"])
    d = {k: _up(torch, c[k]) for k in ("x", "adj", "rowptr", "col", "eid", "w", "gout")}
    b_gx, p_gx = _framed(torch, S, D, torch.float32, float(SENT))
    b_gw, p_gw = _framed(torch, D, D, torch.float32, float(SENT))
    ws, nbytes = _exact_ws(torch, lib.sg_gcn_backward_ws_bytes(S, D, E))
    hip.check(lib.sg_gcn_backward(d["x"].data_ptr(), S, D, d["adj"].data_ptr(), E, d["rowptr"].data_ptr(), d["col"].data_ptr(), d["eid"].data_ptr(),
                                  d["w"].data_ptr(), C.c_float(c["alpha"]), d["gout"].data_ptr(), p_gx, p_gw, ws.data_ptr(), nbytes, None))
    gx, gw = _inside(b_gx, S, D, SENT, "sg_gcn_backward gx"), _inside(b_gw, D, D, SENT, "sg_gcn_backward gw")
    _guard_intact(ws, nbytes, "sg_gcn_backward")
    assert np.isfinite(gx).all() and np.isfinite(gw).all()
    ex, ew = _rel(gx, wx), _rel(gw, ww)
    bound, ref_err = TOL, float("nan")
    if name.startswith("hubs"):
        assert np.all(gx[c["dead"]] == 0) and np.all(wx[c["dead"]] == 0), "a row dead in every output sends nothing back"
        rx, rw = T.gcn_torch(c, torch.float32)
        ref_err = max(_rel(rx, wx), _rel(rw, ww))
        bound = max(TOL, 2.0 * ref_err)
    print(f"gcn backward {name}: rel |HIP - f64| gx {ex:.3g}, gw {ew:.3g}; float32 reference formulation - f64 = {ref_err:.3g}, bound = {bound:.3g}")
    assert max(ex, ew) < bound, (ex, ew, ref_err, bound)


# ---- cross entropy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", T.CE_K + T.CE_GRID_STRIDE[:1])
def test_cross_entropy_edges(env, K):
    """K = 1, 255, 256, 257 (the second trip of the forward's row loop) with C = 2, 40, 41, smoothing on and off, gold at 0 and C - 1,
    logits of scale 1 and 1e4 (saturated: probabilities of exactly 0, the loss finite); K = 6,554 with C = 40, whose 262,160 elements
    leave 16 to the second trip of the backward's grid-stride loop.  The kernels accumulate in float64 and round once: 1e-6 of max(1,
    the largest entry) -- one float32 rounding, 6e-8, and the float32 smoothing constant, with a margin -- far below the 1e-4 ceiling.
    Observed on MI355X over all combinations: loss 5.7e-8, softmax 3.0e-8, glogits 6.9e-9 (relative to max(1, largest entry))."""
    lib, torch, hip = env
    combos = [(C_, sm, s) for C_ in T.CE_C for sm in (0, 1) for s in T.CE_SCALES] if K != T.CE_GRID_STRIDE[0] else [(T.CE_GRID_STRIDE[1], 1, 1.0)]
    worst = dict(loss=0.0, prob=0.0, glogits=0.0)
    for C_, smoothing, logit_scale in combos:
        logits, gold = T.cross_entropy_case(K, C_, logit_scale)
        w_loss, w_prob, w_glog = T.cross_entropy(logits, gold, smoothing, 0.125)
        d_logits, d_gold = _up(torch, logits), _up(torch, gold)
        b_prob, p_prob = _framed(torch, K, C_, torch.float32, float(SENT))
        b_loss, p_loss = _framed(torch, 1, 1, torch.float32, float(SENT))
        b_glog, p_glog = _framed(torch, K, C_, torch.float32, float(SENT))
        hip.check(lib.sg_cross_entropy_forward(d_logits.data_ptr(), K, C_, d_gold.data_ptr(), smoothing, p_prob, p_loss, None))
        hip.check(lib.sg_cross_entropy_backward(p_prob, K, C_, d_gold.data_ptr(), smoothing, C.c_float(0.125), p_glog, None))
        prob, glog = _inside(b_prob, K, C_, SENT, "sg_cross_entropy_forward"), _inside(b_glog, K, C_, SENT, "sg_cross_entropy_backward")
        loss = _inside(b_loss, 1, 1, SENT, "sg_cross_entropy_forward loss")[0]
        assert np.isfinite(loss).all() and np.isfinite(prob).all() and np.isfinite(glog).all(), (K, C_, smoothing, logit_scale)
        err = dict(loss=_rel(loss, [w_loss]), prob=_rel(prob, w_prob), glogits=_rel(glog, w_glog))
        assert max(err.values()) <= 1e-6, (K, C_, smoothing, logit_scale, err)
        if logit_scale > 1 and K * C_ > 80:
            assert (prob == 0).any(), "saturated: some probabilities are exactly 0"
        worst = {k: max(worst[k], err[k]) for k in worst}
    print(f"cross entropy K={K}: max rel |HIP - f64| " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) < TOL


# ---- optimizers -------------------------------------------------------------------------------------------------------------------------------
def _padded(torch, a):
    """a vector inside a sentinel frame of 8 elements on each side -> (buffer, view)"""
    buf = torch.full((a.size + 16,), float(SENT), device="cuda:0")
    buf[8:8 + a.size] = torch.from_numpy(a)
    return buf, buf[8:8 + a.size]


@pytest.mark.parametrize("n", T.OPT_N)
@pytest.mark.parametrize("use_sgd", [True, False], ids=["sgd", "adam"])
def test_optimizer_edges(env, use_sgd, n):
    """n = 1, 255, 257 and 1024 x 256 + 259 (the grid-stride loop's second trip), five steps with train.py:95-99's settings; SGD with
    first_step on step 1 alone (over a momentum buffer that holds 7.5, which that step must not read), Adam at steps 1..5 and once more as step 100,000 (both bias corrections 1); a weight of 0 whose
    gradient is 0 stays exactly 0.  After every step the parameters are compared with the float64 statement; the bound is measured on
    the same inputs: torch.optim in float32 on the CPU is some distance from the statement (the cost of float32), and the kernel gets
    max(2 x that, 1 ulp of |p|) per element.
    Observed on MI355X after the last call, max |HIP - f64| / max |torch float32 - f64|: SGD 8.6e-7 / 8.6e-7 at n = 262,403 and
    8.1e-9 / 6.8e-9 at n = 1; Adam 6.1e-7 / 6.1e-7 and 2.0e-9 / 1.7e-9.  n = 1 is the sharp one (the bound is that element's own): with
    `1.f - 0.999f` for 1 - beta2 in the kernel, 1.3e-5 off, Adam's first step was 5.8e-9 from the statement where torch is 1.6e-9."""
    lib, torch, hip = env
    p0, grads = T.optimizer_case(n)
    want, ref32 = T.optimizer_runs(p0, grads, use_sgd, None), T.optimizer_runs(p0, grads, use_sgd, torch.float32)
    # SGD's momentum buffer starts as 7.5: first_step = 1 overwrites it unread (torch creates the buffer at the first step)
    bufs = [_padded(torch, p0), _padded(torch, np.full(n, 7.5 if use_sgd else 0.0, np.float32)), _padded(torch, np.zeros(n, np.float32))]
    p, a, b = (v for _, v in bufs)
    for i, w in enumerate(want):
        g = _up(torch, grads[i])
        if use_sgd:
            hip.check(lib.sg_optimizer_sgd(p.data_ptr(), g.data_ptr(), a.data_ptr(), n, C.c_float(T.SGD_ARGS["lr"]), C.c_float(T.SGD_ARGS["momentum"]),
                                           C.c_float(T.SGD_ARGS["wd"]), int(i == 0), None))
        else:
            step = i + 1 if i < T.OPT_STEPS else T.OPT_LATE_STEP
            hip.check(lib.sg_optimizer_adam(p.data_ptr(), g.data_ptr(), a.data_ptr(), b.data_ptr(), n, C.c_float(T.ADAM_ARGS["lr"]), C.c_float(T.ADAM_ARGS["wd"]),
                                            step, None))
        got = p.cpu().numpy().astype(np.float64)
        ref_err = float(np.abs(ref32[i] - w).max())
        bound = np.maximum(2.0 * ref_err, np.spacing(np.abs(w).astype(np.float32)).astype(np.float64))
        err = np.abs(got - w)
        print(f"{'sgd' if use_sgd else 'adam'} n={n} call {i + 1}: max |HIP - f64| = {err.max():.3g}, torch float32 - f64 = {ref_err:.3g}")
        assert np.all(err <= bound), f"call {i + 1}: max |HIP - f64| = {err.max():.3g}; torch.optim in float32 is {ref_err:.3g} from it"
        assert n == 1 or got[-1] == 0, "a weight of 0 with gradient 0 stays exactly 0"
    for (buf, _), what in zip(bufs, ("parameters", "first state vector", "second state vector")):
        h = buf.cpu().numpy()
        assert np.all(h[:8] == SENT) and np.all(h[8 + n:] == SENT), f"wrote outside the {what}"
