"""The training step's cluster-level operators without a GPU ("ties in the backward maxima"): the NumPy statements of
tests/train_ops_ref.py against torch float64 autograd of the reference's formulation (oracle/train_ref.py) and against torch.optim, the
tie rules the statements rest on, the seeded case generators of tests/test_gpu_train_edges.py with the conditions under which a case is
unambiguous, and the arguments the library refuses before the first device call."""
import ctypes as C

import numpy as np
import pytest
import torch

import ops_ref as R
import train_ops_ref as T


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _close(got, want, tol=1e-10):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want).max() <= tol * max(1.0, np.abs(want).max())


# ---- tie rules --------------------------------------------------------------------------------------------------------------------------
def test_torch_max_keeps_the_first_maximal_row_by_value():
    """what the statements' first_argmax claims of torch.max: both zeros are one value, the first maximal row takes the whole gradient,
    and a row id repeated in a gather keeps the gradient iff one of its positions is the first maximal one"""
    for pair, first in (([-0.0, 0.0], 0), ([0.0, -0.0], 0), ([1.0, 1.0, 1.0], 0), ([-np.inf, -np.inf], 0), ([-1.0, -0.0, 0.0], 1)):
        x = torch.tensor(pair, dtype=torch.float64).reshape(-1, 1).requires_grad_(True)
        v, i = x.max(dim=0)
        v.sum().backward()
        assert int(i) == first == int(T.first_argmax(np.array(pair).reshape(-1, 1))[0]), pair
        assert x.grad.reshape(-1).tolist() == [float(j == first) for j in range(len(pair))], pair
    x = torch.tensor([[1.0, 5.0], [3.0, 2.0], [0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    ids = [1, 0, 1, 0, 2]                                       # row 1 wins channel 0 at position 0 and is listed again at position 2
    x[ids].max(dim=0)[0].backward(torch.tensor([10.0, 20.0], dtype=torch.float64))
    assert x.grad.tolist() == [[0.0, 20.0], [10.0, 0.0], [0.0, 0.0]]
    grad, written = T.group_max_backward(x.detach().numpy(), np.array([0, 5]), np.array(ids), np.array([[10.0, 20.0]]))
    assert np.array_equal(grad, x.grad.numpy()) and written.all()


# ---- statements against autograd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("random",) + T.TAIL_CASES)
def test_tail_statement_matches_autograd(name):
    if name == "random":
        rng = np.random.default_rng(5)
        K, C_ = 9, 37
        case = dict(feat5=rng.normal(size=(C_, 256)).astype(np.float32), group=np.concatenate([np.arange(K), rng.integers(0, K, C_ - K)]).astype(np.int32),
                    gold=rng.integers(0, 40, K).astype(np.int32), keep=(rng.random((K, 128)) < 0.5).astype(np.float32) * 2, scale=0.37,
                    cls=dict(w1=rng.normal(size=(128, 256)) / 16, gamma=rng.normal(size=128), beta=rng.normal(size=128), w2=rng.normal(size=(40, 128)) / 8,
                             b2=rng.normal(size=40)))
    else:
        case = T.tail_case(name)
    st = T.tail(case["feat5"], case["group"], case["gold"], case["keep"], case["cls"], case["scale"])
    ref = T.tail_torch(case, torch.float64)
    assert abs(st["loss_sum"] - ref["loss_sum"]) <= 1e-10 * max(1.0, abs(ref["loss_sum"]))
    for k in ("gw1", "ggamma", "gbeta", "gw2", "gb2", "gfeat5"):
        assert _close(st[k], ref[k]), (name, k)
    assert np.array_equal(st["gfeat5"] != 0, ref["gfeat5"] != 0), "the same rows of Feat_5 win"


def test_tail_cases_hold_what_they_are_for():
    for name in T.TAIL_CASES:
        case = T.tail_case(name)
        ok, why = T.tail_valid(case)
        assert ok, (name, why)
        K, C_ = case["gold"].size, case["group"].size
        st = T.tail(case["feat5"], case["group"], case["gold"], case["keep"], case["cls"], case["scale"])
        assert np.isfinite(st["loss_sum"]) and all(np.isfinite(st[k]).all() for k in ("gw1", "ggamma", "gbeta", "gw2", "gb2", "gfeat5"))
        if name.startswith("K"):
            assert K == int(name[1:]) and C_ == K + 40
        if name == "K2":
            xhat = (st["feat6"] @ case["cls"]["w1"].astype(np.float64).T - st["mean"]) / np.sqrt(st["var"] + T.BN_EPS)
            assert np.abs(xhat[0] + xhat[1]).max() < 1e-9 and 0.9 < np.median(np.abs(xhat)) <= np.abs(xhat).max() < 1.0, "BatchNorm over two rows: xhat = +-1"
        elif name == "C_equals_K":
            assert C_ == K and sorted(case["group"].tolist()) == list(range(K))
        elif name == "one_big_instance":
            assert np.bincount(case["group"]).tolist() == [1] * T.TAIL_BIG + [C_ - K + 1] + [1] * (K - T.TAIL_BIG - 1)
        elif name == "duplicate_clusters":
            rows = np.nonzero(case["group"] == T.TAIL_DUP)[0]
            assert np.all(st["arg"][T.TAIL_DUP] == rows[0]) and np.all(st["gfeat5"][rows[1:]] == 0), "the first duplicate wins every channel"
        elif name == "keep_null":
            assert case["keep"] is None
        elif name == "keep_zero_row":
            assert np.array_equal(st["logits"][T.TAIL_DROPPED], case["cls"]["b2"].astype(np.float64))
        elif name == "gamma_neg_zero":
            assert case["cls"]["gamma"][5] < 0 and case["cls"]["gamma"][11] == 0 and np.all(st["dh"][:, 11] == 0)
        elif name == "w1_row7_zero":
            # h[:, 7] is 0 for every instance, so its mean, variance and xhat are 0 and ggamma[7] is exactly 0.  dh[:, 7] and gw1[7] are NOT 0:
            # with eps in the denominator BatchNorm is differentiable at a constant channel, dh = gamma / sqrt(eps) (dy - mean dy)
            assert st["mean"][7] == 0 and st["var"][7] == 0 and st["ggamma"][7] == 0
            want = case["cls"]["gamma"][7] / np.sqrt(T.BN_EPS)
            assert np.abs(st["dh"][:, 7]).max() > 0 and np.abs(st["gw1"][7]).max() > 0 and abs(want) > 100
        elif name == "gold_all_equal":
            assert np.unique(case["gold"]).size == 1
        elif name == "gold_0_39":
            assert set(case["gold"].tolist()) == {0, 39}
        elif name == "w2_x1000":
            prob = np.exp(T._log_softmax(st["logits"])).astype(np.float32)
            assert (prob == 0).mean() > 0.5 and st["loss_sum"] > 1e3, "saturated softmax: most probabilities round to 0"


@pytest.mark.parametrize("D", T.GROUPB_D)
def test_group_max_backward_statement_and_cases(D):
    case = T.group_backward_case(D)
    rows, goff, gidx, gout = case["rows"], case["goff"], case["gidx"], case["gout"]
    assert T.group_backward_gap(case) >= T.GAP
    grad, written = T.group_max_backward(rows[:, :D], goff, gidx, gout[:, :D])
    x = torch.tensor(rows[:, :D], dtype=torch.float64, requires_grad=True)
    for g in range(goff.size - 1):
        if goff[g + 1] > goff[g]:
            x[torch.as_tensor(gidx[goff[g]:goff[g + 1]].astype(np.int64))].max(dim=0)[0].backward(torch.tensor(gout[g, :D], dtype=torch.float64))
    assert np.array_equal(grad, x.grad.numpy().astype(np.float32))
    # what the case is for
    sizes = np.diff(goff).tolist()
    assert sizes == list(T.GROUPB_SIZES) and (~written).sum() == 4 and np.unique(gidx).size == written.sum()
    hub = int(np.argmax(sizes))
    ids = gidx[goff[hub]:goff[hub + 1]]
    assert ids.size == 1000 and np.unique(ids).size == 30
    first = ids[T.first_argmax(rows[ids, :D])]                  # the winner's row id is listed again after the winning position
    later = [np.nonzero(ids == first[k])[0].max() > np.nonzero(ids == first[k])[0].min() for k in range(D)]
    assert all(later), "every channel's winner is a repeated id: a later position must not clear it"
    base = len(R.GROUP_SIZES)
    same, zeros_a, zeros_b, ninf = (gidx[goff[g]:goff[g + 1]] for g in range(base, base + 4))
    assert np.all(rows[same, :D] == rows[same[0], :D]) and np.array_equal(grad[same[0], :D], gout[base, :D]) and not grad[same[1:], :D].any()
    for pair, g in ((zeros_a, base + 1), (zeros_b, base + 2)):
        assert np.all(rows[pair, :D] == 0) and np.signbit(rows[pair[0], 0]) != np.signbit(rows[pair[1], 0])
        assert np.array_equal(grad[pair[0], :D], gout[g, :D]) and not grad[pair[1], :D].any(), "both zeros are one value: the first row wins"
    assert np.signbit(rows[zeros_a[0], 0]) and not np.signbit(rows[zeros_b[0], 0])
    assert np.all(rows[ninf, 0:D:3] == -np.inf) and np.array_equal(grad[ninf[0], 0:D:3], gout[base + 3, 0:D:3]), "all -inf: the first row wins"
    if D == 192:
        assert (case["row_stride"], case["out_stride"], case["grow_stride"]) == (192, 256, 192)


def test_segment_max_backward_statement_and_cases():
    cases = T.segment_backward_cases()
    assert set(R.segment_max_cases()) < set(cases)
    for name, c in cases.items():
        rows, off, D, c0 = c["rows"], c["cl_off"], c["D"], c["col0"]
        gout = c["gout"][:, c0:c0 + D]
        if name not in T.SEGB_BUILT_TIES:
            assert T.segment_backward_gap(c) >= T.GAP, name
        grad = T.segment_max_backward(rows, off, gout)
        x = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
        for k in range(off.size - 1):
            if off[k + 1] > off[k]:
                x[int(off[k]):int(off[k + 1])].max(dim=0)[0].backward(torch.tensor(gout[k], dtype=torch.float64))
        want = x.grad.numpy().astype(np.float32) if x.grad is not None else np.zeros_like(rows)
        assert np.array_equal(grad, want), name
    empty = lambda name: np.nonzero(np.diff(cases[name]["cl_off"]) == 0)[0].tolist()
    C_ = cases["gaps"]["cl_off"].size - 1
    assert {1, 2, 4, C_ - 1} <= set(empty("gaps")) and empty("gaps_behind_empty_front")[:2] == [0, 1], "empty clusters in front, inside, at the end"
    c = cases["value_sets"]                                      # channel 4: {-0.0, +0.0} with the +0.0 rows later -- row 0 wins by value
    assert np.all(c["rows"][:256, 4] == 0) and np.signbit(c["rows"][0, 4]) and not np.signbit(c["rows"][:256, 4]).all()
    assert T.segment_max_backward(c["rows"], c["cl_off"], c["gout"][:, :64])[0, 4] == c["gout"][0, 4]
    c = cases["equal_maxima_in_two_blocks"]
    arg = T.first_argmax(c["rows"])
    assert np.all(arg[0::2] == 70) and np.all(arg[1::2] == 10) and np.all(c["rows"][150] == c["rows"][arg, np.arange(64)])
    assert cases["trainer_layout"]["col0"] == 128 and cases["trainer_layout"]["out_stride"] == 192
    assert cases["C0"]["cl_off"].size == 1 and cases["N0"]["rows"].shape[0] == 0


@pytest.mark.parametrize("name", ("random",) + T.GCN_CASES)
def test_gcn_backward_statement_matches_autograd(name):
    if name == "random":
        rng = np.random.default_rng(40)
        S, D = 40, 24
        pairs = sorted({(min(a, b), max(a, b)) for a, b in rng.integers(0, S, (300, 2)) if a != b})[:110]
        case = dict(x=rng.normal(size=(S, D)), adj=np.array(pairs, np.int32), w=rng.normal(size=(D, D)) / np.sqrt(D), gout=rng.normal(size=(S, D)), alpha=0.125)
    else:
        case = T.gcn_case(name)
        assert T.gcn_gap(case) >= T.GAP, "every pre-activation at least GAP from the ReLU's corner"
    gx, gw, pre = T.gcn_backward(case["x"], case["adj"], case["w"], case["alpha"], case["gout"])
    rx, rw = T.gcn_torch(case, torch.float64)
    assert _close(gx, rx) and _close(gw, rw), name
    if name.startswith("hubs"):
        D = case["x"].shape[1]
        deg = np.diff(case["rowptr"])
        assert deg[0] == 300 and deg[1] == 257 and deg[case["dead"]] == 0 and (deg == 0).sum() >= 2 and np.all(deg[2:] < 256)
        assert np.all(pre[case["dead"]] < 0) and (D == 1 or (pre > 0).any(axis=1).sum() == pre.shape[0] - 1), "one row dead everywhere, only that one"
        a, b = case["pair"]
        assert np.array_equal(case["x"][a], case["x"][b]) and [a, b] in case["adj"].tolist()
        e = case["adj"].tolist().index([a, b])
        assert abs(R.edge_distance(case["x"], case["adj"])[e] - np.sqrt(D) * 1e-6) < 1e-12
        assert len({tuple(sorted(p)) for p in case["adj"].tolist()}) == case["adj"].shape[0] and np.all(case["adj"][:, 0] != case["adj"][:, 1])
    elif name == "S1":
        assert case["adj"].shape == (0, 2) and case["x"].shape[0] == 1
    elif name == "S2":
        assert case["adj"].tolist() == [[1, 0]]


@pytest.mark.parametrize("smoothing", [0, 1])
def test_cross_entropy_statement_matches_reference_formula(smoothing):
    import torch.nn.functional as F
    for K, C_, scale in [(37, 40, 1.0)] + [(K, C_, s) for K in T.CE_K for C_ in T.CE_C for s in T.CE_SCALES]:
        logits, gold = T.cross_entropy_case(K, C_, scale)
        assert gold[-1] == C_ - 1 and (K == 1 or gold[0] == 0)
        loss, prob, glog = T.cross_entropy(logits, gold, smoothing, 0.125)
        x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
        g = torch.as_tensor(gold.astype(np.int64))
        if smoothing:                                            # util.py:12-29
            one_hot = torch.zeros_like(x).scatter(1, g.view(-1, 1), 1)
            one_hot = one_hot * (1 - 0.2) + (1 - one_hot) * 0.2 / (C_ - 1)
            want = -(one_hot * F.log_softmax(x, dim=1)).sum()
        else:
            want = F.cross_entropy(x, g, reduction="sum")
        (want * 0.125).backward()
        assert np.isfinite(loss) and abs(loss - want.item()) <= 1e-10 * max(1.0, abs(want.item())), (K, C_, scale)
        assert _close(glog, x.grad.numpy()) and _close(prob, torch.softmax(x.detach(), dim=1).numpy())
    K, C_ = T.CE_GRID_STRIDE
    assert K * C_ == 1024 * 256 + 16, "16 elements are left to the second trip of the backward's grid-stride loop"


@pytest.mark.parametrize("use_sgd", [True, False])
def test_optimizer_statements_match_torch_optim(use_sgd):
    for n in T.OPT_N[1:3] + (1000,):
        p0, grads = T.optimizer_case(n)
        mine, ref = T.optimizer_runs(p0, grads, use_sgd, None), T.optimizer_runs(p0, grads, use_sgd, torch.float64)
        assert len(mine) == len(ref) == T.OPT_STEPS + (0 if use_sgd else 1)
        for a, b in zip(mine, ref):
            assert np.abs(a - b).max() <= 1e-14 * max(1.0, np.abs(b).max())
            assert a[-1] == 0 and p0[-1] == 0 and not grads[:, -1].any(), "a weight of 0 with gradient 0 stays exactly 0"
    assert T.OPT_N[-1] > 1024 * 256 + 256
    assert abs(1.0 - 0.999 ** T.OPT_LATE_STEP) > 1.0 - 1e-12 and abs(1.0 - 0.9 ** T.OPT_LATE_STEP) == 1.0, "bias corrections of 1"


def test_every_generator_is_deterministic():
    calls = [lambda n=n: T.tail_case(n) for n in T.TAIL_CASES] + [lambda D=D: T.group_backward_case(D) for D in T.GROUPB_D]
    calls += [lambda: T.segment_backward_cases()] + [lambda n=n: T.gcn_case(n) for n in T.GCN_CASES]
    calls += [lambda K=K, C_=C_, s=s: T.cross_entropy_case(K, C_, s) for K in T.CE_K for C_ in T.CE_C for s in T.CE_SCALES]
    calls += [lambda n=n: T.optimizer_case(n) for n in T.OPT_N]
    for call in calls:
        assert _same(call(), call())
    assert not _same(T.group_backward_case(64, seed=0), T.group_backward_case(64, seed=1))


# ---- refused arguments ------------------------------------------------------------------------------------------------------------------------
def test_library_refuses_before_the_first_device_call(sg_lib):
    from seggroup_amd import hip
    buf = (C.c_char * 1024)()                                    # never read: every call below is refused on its arguments
    p = C.addressof(buf)
    big = 1 << 40
    L = sg_lib
    f = C.c_float(1.0)
    calls = {
        "tail forward: K = 1": (L.sg_train_tail_forward(p, 5, p, 1, p, None, p, p, p, p, big, None), hip.SG_EUNSUP),
        "tail forward: K = 0": (L.sg_train_tail_forward(p, 5, p, 0, p, None, p, p, p, p, big, None), hip.SG_EUNSUP),
        "tail forward: C = 0": (L.sg_train_tail_forward(p, 0, p, 2, p, None, p, p, p, p, big, None), hip.SG_EINVAL),
        "tail forward: short workspace": (L.sg_train_tail_forward(p, 5, p, 2, p, None, p, p, p, p, L.sg_train_tail_ws_bytes(5, 2) - 1280, None), hip.SG_ENOMEM),
        "tail backward: K = 1": (L.sg_train_tail_backward(5, 1, p, None, p, f, p, p, p, p, p, p, p, big, None), hip.SG_EINVAL),
        "tail backward: short workspace": (L.sg_train_tail_backward(5, 2, p, None, p, f, p, p, p, p, p, p, p, L.sg_train_tail_ws_bytes(5, 2) - 1280, None), hip.SG_ENOMEM),
        "tail BN statistics: K = 1": (L.sg_train_tail_bn_stats(p, big, 1, p, None), hip.SG_EINVAL),
        "group max backward: D = 0": (L.sg_group_max_rows_backward(p, 4, 0, p, p, 1, p, 4, p, 4, None), hip.SG_EINVAL),
        "segment max backward: D = 1025": (L.sg_segment_max_backward(p, 10, 1025, p, 1, p, 1025, p, p, big, None), hip.SG_EINVAL),
        "segment max backward: D = 0": (L.sg_segment_max_backward(p, 10, 0, p, 1, p, 4, p, p, big, None), hip.SG_EINVAL),
        "segment max backward: short workspace": (L.sg_segment_max_backward(p, 10, 64, p, 3, p, 64, p, p, L.sg_segment_max_backward_ws_bytes(3, 64) - 256, None),
                                                  hip.SG_ENOMEM),
        "GCN backward: D = 257": (L.sg_gcn_backward(p, 3, 257, p, 1, p, p, p, p, f, p, p, p, p, big, None), hip.SG_EINVAL),
        "GCN backward: short workspace": (L.sg_gcn_backward(p, 3, 256, p, 1, p, p, p, p, f, p, p, p, p, L.sg_gcn_backward_ws_bytes(3, 256, 1) - 1280, None),
                                          hip.SG_ENOMEM),
        "cross entropy: C = 1": (L.sg_cross_entropy_forward(p, 4, 1, p, 1, p, p, None), hip.SG_EINVAL),
        "cross entropy backward: C = 1": (L.sg_cross_entropy_backward(p, 4, 1, p, 1, f, p, None), hip.SG_EINVAL),
        "cross entropy: K = 0": (L.sg_cross_entropy_forward(p, 0, 40, p, 1, p, p, None), hip.SG_EINVAL),
        "Adam: step = 0": (L.sg_optimizer_adam(p, p, p, p, 10, f, f, 0, None), hip.SG_EINVAL),
        "Adam: step = -1": (L.sg_optimizer_adam(p, p, p, p, 10, f, f, -1, None), hip.SG_EINVAL),
        "SGD: n = -1": (L.sg_optimizer_sgd(p, p, p, -1, f, f, f, 1, None), hip.SG_EINVAL),
    }
    for what, (rc, want) in calls.items():
        assert rc == want, what
    assert L.sg_train_tail_forward(p, 5, p, 1, p, None, p, p, p, p, big, None) == hip.SG_EUNSUP and b"BatchNorm1d" in L.sg_last_error()
    assert L.sg_gcn_backward(p, 3, 257, p, 1, p, p, p, p, f, p, p, p, p, big, None) == hip.SG_EINVAL and b"D=257" in L.sg_last_error()
    assert L.sg_optimizer_adam(p, p, p, p, 10, f, f, 0, None) == hip.SG_EINVAL and b"step counts from 1" in L.sg_last_error()
    # nothing to do is not an error, and touches nothing either
    assert L.sg_group_max_rows_backward(p, 4, 4, p, p, 0, p, 4, p, 4, None) == 0 and L.sg_optimizer_sgd(p, p, p, 0, f, f, f, 1, None) == 0
    assert L.sg_segment_max_backward(p, 0, 64, p, 2, p, 64, p, p, big, None) == 0 and L.sg_segment_max_backward(p, 10, 64, p, 0, p, 64, p, p, big, None) == 0
