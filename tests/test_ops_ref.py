"""The small operators of the scene path without a GPU ("signed zero in the float max"): the NumPy statements of
tests/ops_ref.py against oracle/cpu_ref.py on a committed scene, the seeded case generators of tests/test_gpu_ops_edges.py, a NumPy
emulation of the float max's two integer atomics, and the arguments the library refuses before the first device call."""
import ctypes as C

import numpy as np
import pytest

import ops_ref as R
from conftest import make_fixture_scene


@pytest.fixture(scope="module")
def scene(golden_index):
    from oracle import cpu_ref as O
    sc = make_fixture_scene(golden_index, "tiny_dup_4k")
    part = O.Partition(sc.weak_label[:, 1], sc.weak_label[:, 0], sc.seg)
    return sc, part, O.Layer(part)


def test_statements_agree_with_the_oracle_on_a_scene(scene, weight_sets):
    from oracle import cpu_ref as O
    sc, part, layer = scene
    N, S, V = sc.num_points, sc.num_segments, sc.unmap.shape[0]
    rng = np.random.default_rng(1)
    # contraction: the scene's mesh edges through its over-segmentation
    ref = O.contract_edges(sc.adj, part, np.arange(N), layer)
    got = R.contract(sc.adj, sc.seg, N, S)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert R.contract(np.zeros((0, 2), np.int64), sc.seg, N, S).shape == (0, 2)
    # export: a plain double gather where everything is in range
    tables = rng.integers(-1, 50, (3, S)).astype(np.int32)
    assert np.array_equal(R.export(sc.unmap, sc.seg, N, tables), tables[:, sc.seg[sc.unmap]])
    # segment max: member order, clusters contiguous
    members = np.concatenate(layer.members)
    off = np.concatenate([[0], np.cumsum([len(m) for m in layer.members])])
    rows = rng.normal(size=(N, 64)).astype(np.float32)
    cl = np.repeat(np.arange(layer.count), np.diff(off))
    assert np.array_equal(R.segment_max(rows, cl, layer.count), np.stack([rows[off[c]:off[c + 1]].max(0) for c in range(layer.count)]))
    assert np.all(R.segment_max(rows[:5], np.zeros(5, np.int32), 3)[1:] == -np.inf)
    # group max / mean and the edge distance on cluster features
    feat = rng.normal(size=(layer.count, 192)).astype(np.float32)
    groups = [rng.choice(layer.count, size=rng.integers(1, 9), replace=False) for _ in range(12)]
    goff = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    gidx = np.concatenate(groups).astype(np.int32)
    assert np.array_equal(R.group_max(feat, goff, gidx), O.group_max(feat, groups))
    assert np.allclose(R.group_mean(feat, goff, gidx), np.stack([feat[g].astype(np.float64).mean(0) for g in groups]), rtol=0, atol=1e-15)
    empty = np.array([0, 0, 2], np.int32)
    assert np.all(R.group_max(feat, empty, gidx)[0] == -np.inf) and np.isnan(R.group_mean(feat, empty, gidx)[0]).all()
    adj = rng.integers(0, layer.count, (300, 2)).astype(np.int32)
    assert np.array_equal(R.edge_distance(feat, adj).astype(np.float32), O.edge_distance(feat, adj))
    # centring: the oracle rounds the mean to float32 first, the statement stays in float64 -- one ulp of the coordinates apart
    ref9 = O.centre_per_cluster(sc.data, layer)
    assert np.abs(R.centre(sc.data, members, off) - ref9[members, 6:9]).max() <= np.spacing(np.abs(sc.data[:, :3]).max())
    # evaluate: with max_ins above every id it is the oracle's
    sem_pred = rng.integers(1, 41, V).astype(np.int32)
    ins_pred = rng.integers(-1, 6, V).astype(np.int32)
    for a, b in zip(R.evaluate(sc.gt, sem_pred, ins_pred, 6), O.evaluate(sc.gt, sem_pred, ins_pred)):
        assert np.array_equal(a, b, equal_nan=True)
    cut = R.evaluate(sc.gt, sem_pred, ins_pred, 3)
    assert cut[1].sum() < O.evaluate(sc.gt, sem_pred, ins_pred)[1].sum() and np.array_equal(cut[2], O.evaluate(sc.gt, sem_pred, ins_pred)[2], equal_nan=True)
    # MLP1 in the reference's float32 formulation is the same operator as the float64 oracle
    W = weight_sets["ins_infer"]
    samples, _ = O.sample_clusters(sc.data, layer, 64, transform=True)
    ref, idx = O.mlp1_forward(samples, W, return_knn=True)
    assert np.abs(R.mlp1_fp32(samples, W, idx) - ref).max() < 1e-5


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def test_every_generator_is_deterministic():
    calls = [lambda: R.segment_max_cases(), lambda: R.centre_case(), lambda: R.centre_case(900.0)]
    calls += [lambda C_=C_, v=v: R.mlp1_samples(C_, v) for C_ in R.MLP1_C for v in ("plain",) + R.MLP1_DATA]
    calls += [lambda D=D: R.group_case(D) for D in R.GROUP_D]
    calls += [lambda D=D, E=E, s=s: R.edge_case(D, E, s) for D in R.EDGE_D for E in R.EDGE_E for s in (1.0, 1e4)]
    calls += [lambda S=S: R.contract_case(S) for S in R.CONTRACT_S]
    calls += [lambda V=V: R.export_case(V) for V in R.EXPORT_V]
    calls += [lambda V=V, m=m, k=k: R.eval_case(V, m, k) for V in R.EXPORT_V + (4000,) for m in R.EVAL_MAX_INS for k in ("mixed", "all_invalid")]
    for call in calls:
        assert _same(call(), call())
    assert not _same(R.group_case(64, seed=0), R.group_case(64, seed=1))


def test_the_cases_hold_what_they_are_for():
    cases = R.segment_max_cases()
    rows, cl, C_ = cases["value_sets"]
    ref = R.segment_max(rows, cl, C_)
    for c in range(2):
        assert np.all(ref[c, 0::10] < 0) and np.all(ref[c, 5::10] == -np.inf) and np.all(ref[c, 6::10] == np.inf)
        for k in (2, 3, 4):
            assert np.all(ref[c, k::10] == 0)
        assert np.all(np.signbit(ref[c, 2::10])) and np.all(np.signbit(ref[c, 3::10])), "the maximum is the NEGATIVE zero"
        assert np.all(ref[c, 7::10] == -R.SUB) and np.all(ref[c, 8::10] == R.SUB) and np.all(ref[c, 9::10] == -3.0)
    rows, cl, C_ = cases["gaps"]
    assert np.all(np.diff(cl) >= 0) and np.isinf(R.segment_max(rows, cl, C_)[[1, 2, 4, C_ - 1]]).all()
    assert np.all(np.diff(cases["singletons_130"][1]) == 1) and cases["boundary_at_row_64"][1][63:65].tolist() == [0, 1]
    for D in R.GROUP_D:
        rows, goff, gidx = R.group_case(D)
        assert sorted(np.diff(goff).tolist()) == sorted(R.GROUP_SIZES)
        hub = int(np.argmax(np.diff(goff)))
        ids = gidx[goff[hub]:goff[hub + 1]]
        assert ids.size == 1000 and 20 < np.unique(ids).size < 1000, "a hub with repeated row ids"
        mean = R.group_mean(rows[:, :D], goff, gidx)
        assert np.isfinite(mean[hub]).all(), "the hub's mean is a finite sum of 1,000 terms in every channel, D = 1 included"
        assert np.all(mean[0] == -np.inf) and np.all(R.group_max(rows[:, :D], goff, gidx)[0] == -np.inf), "the group of one is the -inf row"
        if D >= 64:
            small = [g for g in range(len(goff) - 1) if 1 < goff[g + 1] - goff[g] < 10]
            assert np.isinf(mean[small]).any() and np.isfinite(mean[small]).any(), "-inf entries inside the small groups too"
    for S in R.CONTRACT_S:
        adj, seg, N = R.contract_case(S)
        assert seg.max() < S and (seg == -1).any() and (adj == -1).any() and (adj == N).any(), "no segment id >= S reaches the kernel"
        pairs = R.contract(adj, seg, N, S)
        assert (pairs.shape[0] == 0) == (S == 1)
        if S == 2900:                                            # 257 blocks of 1,024 bitmap words: the scan's second trip, and pairs in its last blocks
            words = (S * S + 31) // 32
            assert (words + 1023) // 1024 > 256
            blocks = (pairs[:, 0].astype(np.int64) * S + pairs[:, 1]) // (32 * 1024)
            assert {254, 255, 256} <= set(blocks.tolist()) and pairs.shape[0] > 15000
    for m in R.EVAL_MAX_INS:
        gt, sem, ins = R.eval_case(4000, m)
        valid = gt[:, 0] != 0
        assert ins.max() >= m and (ins[valid] == m - 1).any() and {-1, 0, 41} <= set(sem.tolist())
        assert sem[np.nonzero(valid & (ins == m - 1))[0][0]] == -1
        if m > 1:
            assert ((gt[valid, 1] == ins[valid]) & (ins[valid] >= 0) & (ins[valid] < m)).sum() > 100 and np.unique(ins[(ins >= 0) & (ins < m)]).size > min(m, 4000) // 3
        assert not (R.eval_case(4000, m, "all_invalid")[0][:, 0] != 0).any()


def test_float_max_on_integer_atomics_orders_signed_zero():
    """the rule of atomic_max_float (csrc/kernels_graph.hip) and of EdgeConv's cluster_max_out, emulated on the bits: split on the sign bit,
    every value orders correctly against every stored value; split on v >= 0 (the earlier rule), -0.0 loses to everything negative"""
    vals = R.ORDER_VALUES
    for s in vals:
        for v in vals:
            got = R.float_max_atomic(s, v)
            assert got == max(s, v), (s, v, got)
            if s != v:                                           # not a pair of zeros / the same value: the winner's bits exactly
                want = v if v > s else s
                assert got.tobytes() == np.float32(want).tobytes(), (s, v, got)
    rng = np.random.default_rng(0)
    for _ in range(200):                                         # any arrival order on top of the -inf fill
        seq = rng.choice(len(vals), rng.integers(1, 9))
        cell = R.NEG_INF
        for i in seq:
            cell = R.float_max_atomic(cell, vals[i])
        assert cell == max(vals[i] for i in seq)
    assert R.float_max_atomic(R.NEG_INF, np.float32(-0.0)) == 0 and np.signbit(R.float_max_atomic(np.float32(-1.0), np.float32(-0.0)))
    # the earlier rule: what the GPU cases {-0.0} and {-1.0, -0.0} show on a library built before the change
    assert R.float_max_atomic(R.NEG_INF, np.float32(-0.0), split="v >= 0") == -np.inf
    assert R.float_max_atomic(np.float32(-1.0), np.float32(-0.0), split="v >= 0") == -1.0
    for s in vals:
        for v in vals:
            if not (v == 0 and np.signbit(v)):
                assert R.float_max_atomic(s, v, split="v >= 0").tobytes() == R.float_max_atomic(s, v).tobytes(), "nothing else changes"


def test_library_refuses_before_the_first_device_call(sg_lib):
    from seggroup_amd import hip
    buf = (C.c_char * 1024)()                                    # never read: every call below is refused on its arguments
    p = C.addressof(buf)
    big = 1 << 40
    L = sg_lib
    calls = {
        "segment max: D = 63": (L.sg_segment_max(p, 10, 63, p, p, 64, 1, None), hip.SG_EINVAL),
        "segment max: D = 128": (L.sg_segment_max(p, 10, 128, p, p, 128, 1, None), hip.SG_EINVAL),
        "contraction: S = 46341": (L.sg_contract_point_edges(p, 1, p, 10, 46341, p, 1, p, p, big, None), hip.SG_EUNSUP),
        "contraction: S = 0": (L.sg_contract_point_edges(p, 1, p, 10, 0, p, 1, p, p, big, None), hip.SG_EINVAL),
        "contraction: short workspace": (L.sg_contract_point_edges(p, 1, p, 10, 181, p, 1, p, p, L.sg_contract_ws_bytes(181) - 512, None), hip.SG_ENOMEM),
        "edge distance: stride below D": (L.sg_edge_distance(p, 63, 64, p, 1, p, None), hip.SG_EINVAL),
        "edge distance: D = 0": (L.sg_edge_distance(p, 4, 0, p, 1, p, None), hip.SG_EINVAL),
        "MLP1: stride 127": (L.sg_mlp1_forward(p, 1, p, p, p, p, 127, p, big, None), hip.SG_EINVAL),
        "MLP1: short workspace": (L.sg_mlp1_forward(p, 33, p, p, p, p, 128, p, L.sg_mlp1_ws_bytes(33) - 256, None), hip.SG_ENOMEM),
        "evaluate: max_ins = 0": (L.sg_evaluate(p, p, p, 10, 0, p, p, p, p, big, None), hip.SG_EINVAL),
        "evaluate: max_ins = -3": (L.sg_evaluate(p, p, p, 10, -3, p, p, p, p, big, None), hip.SG_EINVAL),
        "evaluate: short workspace": (L.sg_evaluate(p, p, p, 10, 2049, p, p, p, p, L.sg_eval_ws_bytes(2049) - 256, None), hip.SG_ENOMEM),
    }
    for what, (rc, want) in calls.items():
        assert rc == want, what
    assert L.sg_segment_max(p, 10, 63, p, p, 64, 1, None) == hip.SG_EINVAL and b"D == 64" in L.sg_last_error()
    assert L.sg_contract_point_edges(p, 1, p, 10, 46341, p, 1, p, p, big, None) == hip.SG_EUNSUP and b"46341" in L.sg_last_error()
    assert L.sg_contract_ws_bytes(46340) > 46340 * 46340 // 8
