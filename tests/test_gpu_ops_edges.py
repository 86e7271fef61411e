"""Edge shapes of the scene path's small operators on the GPU ("signed zero in the float max"): sg_mlp1_forward,
sg_segment_max, sg_group_max_rows / sg_group_mean_rows, sg_edge_distance, sg_contract_point_edges, sg_center_clusters, sg_export_labels
and sg_evaluate against the plain statements of tests/ops_ref.py, at the sizes where their kernels change path: one cluster, the 32-lane
boundary of MLP1's partial sums, a block spanning many clusters, empty groups and hubs, the paired / tail split of the edge distance,
the second trip of the contraction's block scan, the LDS / global split of the metric counters (max_ins = 2048 / 2049), both zeros,
infinities and subnormals in the float max.  Every output is written into a larger buffer filled with a sentinel, which must survive
outside the rows and columns the operator owns.  Integers bit-equal; floats: 1e-4 against the float64 statement is the ceiling
(north_star), the bound worked out per operator below is what is asserted beside it, and the observed maximum is in the message
(the figures measured on an MI355X are in each test's docstring)."""
import numpy as np
import pytest

import ops_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
SENT = np.float32(-7.25e11)          # float sentinel: no operator here produces it
ISENT = -77


@pytest.fixture(scope="module")
def env(sg_lib):
    import torch
    from seggroup_amd import hip
    hip.require_device()
    return sg_lib, torch, hip


def _up(torch, a):
    """upload.  The caller holds the tensor in a name until its result is read back: a temporary dropped right after `.data_ptr()` goes
    back to the caching allocator before the library is called, and the next upload of the same expression is written over it."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to("cuda:0") if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda:0")


def _framed(torch, rows, cols, dtype, sentinel):
    """[rows + 2, cols] filled with the sentinel; the operator gets the address of row 1"""
    buf = torch.full((rows + 2, cols), sentinel, dtype=dtype, device="cuda:0")
    return buf, buf[1:].data_ptr()


def _inside(buf, rows, cols, sentinel, what):
    """the operator's [rows, cols]; everything else of the frame still holds the sentinel"""
    h = buf.cpu().numpy()
    assert np.all(h[0] == sentinel) and np.all(h[rows + 1:] == sentinel), f"{what}: wrote outside its rows"
    assert np.all(h[1:rows + 1, cols:] == sentinel), f"{what}: wrote outside its columns"
    return h[1:rows + 1, :cols]


def _exact_ws(torch, nbytes):
    """a workspace of exactly nbytes in front of 256 guard bytes"""
    ws = torch.full((int(nbytes) + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    return ws, int(nbytes)


def _guard_intact(ws, nbytes, what):
    assert bool((ws[nbytes:] == 0xA5).all().item()), f"{what}: wrote past its workspace"


# ---- MLP1 -------------------------------------------------------------------------------------------------------------------------------
_mlp1_cache = {}


def _mlp1_reference(samples_key, weights_key, weight_sets):
    """float64 statement (and its kNN) of one (samples, weights) pair, computed once"""
    from oracle import cpu_ref as O
    key = (samples_key, weights_key)
    if key not in _mlp1_cache:
        samples = R.mlp1_samples(*samples_key)
        W = R.mlp1_weights(weight_sets["ins_infer"], weights_key)
        ref, idx = O.mlp1_forward(samples, W, return_knn=True)
        _mlp1_cache[key] = (samples, W, ref, idx)
    return _mlp1_cache[key]


def _mlp1_run(env, samples, W):
    lib, torch, hip = env
    C_ = samples.shape[0]
    buf, p_out = _framed(torch, C_, 192, torch.float32, float(SENT))            # feat_stride = 192 > 128
    ws, nbytes = _exact_ws(torch, lib.sg_mlp1_ws_bytes(C_))
    w, g, b = (_up(torch, W[k]) for k in ("mlp_1.conv1.0.weight", "mlp_1.bn1.weight", "mlp_1.bn1.bias"))
    d_s = _up(torch, samples)
    hip.check(lib.sg_mlp1_forward(d_s.data_ptr(), C_, w.data_ptr(), g.data_ptr(), b.data_ptr(), p_out, 192, ws.data_ptr(),
                                  nbytes, None))
    got = _inside(buf, C_, 128, SENT, "sg_mlp1_forward")
    _guard_intact(ws, nbytes, "sg_mlp1_forward")
    return got


@pytest.mark.parametrize("weights", R.MLP1_WEIGHTS)
@pytest.mark.parametrize("C_", R.MLP1_C)
def test_mlp1_cluster_counts_and_weight_variants(env, weight_sets, C_, weights):
    """C = 1, either side of the 32 lanes that sum k_mlp1_finalize's partials, and 97; gamma as trained, with negative entries, and with
    gamma[9] = 0, where the channel is LReLU(beta) exactly.  Observed on MI355X: at most 1.4e-6."""
    samples, W, ref, _ = _mlp1_reference((C_, "plain"), weights, weight_sets)
    got = _mlp1_run(env, samples, W)
    err = float(np.abs(got - ref).max())
    print(f"mlp1 C={C_} {weights}: max |HIP - f64| = {err:.3g}")
    assert np.isfinite(got).all()
    assert err < TOL, f"max |HIP - oracle| = {err:.3g}"
    if weights == "zero_gamma":
        beta = np.float32(W["mlp_1.bn1.bias"][9])
        want = max(beta, np.float32(0.2) * beta)
        assert np.all(got[:, 9] == want) and np.all(got[:, 64 + 9] == want), "gamma = 0: the channel is LReLU(beta), exactly"


@pytest.mark.parametrize("variant", R.MLP1_DATA)
def test_mlp1_data_variants(env, weight_sets, variant):
    """C = 33: a cloud 900 m from the origin (the kNN score's |x|^2 terms cancel), a colourless one (singular 6x6 covariance), clusters of
    five distinct points (score ties: the earlier candidate wins), and every sample of every cluster identical (variance 0: a = gamma /
    sqrt(1e-5) = 316 gamma amplifies the float32 rounding of the folded weights).  The bounds of `grey` and `all_identical` are not fixed in
    advance: the same input goes through the reference's own formulation in float32 (conv, batch-statistics
    BatchNorm, LeakyReLU, max: ops_ref.mlp1_fp32), its distance from the float64 statement is what float32 costs there, and the kernel
    gets max(1e-4, 2 x that) -- the factor 2 for a different but equally valid float32 order.
    Observed on MI355X, max |HIP - float64 statement|: far_900 1.4e-6, five_points 7.2e-7, grey 9.5e-7 (the float32 reference
    formulation: 6.7e-6, so the bound is 1e-4), all_identical 2.2e-5 (the float32 reference formulation: 1.4e-5, bound 1e-4)."""
    samples, W, ref, idx = _mlp1_reference((33, variant), "as_is", weight_sets)
    got = _mlp1_run(env, samples, W)
    err = float(np.abs(got - ref).max())
    bound, ref_err = TOL, float("nan")
    if variant in ("grey", "all_identical"):
        ref_err = float(np.abs(R.mlp1_fp32(samples, W, idx).astype(np.float64) - ref).max())
        bound = max(TOL, 2.0 * ref_err)
    print(f"mlp1 {variant}: max |HIP - f64| = {err:.3g}, float32 reference formulation - f64 = {ref_err:.3g}, bound = {bound:.3g}")
    assert np.isfinite(got).all()
    assert err < bound, f"max |HIP - oracle| = {err:.3g}; the float32 reference formulation is {ref_err:.3g} from it; bound {bound:.3g}"


# ---- segment max ------------------------------------------------------------------------------------------------------------------------
_segmax_cases = R.segment_max_cases()


@pytest.mark.parametrize("name", sorted(_segmax_cases))
def test_segment_max_edges(env, name):
    """by VALUE and exact: one cluster of 1 / 63 / 64 / 65 / 200 rows, 130 singletons (a block of 64 rows spans 64 clusters), a boundary at
    row 64, ascending ids with gaps (the skipped clusters stay -inf), and per channel: all negative, mixed, {-1.0, -0.0}, {-0.0},
    {-0.0, +0.0}, -inf alone, +inf, subnormals of both signs, -inf beside a finite negative -- over a cluster of four blocks, whose
    partial maxima meet in the float max's integer atomics.  A maximum of exactly -0.0 is the case the split on v >= 0 lost."""
    lib, torch, hip = env
    rows, cl, C_ = _segmax_cases[name]
    ref = R.segment_max(rows, cl, C_)
    buf, p_out = _framed(torch, C_, 70, torch.float32, float(SENT))              # out_stride = 70 > 64
    d_rows, d_cl = _up(torch, rows), _up(torch, cl)
    hip.check(lib.sg_segment_max(d_rows.data_ptr(), rows.shape[0], 64, d_cl.data_ptr(), p_out, 70, C_, None))
    got = _inside(buf, C_, 64, SENT, "sg_segment_max")
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{name}: {bad.shape[0]} of {got.size} differ, first (cluster, channel) {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {ref[tuple(bad[0])]!r}"


# ---- group max / mean ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.GROUP_D)
def test_group_max_and_mean_edges(env, D):
    """row_stride = D + 5 and out_stride = D + 7; one call with groups of 0, 1, 3, 4, 5, 8, 9 and 1,000 rows (the 4-way unroll and its
    tail; a hub with repeated row ids drawn from rows without -inf, so its mean is a finite sum of 1,000 terms), -inf entries in the
    other groups and a whole -inf row as the group of one.  Max: exact, an empty group is -inf.  Mean: the kernel sums in
    float64 and rounds once, so 1 ulp of the float64 mean (half an ulp for the rounding, the rest for the order of the float64 sum); an
    empty group is NaN.  Observed on MI355X: mean within 6e-8 of the float64 statement over all groups, within 2.9e-8 (0.5 ulp) over the
    hub of 1,000 rows, where a float32 or shortened sum would show first."""
    lib, torch, hip = env
    rows, goff, gidx = R.group_case(D)
    G = goff.size - 1
    d_rows, d_goff, d_gidx = _up(torch, rows), _up(torch, goff), _up(torch, gidx)
    ref = R.group_max(rows[:, :D], goff, gidx)
    buf, p_out = _framed(torch, G, D + 7, torch.float32, float(SENT))
    hip.check(lib.sg_group_max_rows(d_rows.data_ptr(), D + 5, D, d_goff.data_ptr(), d_gidx.data_ptr(), G, p_out, D + 7, None))
    got = _inside(buf, G, D, SENT, "sg_group_max_rows")
    assert np.array_equal(got, ref), f"D={D}: groups {np.unique(np.argwhere(got != ref)[:, 0]).tolist()} differ (sizes {np.diff(goff).tolist()})"
    assert np.all(got[np.diff(goff) == 0] == -np.inf)

    ref = R.group_mean(rows[:, :D], goff, gidx)
    buf, p_out = _framed(torch, G, D + 7, torch.float32, float(SENT))
    hip.check(lib.sg_group_mean_rows(d_rows.data_ptr(), D + 5, D, d_goff.data_ptr(), d_gidx.data_ptr(), G, p_out, D + 7, None))
    got = _inside(buf, G, D, SENT, "sg_group_mean_rows")
    assert np.isnan(got[np.diff(goff) == 0]).all() and np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got == -np.inf, ref == -np.inf) and not np.isposinf(got).any()
    hub = int(np.argmax(np.diff(goff)))
    assert np.isfinite(ref[hub]).all(), "the hub's mean is a finite sum of 1,000 terms in every channel"
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    hub_err = np.abs(got[hub] - ref[hub])
    print(f"group mean D={D}: max |HIP - f64| = {err.max():.3g}, over the hub of 1,000 rows {hub_err.max():.3g} ({(hub_err / np.spacing(np.abs(ref[hub]).astype(np.float32))).max():.2f} ulp)")
    assert err.max() < TOL, f"max |HIP - f64| = {err.max():.3g}"
    assert np.all(err <= np.spacing(np.abs(ref[fin]).astype(np.float32)) + 1e-12), f"more than 1 ulp: max |HIP - f64| = {err.max():.3g}"


# ---- edge distance ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", R.EDGE_E)
@pytest.mark.parametrize("D", R.EDGE_D)
def test_edge_distance_edges(env, D, E):
    """feat_stride = D + 3; D on either side of the paired loop's k + 64 < D and of its second trip; E = 1, 5 and 1,503 (no multiple of the
    4 edges of a block).  The kernel accumulates in float64 and rounds once: relative 1e-6 of the float64 value (one float32 rounding, 6e-8,
    with a margin of 8 ulp) for features of scale 1 and of scale 1e4, and 1e-4 absolute at scale 1; a self-edge is sqrt(D) 1e-6.
    Observed on MI355X: relative 6e-8."""
    lib, torch, hip = env
    for scale in (1.0, 1e4):
        feat, adj = R.edge_case(D, E, scale)
        ref = R.edge_distance(feat[:, :D], adj)
        buf = torch.full((E + 8,), float(SENT), device="cuda:0")
        d_feat, d_adj = _up(torch, feat), _up(torch, adj)
        hip.check(lib.sg_edge_distance(d_feat.data_ptr(), D + 3, D, d_adj.data_ptr(), E, buf[4:].data_ptr(), None))
        h = buf.cpu().numpy()
        assert np.all(h[:4] == SENT) and np.all(h[E + 4:] == SENT), "sg_edge_distance: wrote outside its E values"
        got = h[4:E + 4].astype(np.float64)
        rel = float((np.abs(got - ref) / ref).max())
        print(f"edge distance D={D} E={E} scale={scale:g}: max relative error {rel:.3g}")
        assert rel <= 1e-6, f"scale {scale:g}: max relative error {rel:.3g}"
        if scale == 1.0:
            assert np.abs(got - ref).max() < TOL
        assert abs(got[0] - np.sqrt(D) * 1e-6) <= 1e-6 * np.sqrt(D) * 1e-6, f"self-edge: {got[0]!r} against sqrt({D}) 1e-6"


# ---- contraction ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.CONTRACT_S)
def test_contract_point_edges_edges(env, S):
    """S = 1 (no pair), 2, 181 (S*S no multiple of 32) and 2,900 (257 blocks of bitmap words: the block scan's carry takes a second
    trip, and every pair of the 40 highest segments sits in its last blocks); endpoints -1 and N, segment ids -1, duplicates in both
    orders.  No segment id >= S reaches the kernel.  With out_capacity below the count the count stays full, the rows up to the capacity
    are right and nothing is written beyond it."""
    lib, torch, hip = env
    adj, seg, N = R.contract_case(S)
    ref = R.contract(adj, seg, N, S)
    n = ref.shape[0]
    d_adj, d_seg = _up(torch, adj), _up(torch, seg)
    for cap in (n + 5, n // 2):
        out = torch.full((cap + 8, 2), ISENT, dtype=torch.int32, device="cuda:0")
        cnt = torch.full((4,), ISENT, dtype=torch.int32, device="cuda:0")
        ws, nbytes = _exact_ws(torch, lib.sg_contract_ws_bytes(S))
        hip.check(lib.sg_contract_point_edges(d_adj.data_ptr(), adj.shape[0], d_seg.data_ptr(), N, S, out.data_ptr(), cap, cnt.data_ptr(),
                                              ws.data_ptr(), nbytes, None))
        h, c = out.cpu().numpy(), cnt.cpu().numpy()
        assert c[0] == n and np.all(c[1:] == ISENT), f"S={S} capacity {cap}: count {c.tolist()}, want {n}"
        k = min(n, cap)
        assert np.array_equal(h[:k], ref[:k]), f"S={S} capacity {cap}: first differing row {np.nonzero(np.any(h[:k] != ref[:k], axis=1))[0][:1].tolist()}"
        assert np.all(h[k:] == ISENT), f"S={S} capacity {cap}: wrote past row {k}"
        _guard_intact(ws, nbytes, "sg_contract_point_edges")


# ---- centring -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 900.0])
def test_center_clusters_edges(env, offset):
    """clusters of 1, 255, 256, 257 and 3,000 points (one tile, a full tile, a tile of one point, twelve tiles) in one call, in a
    permuted member order, around the origin and 900 m away.  The mean is summed in float64 and rounded to float32 once, then one float32
    subtraction: 2 ulp of the largest coordinate against the float64 statement (1.2e-4 at 900 m).  Copies, the zero padding and the kNN
    operand [x, y, z, fl(fl(x2 + y2) + z2)] are exact."""
    lib, torch, hip = env
    data, members, off, (tc, lo, hi, cto) = R.centre_case(offset)
    N, C_, T = data.shape[0], off.size - 1, tc.size
    d = [_up(torch, x) for x in (data, members, off, tc, lo, hi, cto)]
    b9, p9 = _framed(torch, N, 12, torch.float32, float(SENT))
    b4, p4 = _framed(torch, N, 4, torch.float32, float(SENT))
    ws, nbytes = _exact_ws(torch, lib.sg_center_ws_bytes(T, C_))
    hip.check(lib.sg_center_clusters(d[0].data_ptr(), N, d[1].data_ptr(), d[2].data_ptr(), C_, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), T,
                                     d[6].data_ptr(), p9, p4, ws.data_ptr(), nbytes, None))
    got9, got4 = _inside(b9, N, 12, SENT, "sg_center_clusters x9m"), _inside(b4, N, 4, SENT, "sg_center_clusters xyzw")
    _guard_intact(ws, nbytes, "sg_center_clusters")
    assert np.array_equal(got9[:, :6], data[members]) and np.all(got9[:, 9:] == 0)
    assert np.array_equal(got4, R.xyzw(data, members))
    err = float(np.abs(got9[:, 6:9] - R.centre(data, members, off)).max())
    bound = 2.0 * float(np.spacing(np.abs(data[:, :3]).max()))
    print(f"centre offset={offset:g}: max |HIP - f64| = {err:.3g}, bound {bound:.3g}")
    assert err <= bound, f"max |HIP - f64| = {err:.3g} > 2 ulp = {bound:.3g}"
    assert np.all(got9[0, 6:9] == 0), "a cluster of one point is its own mean"


# ---- export / evaluate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", R.EXPORT_V)
def test_export_labels_edges(env, V):
    """V = 0, 1, 255, 257; unmap entries -1 and N and segment ids -1 and S give -1"""
    lib, torch, hip = env
    unmap, seg, N, tables = R.export_case(V)
    T, S = tables.shape
    ref = R.export(unmap, seg, N, tables)
    buf = torch.full((T * V + 16,), ISENT, dtype=torch.int32, device="cuda:0")
    d_unmap, d_seg, d_tables = _up(torch, unmap), _up(torch, seg), _up(torch, tables)
    hip.check(lib.sg_export_labels(d_unmap.data_ptr(), V, d_seg.data_ptr(), N, d_tables.data_ptr(), T, S,
                                   buf[8:].data_ptr(), None))
    h = buf.cpu().numpy()
    assert np.all(h[:8] == ISENT) and np.all(h[8 + T * V:] == ISENT), "sg_export_labels: wrote outside its T x V values"
    assert np.array_equal(h[8:8 + T * V].reshape(T, V), ref)
    if V >= 8:
        assert np.all(ref[:, 1:5] == -1)


EVAL_CASES = [(V, m, "mixed") for V in R.EXPORT_V for m in (1, 2049)] + [(4000, m, "mixed") for m in R.EVAL_MAX_INS] + \
             [(4000, 2048, "all_invalid"), (4000, 5000, "all_invalid")]


@pytest.mark.parametrize("V,max_ins,kind", EVAL_CASES, ids=["V%d-ins%d-%s" % c for c in EVAL_CASES])
def test_evaluate_edges(env, V, max_ins, kind):
    """max_ins = 1, 2,048 (the per-instance counters still fit the block's LDS), 2,049 and 5,000 (global atomics), ids over the whole
    range; ids >= max_ins ignored; every ground-truth class 0; semantic predictions 0, 41 and -1; -1 at the first vertex of the highest
    instance id (Python's negative index: class 38).  Counts are integers: exact against cpu_ref.evaluate."""
    lib, torch, hip = env
    gt, sem, ins = R.eval_case(V, max_ins, kind)
    ref = R.evaluate(gt, sem, ins, max_ins)
    iou_s, iou_i, acc = np.full(80, SENT, np.float32), np.full(80, SENT, np.float32), np.full(4, SENT, np.float32)
    ws, nbytes = _exact_ws(torch, lib.sg_eval_ws_bytes(max_ins))
    d_gt, d_sem, d_ins = _up(torch, gt), _up(torch, sem), _up(torch, ins)
    hip.check(lib.sg_evaluate(d_gt.data_ptr(), d_sem.data_ptr(), d_ins.data_ptr(), V, max_ins,
                              iou_s.ctypes.data, iou_i.ctypes.data, acc.ctypes.data, ws.data_ptr(), nbytes, None))
    _guard_intact(ws, nbytes, "sg_evaluate")
    assert np.array_equal(iou_s.reshape(1, 2, 40), ref[0])
    assert np.array_equal(iou_i.reshape(1, 2, 40), ref[1]), f"classes {np.nonzero(np.any(iou_i.reshape(2, 40) != ref[1][0], axis=0))[0].tolist()} differ"
    assert np.allclose(acc, ref[2], rtol=0, atol=1e-7, equal_nan=True)
    if kind == "all_invalid" or V == 0:
        assert np.isnan(acc).all() and not iou_s.any() and not iou_i.any()
    elif max_ins > 1 and V >= 255:
        assert ref[1][0, 0].sum() > 0 and ref[1][0, :, 38].sum() > 0, "the case holds matched instances and the wrapped class"
