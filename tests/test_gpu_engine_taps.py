"""Stage-level float parity of the scene engine (sg_engine_submit_debug) -- the code bench.py times and infer.py runs by default.

The label-level engine tests (tests/test_gpu_scene.py) cannot see a float error that moves no scene across a grouping threshold.
Here every scene of a batch leaves its stage taps -- FPS samples, MLP1 features, the member-order kNN tables, the cluster features in
front of each GCN (featA: what the batched EdgeConv, its BatchNorm folds and k_cluster_affine_b produce), the GCN outputs and the
decision distances, the adjacency lists -- and they are compared with
  * the single-scene pipeline (sg_pipeline_forward with the same taps): integer taps bit-exact, float taps bit-exact wherever the
    engine walks the scene's EdgeConv tile groups with as many workgroups as the single-scene launch does (include/seggroup_hip.h),
    within ENGINE_TOL elsewhere;
  * the float64 oracle (cpu_ref.forward_scene(..., keep=True)): the keys and tolerances of test_stage_taps_match_oracle.

The scenes sit where batching goes wrong: a ragged group (a 150k-point scan beside scenes of 4k, 20k and 90 points), clusters smaller
than the 20 neighbours of the kNN (padded rows), a scan ~900 m from the origin (second moments of the BatchNorm folds), a hub cluster
with more than 256 neighbours (the GCN's unstaged rows), and one scene of SG_MAX_POINTS points."""
import os

import numpy as np
import pytest

from conftest import ROOT, make_fixture_scene

pytestmark = pytest.mark.gpu
FLOAT_TOL = 1e-4            # north-star tolerance against the oracle (test_stage_taps_match_oracle)
SAMPLE_TOL = 1e-5           # FPS samples against the oracle (test_stage_taps_match_oracle)
ENGINE_TOL = 1e-5           # engine vs pipeline where the BatchNorm partial sums are added in another association (the maxima are printed)
SHAPES = [(1, 1), (1, 6), (3, 4), (2, 8)]           # groups x scenes per group; 2 x 8 has more slots than the batch has scenes


def hub_scene(n_ring=360, ring_pts=16, floor_pts=9000, seed=5):
    """A disc-shaped floor segment (9,000 points) ringed by 360 small segments that touch it.  Every segment carries its own weak
    instance label, so no two segments ever merge (label veto): the floor is one cluster with ~300 cluster neighbours in every layer."""
    from scipy.spatial import cKDTree
    from seggroup_amd import synthetic
    rng = np.random.default_rng(seed)
    R0, width = 2.0, 0.08
    r_f = R0 * np.sqrt(rng.uniform(0, 1, floor_pts))
    a_f = rng.uniform(0, 2 * np.pi, floor_pts)
    k = np.repeat(np.arange(n_ring), ring_pts)
    a_r = (k + rng.uniform(0, 1, k.size)) * (2 * np.pi / n_ring)
    r_r = R0 + width * rng.uniform(0, 1, k.size)
    r, a = np.concatenate([r_f, r_r]), np.concatenate([a_f, a_r])
    lab = np.concatenate([np.zeros(floor_pts, np.int64), 1 + k])
    n = r.size
    perm = rng.permutation(n)
    r, a, lab = r[perm], a[perm], lab[perm]
    data = np.empty((n, 6), np.float32)
    data[:, 0] = 4.0 + r * np.cos(a)
    data[:, 1] = 3.0 + r * np.sin(a)
    data[:, 2] = rng.uniform(0, 0.01, n)
    data[:, 3:] = rng.uniform(-1, 1, (n, 3))
    seg = synthetic._renumber_by_first_point(lab)
    xyz = data[:, :3].astype(np.float64)
    _, nb = cKDTree(xyz).query(xyz, k=7)
    src = np.repeat(np.arange(n, dtype=np.int64), 6)
    dst = nb[:, 1:].reshape(-1).astype(np.int64)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    adj = np.stack([key // n, key % n], 1).astype(np.int64)
    sem = np.where(lab == 0, 1, 2 + lab % 38)
    weak = np.stack([sem, lab], 1).astype(np.int64)
    gt = np.stack([sem + 1, lab + 1], 1).astype(np.int64)
    return synthetic.Scene(name="hub", data=data, weak_label=weak, seg=seg.astype(np.int32), adj=adj, unmap=np.arange(n, dtype=np.int64), gt=gt)


def far_scene():
    """test_scan_far_from_the_origin_matches_oracle's construction, ~900 m out instead of ~100 m"""
    from seggroup_amd import synthetic
    sc = synthetic.make_scene(20000, 200, 9100)
    sc.data[:, 0] += np.float32(903.0)
    sc.data[:, 1] -= np.float32(871.0)
    sc.data[:, 2] += np.float32(41.0)
    return sc


def _weights(mode_name):
    from seggroup_amd import weights
    return weights.load_npz(os.path.join(ROOT, "tests", "golden", "weights_g1.npz" if mode_name == "sem_infer" else "weights_g2.npz"))


def _alloc(ds):
    """Zeroed tap buffers for one scene and the hip.Debug that points at them."""
    import torch
    from seggroup_amd import hip
    N, S, E, dev = ds.N, ds.S, max(ds.E0, 1), "cuda:0"
    t = dict(samples1=torch.zeros(S, 64, 6, device=dev), feat1=torch.zeros(S, 128, device=dev),
             knn=[torch.full((N, 20), -1, dtype=torch.int32, device=dev) for _ in range(2)],
             members=[torch.full((N,), -1, dtype=torch.int32, device=dev) for _ in range(2)],
             cat=[torch.zeros(S, 192, device=dev), torch.zeros(S, 256, device=dev)],
             gcn=[np.zeros((S, 192), np.float32), np.zeros((S, 256), np.float32)],
             dist=[np.zeros(E, np.float32) for _ in range(3)], adj=[np.zeros((E, 2), np.int32) for _ in range(4)])
    d = hip.Debug()
    d.d_samples1, d.d_feat1 = t["samples1"].data_ptr(), t["feat1"].data_ptr()
    for i in range(2):
        d.d_knn[i], d.d_members[i], d.d_cat[i] = t["knn"][i].data_ptr(), t["members"][i].data_ptr(), t["cat"][i].data_ptr()
        d.h_gcn[i] = t["gcn"][i].ctypes.data
    for i in range(3):
        d.h_dist[i] = t["dist"][i].ctypes.data
    for i in range(4):
        d.h_adj[i] = t["adj"][i].ctypes.data
        d.n_adj[i] = -1
    return t, d


def _collect(t, d, res, ins):
    """Host arrays of what a forward filled: kNN tables as point ids (order included), the first C rows of the cluster taps."""
    import torch
    torch.cuda.synchronize()
    n_adj = list(d.n_adj)
    out = dict(trace=list(res.trace), n_adj=n_adj, samples1=t["samples1"].cpu().numpy(), feat1=t["feat1"].cpu().numpy(),
               digest=_digest(res))
    nlay = 2 if ins else 1
    out["adj"] = [t["adj"][i][:n_adj[i]].copy() for i in range(2 * nlay)]
    out["dist"] = [t["dist"][i][:n_adj[i]].copy() for i in range(1 + 2 * (nlay - 1))]
    if ins:
        for key in ("knn", "cat", "gcn"):
            out[key] = []
        for i in range(2):
            members = t["members"][i].cpu().numpy()
            knn_pts = np.full((members.shape[0], 20), -1, np.int64)
            knn_pts[members] = members[t["knn"][i].cpu().numpy()]
            out["knn"].append(knn_pts)
            C, D = res.trace[1 + i], (192, 256)[i]
            out["cat"].append(t["cat"][i].cpu().numpy().reshape(-1)[:C * D].reshape(C, D))
            out["gcn"].append(t["gcn"][i].reshape(-1)[:C * D].reshape(C, D).copy())
    return out


def _digest(res):
    import bench
    return bench.label_digest(res)


def _float_taps(o):
    yield "feat1", o["feat1"]
    for i, d in enumerate(o["dist"]):
        yield f"dist{i}", d
    for i in range(len(o.get("cat", []))):
        yield f"cat{i + 2}", o["cat"][i]
        yield f"gcn{i + 2}", o["gcn"][i]


def _maxdiff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.size else 0.0


def compare_with_pipeline(got, want, exact, tag):
    """Integer taps and samples bit-exact; float taps bit-exact if `exact`, else within ENGINE_TOL (the maxima are printed)."""
    assert got["trace"] == want["trace"], tag
    assert got["digest"] == want["digest"], f"{tag}: labels / metrics"
    assert got["n_adj"] == want["n_adj"], f"{tag}: adjacency rows"
    for i, (a, b) in enumerate(zip(got["adj"], want["adj"])):
        assert np.array_equal(a, b), f"{tag}: adj_{i + 1}"
    for i, (a, b) in enumerate(zip(got.get("knn", []), want.get("knn", []))):
        assert np.array_equal(a, b), f"{tag}: layer {i + 2} kNN table (as point ids, order included)"
    assert got["samples1"].tobytes() == want["samples1"].tobytes(), f"{tag}: FPS samples"
    worst = {}
    for (nm, a), (_, b) in zip(_float_taps(got), _float_taps(want)):
        assert a.shape == b.shape, (tag, nm)
        worst[nm] = _maxdiff(a, b)
        if exact:
            assert a.tobytes() == b.tobytes(), f"{tag}: {nm} differs from the single-scene pipeline by up to {worst[nm]:.3g} (expected bit-identical)"
        else:
            assert worst[nm] <= ENGINE_TOL, f"{tag}: {nm} differs from the single-scene pipeline by {worst[nm]:.3g}"
    print(f"ENGINE-vs-PIPELINE {tag} exact={exact} " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


def compare_with_oracle(got, ref, tag):
    st = ref["stages"]
    assert got["trace"][:len(ref["trace"])] == ref["trace"], tag
    obs = {"samples": _maxdiff(got["samples1"], st["samples"])}
    assert obs["samples"] < SAMPLE_TOL, (tag, obs)
    adjs = [st["adj1"], st["adj2"]] + ([st["mlp_2"]["adj"], st["mlp_3"]["adj"]] if "knn" in got else [])
    for i, a in enumerate(adjs):
        assert got["n_adj"][i] == a.shape[0] and np.array_equal(got["adj"][i], a), f"{tag}: adj_{i + 1} vs the oracle"
    obs["feat1"] = _maxdiff(got["feat1"], st["feat1"])
    obs["d1"] = _maxdiff(got["dist"][0], st["d1"])
    if "knn" in got:
        for i, nm in enumerate(("mlp_2", "mlp_3")):
            assert np.array_equal(got["knn"][i], st[nm]["knn"]), f"{tag}: {nm} kNN table vs the oracle"
            obs[f"{nm}.cat"] = _maxdiff(got["cat"][i], st[nm]["cat"])
            obs[f"{nm}.gcn"] = _maxdiff(got["gcn"][i], st[nm]["gcn"])
            obs[f"{nm}.d"] = _maxdiff(got["dist"][1 + i], st[nm]["d"])
    print(f"ENGINE-vs-ORACLE {tag} " + " ".join(f"{k}={v:.2e}" for k, v in obs.items()))
    bad = {k: v for k, v in obs.items() if k != "samples" and not v < FLOAT_TOL}
    assert not bad, f"{tag}: taps off the oracle by more than {FLOAT_TOL}: {bad} (all maxima: {obs})"


def _exact_expected(N, per_group):
    """The engine gives a scene min(its tile groups, 2 x CUs / scenes in the super-step) EdgeConv workgroups, the single-scene launch
    min(its tile groups, 2 x CUs); a super-step holds at most per_group scenes.  Equal counts -> the same partial sums in the same order."""
    import torch
    resident = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    groups = -(-N // 128)
    return per_group == 1 or groups <= max(1, resident // per_group)


def run_pipeline(W, caps, scenes, mode):
    from seggroup_amd import hip
    from seggroup_amd.model import Pipeline
    pipe = Pipeline(W, *caps, device="cuda:0")
    out = []
    for ds in scenes:
        t, d = _alloc(ds)
        res = pipe.forward(ds, mode, d)
        out.append(_collect(t, d, res, mode == hip.MODE_INS_INFER))
    pipe.close()
    return out


def run_engine(W, caps, scenes, mode, groups, per_group, knn_variant=None):
    from seggroup_amd import hip
    from seggroup_amd.model import Engine
    eng = Engine(W, caps, groups=groups, per_group=per_group, device="cuda:0", timing=0)
    if knn_variant is not None:
        eng.set_knn_variant(knn_variant)
    taps = [_alloc(ds) for ds in scenes]
    res = eng.run(scenes, mode, debug=[d for _, d in taps])
    out = [_collect(t, d, r, mode == hip.MODE_INS_INFER) for (t, d), r in zip(taps, res)]
    eng.close()
    return out


def _caps(scenes):
    return (max(s.N for s in scenes), max(s.S for s in scenes), max(s.E0 for s in scenes), max(s.V for s in scenes))


@pytest.fixture(scope="module")
def ins_batch(golden_index):
    """The ins_infer batch: the ragged group first (one 150k-point scan, three small fixtures, 90 points), then the scenes of small
    clusters, far from the origin and with a hub.  Oracle and pipeline taps are computed once."""
    from oracle import cpu_ref
    from seggroup_amd import hip, synthetic
    from seggroup_amd.scene import DeviceScene
    host = {nm: make_fixture_scene(golden_index, nm) for nm in ("scene_150k", "tiny_4k", "tiny_dup_4k", "island_20k")}
    host["mini_90"] = synthetic.make_scene(90, 3, 5, min_seg=4)
    host["small_clusters"] = synthetic.make_scene(2500, 120, 124, min_seg=1)
    host["far_900m"] = far_scene()
    host["hub"] = hub_scene()
    names = list(host)
    W = _weights("ins_infer")
    scenes = [DeviceScene.from_synthetic(host[nm], device="cuda:0") for nm in names]
    oracle = [cpu_ref.forward_scene(host[nm], W, "ins_infer", keep=True) for nm in names]
    caps = _caps(scenes)
    pipe = run_pipeline(W, caps, scenes, hip.MODE_INS_INFER)
    return dict(names=names, host=host, scenes=scenes, oracle=oracle, pipe=pipe, caps=caps, W=W)


def test_the_batch_reaches_the_cases_it_is_for(ins_batch):
    """No vacuous pass: the hub row exceeds the GCN's staged degree (256) in both layers, the small-cluster scene has clusters of
    fewer than 20 points (padded kNN rows), the ragged group mixes sizes, and the pipeline agrees with the oracle's trace."""
    b = ins_batch
    for nm, o, ref in zip(b["names"], b["pipe"], b["oracle"]):
        assert o["trace"] == ref["trace"], nm
    hub = b["pipe"][b["names"].index("hub")]
    for i in (1, 2):                                               # adjacency in front of the L2 / L3 GCN
        deg = np.bincount(hub["adj"][i].reshape(-1))
        assert deg.max() > 256, f"hub scene: largest cluster degree {deg.max()} in front of GCN {i + 1}"
    st = b["oracle"][b["names"].index("small_clusters")]["stages"]
    for nm in ("mlp_2", "mlp_3"):
        assert min(len(m) for m in st[nm]["members"]) < 20, nm
    sizes = [s.N for s in b["scenes"][:5]]
    assert max(sizes) == 150000 and min(sizes) < 100


@pytest.mark.parametrize("groups,per_group", SHAPES, ids=[f"{g}x{b}" for g, b in SHAPES])
def test_engine_taps_match_pipeline_and_oracle(ins_batch, groups, per_group):
    from seggroup_amd import hip
    b = ins_batch
    got = run_engine(b["W"], b["caps"], b["scenes"], hip.MODE_INS_INFER, groups, per_group)
    for nm, ds, g, p, ref in zip(b["names"], b["scenes"], got, b["pipe"], b["oracle"]):
        tag = f"{groups}x{per_group}/{nm}"
        compare_with_pipeline(g, p, _exact_expected(ds.N, per_group), tag)
        compare_with_oracle(g, ref, tag)


@pytest.mark.parametrize("variant", [8, 1, 2])
def test_engine_knn_variants_on_the_ragged_group(ins_batch, variant):
    """sg_engine_set_knn_variant: every batched kNN kernel gives the pipeline's table, so every tap equals the pipeline's."""
    from seggroup_amd import hip
    b = ins_batch
    got = run_engine(b["W"], b["caps"], b["scenes"][:5], hip.MODE_INS_INFER, 1, 6, knn_variant=variant)
    for nm, ds, g, p in zip(b["names"][:5], b["scenes"][:5], got, b["pipe"][:5]):
        compare_with_pipeline(g, p, _exact_expected(ds.N, 6), f"knn{variant}/1x6/{nm}")


def test_engine_taps_in_sem_infer_mode(ins_batch):
    """sem_infer stops after the structural layer: samples, MLP1 features, adj_1 / adj_2 and the first decision distances."""
    from oracle import cpu_ref
    from seggroup_amd import hip
    b = ins_batch
    W = _weights("sem_infer")
    pick = [b["names"].index(nm) for nm in ("island_20k", "far_900m")]
    scenes = [b["scenes"][i] for i in pick]
    want = run_pipeline(W, b["caps"], scenes, hip.MODE_SEM_INFER)
    for groups, per_group in ((1, 1), (1, 6)):
        got = run_engine(W, b["caps"], scenes, hip.MODE_SEM_INFER, groups, per_group)
        for i, g, p in zip(pick, got, want):
            tag = f"sem/{groups}x{per_group}/{b['names'][i]}"
            compare_with_pipeline(g, p, True, tag)
            compare_with_oracle(g, cpu_ref.forward_scene(b["host"][b["names"][i]], W, "sem_infer", keep=True), tag)


def test_engine_taps_at_the_largest_scene_size():
    """One scene of SG_MAX_POINTS points (oracle too slow): alone in a group it is bit-identical to the pipeline; beside two
    small scenes its EdgeConv walks fewer workgroups, and its float taps stay within ENGINE_TOL."""
    from seggroup_amd import hip, synthetic
    from seggroup_amd.scene import DeviceScene
    W = _weights("ins_infer")
    host = [synthetic.make_scene(1 << 20, 8000, 77), synthetic.make_scene(3000, 30, 40002),
            synthetic.make_scene(3000, 150, 41003, min_seg=1)]
    assert host[0].num_points == 1 << 20
    scenes = [DeviceScene.from_synthetic(s, device="cuda:0") for s in host]
    del host
    caps = _caps(scenes)
    want = run_pipeline(W, caps, scenes, hip.MODE_INS_INFER)
    got = run_engine(W, caps, scenes[:1], hip.MODE_INS_INFER, 1, 1)
    compare_with_pipeline(got[0], want[0], True, "1x1/max_points")
    got = run_engine(W, caps, scenes, hip.MODE_INS_INFER, 1, 3)
    for nm, ds, g, p in zip(("max_points", "small_a", "small_b"), scenes, got, want):
        compare_with_pipeline(g, p, _exact_expected(ds.N, 3), f"1x3/{nm}")
