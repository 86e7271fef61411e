"""The one-wave kNN kernels' tile-level segment pretest (phase B: the staged segment boxes are tested 32 at once, one per lane, against the
box of the tile's 64 queries and the weakest threshold any lane holds; only the survivors reach the exact per-lane test).

The pretest may only skip work, so every table here must equal, entry for entry, the brute-force kernel's (sg_cluster_knn) and the oracle's
(cluster_knn, through `members`).  The scenes are built for what the pretest adds: clusters of <= 32, 33-64 and > 64 segments (a full, a
partial and several staged batches), random unions (most of a cluster's segments are far from any tile: mostly a rejection test), tiles
that span former clusters and former clusters without a list in the seeded kernel, coordinates far from the origin (what the slack term
9.6e-7 * (qw + box[6]) is for) and duplicated points (ties).  The bound itself is restated in NumPy float32 and held against the per-lane
bound without a GPU."""
import copy

import numpy as np
import pytest

from test_gpu_ops import _knn_layer_setup, _semantic_inputs, _up

SCENE = (2600, 520, 95, dict(min_seg=1))
DUP_SCENE = (2400, 200, 92, dict(min_seg=1, dup_frac=0.2))


@pytest.fixture(scope="module")
def env(sg_lib):
    import torch
    from seggroup_amd import hip
    hip.require_device()
    return sg_lib, torch, hip


_scenes = {}


def _scene(cfg, shift=None):
    from seggroup_amd import synthetic
    key = (cfg[:3], shift)
    if key not in _scenes:
        sc = synthetic.make_scene(cfg[0], cfg[1], cfg[2], **cfg[3])
        if shift is not None:
            sc = copy.copy(sc)
            sc.data = sc.data.copy()
            sc.data[:, :3] += np.asarray(shift, np.float32)
        _scenes[key] = sc
    return _scenes[key]


def _segments_per_cluster(sc, L):
    return np.array([len(np.unique(sc.seg[m])) for m in L.members])


def _check_against_both_references(sc, L, d, table, what):
    from oracle import cpu_ref as O
    N = sc.num_points
    brute = d["brute"].cpu().numpy()
    ref = O.cluster_knn(sc.data[:, :3], L, 20)[d["members_np"]]
    assert np.array_equal(d["members_np"][brute], ref), f"{what}: brute force != oracle"
    assert table.min() >= 0 and table.max() < N, f"{what}: entries outside the scene ({table.min()} .. {table.max()})"
    assert np.array_equal(brute, table), f"{what}: {int(np.any(brute != table, axis=1).sum())} rows differ from brute force"
    assert np.array_equal(d["members_np"][table], ref), f"{what}: table != oracle"


def _run_unseeded(env, sc, L, variant=1):
    lib, torch, hip = env
    d = _knn_layer_setup(lib, torch, hip, sc, L)
    N = sc.num_points
    out = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_cluster_knn_sorted_w(d["sxyzw"].data_ptr(), d["smpos"].data_ptr(), N, d["off"].data_ptr(), d["tc4"].data_ptr(), d["lo4"].data_ptr(),
                                          d["hi4"].data_ptr(), d["nt4"], d["cso"].data_ptr(), d["order"].data_ptr(), d["dst"].data_ptr(),
                                          d["segoff"].data_ptr(), d["co"].data_ptr(), d["box"].data_ptr(), d["cbox"].data_ptr(), d["slot"].data_ptr(), 20,
                                          d["pos0"], variant, out.data_ptr(), None))
    return d, out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [None, (100.0, -60.0, 30.0)], ids=["at-origin", "shifted-100-60-30"])
def test_staging_batch_boundaries_unseeded(env, shift):
    """One wave per tile (variant 1), clusters of 3 .. 165 segments: a batch that is not full, exactly one batch and several batches, at the
    origin and shifted by (100, -60, 30), where the scores' rounding error is what the bound's slack term has to cover."""
    sc = _scene(SCENE, shift)
    seen = []
    for target in (8, 4):
        _, L = _semantic_inputs(sc, target)
        nseg = _segments_per_cluster(sc, L)
        seen += nseg.tolist()
        assert (nseg > 64).any(), nseg
        d, table = _run_unseeded(env, sc, L)
        _check_against_both_references(sc, L, d, table, f"{target} clusters")
    seen = np.array(seen)
    assert (seen <= 32).any() and ((seen > 32) & (seen <= 64)).any() and (seen > 64).any(), seen


@pytest.mark.gpu
def test_duplicated_points_in_a_cluster_of_several_batches(env):
    """Ties (20 % duplicated points) in clusters of 38, 54 and 91 segments: the index order of equal scores must survive."""
    sc = _scene(DUP_SCENE)
    _, L = _semantic_inputs(sc, 4)
    assert (_segments_per_cluster(sc, L) > 32).any()
    d, table = _run_unseeded(env, sc, L)
    _check_against_both_references(sc, L, d, table, "duplicates")


@pytest.mark.gpu
def test_seeded_tiles_across_former_clusters(env):
    """sg_knn_seed_points + sg_cluster_knn_seeded, fine layer of 60 clusters (22 of them <= 20 points: no list, seg_prevcl = -1), coarse layers
    of 8 and 4: tiles inside one former cluster drop its segments in the pretest, tiles that span former clusters must not."""
    lib, torch, hip = env
    import oracle.cpu_ref as O
    sc = _scene(SCENE)
    N, S = sc.num_points, sc.num_segments
    part, Lf = _semantic_inputs(sc, 60)
    f = _knn_layer_setup(lib, torch, hip, sc, Lf)
    seed = torch.full((N, 20), -1, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_knn_seed_points(f["brute"].data_ptr(), f["members"].data_ptr(), N, 20, seed.data_ptr(), None))
    fine_sizes = np.diff(f["off_np"])
    cl_of_seg = np.empty(S, np.int64)
    for c, m in enumerate(Lf.members):
        cl_of_seg[np.unique(sc.seg[m])] = c
    seg_prevcl = np.where(fine_sizes[cl_of_seg] > 20, cl_of_seg, -1).astype(np.int32)
    assert (seg_prevcl >= 0).any() and (seg_prevcl < 0).any()
    d_prev = _up(torch, seg_prevcl)
    rng = np.random.default_rng(10)
    for coarse in (8, 4):                                       # keep merging the same partition
        while len(part.roots()) > coarse:
            r = part.roots()
            a, b = rng.choice(len(r), 2, replace=False)
            part.ins[r[a]] = -1
            part.union(r[a], r[b])
        Lc = O.Layer(part)
        c = _knn_layer_setup(lib, torch, hip, sc, Lc)
        # former cluster of every member position; a tile = 64 consecutive positions of one cluster
        prev_of_pos = seg_prevcl[sc.seg[c["members_np"]]]
        lo4, hi4 = c["lo4"].cpu().numpy(), c["hi4"].cpu().numpy()
        spans = mixed = 0
        for lo, hi in zip(lo4, hi4):
            u = np.unique(prev_of_pos[lo:hi])
            spans += (u >= 0).sum() >= 2
            mixed += len(u) >= 2 and u[0] < 0
        assert spans > 0, "no tile spans two former clusters"
        assert mixed > 0, "no tile holds queries with and without a seed list"
        rec_np = np.zeros((N, 4), np.float32)
        rec_np[:, :3] = sc.data[:, :3]
        rec_np[:, 3] = c["pos_of_point"].cpu().numpy().astype(np.int32).view(np.float32)
        rec = _up(torch, rec_np)
        out = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_cluster_knn_seeded(c["sxyzw"].data_ptr(), c["smpos"].data_ptr(), N, c["off"].data_ptr(), c["tc4"].data_ptr(),
                                            c["lo4"].data_ptr(), c["hi4"].data_ptr(), c["nt4"], c["cso"].data_ptr(), c["order"].data_ptr(),
                                            c["dst"].data_ptr(), c["segoff"].data_ptr(), c["co"].data_ptr(), c["box"].data_ptr(), c["cbox"].data_ptr(),
                                            c["slot"].data_ptr(), seed.data_ptr(), d_prev.data_ptr(), c["members"].data_ptr(),
                                            rec.data_ptr(), 20, c["pos0"], out.data_ptr(), None))
        _check_against_both_references(sc, Lc, c, out.cpu().numpy(), f"seeded, {coarse} clusters")


def _f32(x):
    return np.asarray(x, np.float32)


def _lane_bound(q, w, lo, hi, b6):
    """knn_device.h, box_score_bound(): one rounding per operation, in its order."""
    d = np.maximum(np.maximum(lo[:, None, :] - q, q - hi[:, None, :]), _f32(0))
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return -s * _f32(0.999999) + _f32(9.6e-7) * (w + b6[:, None])


def _tile_bound(q, w, lo, hi, b6):
    """The pretest's bound: the same expression on the box of the tile's queries and their largest w."""
    qlo, qhi, qw = q.min(axis=1), q.max(axis=1), w.max(axis=1)
    g = np.maximum(np.maximum(lo - qhi, qlo - hi), _f32(0))
    s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    return -s * _f32(0.999999) + _f32(9.6e-7) * (qw + b6)


@pytest.mark.parametrize("offset,spread,box", [(0.0, 4.0, 0.5), (0.0, 0.3, 2.0), (1000.0, 4.0, 0.5), (1000.0, 0.05, 0.0), (0.0, 1e-3, 0.0), (-1000.0, 30.0, 5.0)],
                         ids=["room", "queries-inside-the-box", "offset-1e3", "offset-1e3-degenerate-box", "degenerate-box-at-origin", "offset-minus-1e3-wide"])
def test_tile_bound_is_never_below_a_lanes_bound(offset, spread, box):
    """The exactness argument, executed: for 20,000 (box, 64-query tile) pairs per case (120,000 in all) the tile's bound, in float32 and in the
    kernel's operation order, is >= box_score_bound() of every lane -- so a segment a lane would accept is never dropped."""
    rng = np.random.default_rng(int(abs(offset)) + int(box * 10) + 7)
    P = 20000
    centre = _f32(offset + rng.uniform(-5, 5, (P, 1, 3)))
    q = _f32(centre + rng.uniform(-spread, spread, (P, 64, 3)))
    w = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
    bc = _f32(offset + rng.uniform(-5, 5, (P, 3)))
    half = _f32(rng.uniform(0, box, (P, 3)))
    half[::3] = 0                                               # every third box is a point
    lo, hi = bc - half, bc + half
    b6 = _f32((np.maximum(np.abs(lo), np.abs(hi)) ** 2).sum(axis=1))
    assert q.dtype == lo.dtype == b6.dtype == w.dtype == np.float32
    lane, tile = _lane_bound(q, w, lo, hi, b6), _tile_bound(q, w, lo, hi, b6)
    assert lane.dtype == tile.dtype == np.float32
    inside = np.all((q >= lo[:, None, :]) & (q <= hi[:, None, :]), axis=-1)
    if box >= 2.0:
        assert inside.any()
    assert np.all(tile[:, None] >= lane), f"{int((tile[:, None] < lane).sum())} lanes hold a bound above their tile's"
