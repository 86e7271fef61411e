"""Global registration on the GPU (seggroup_amd/register.py) against tests/register_ref.py: sg_fpfh's bin counts integer
for integer and its descriptors within one fp32 ulp on every decided point, sg_feature_nearest bit-equal to the NumPy float32 statement,
sg_ransac_count's rejections exactly and its counts between the reference's two radii, and the pipeline: a coarse pose inside ICP's
basin from 150 degrees and 1.5 m away, from which ICP ends where it ends from the true pose -- and does not without it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import pcseg_radius_ref as Q
import pcseg_ref as R
import register_ref as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


_rooms = {}


def _described(seed):
    """register_ref.describe of jittered_room(seed, 1500, 1e-3) at the radii 0.15 / 0.30, once per process, with the cloud as `xyz`"""
    if seed not in _rooms:
        xyz = G.jittered_room(seed, 1500, 1e-3)
        _rooms[seed] = dict(G.describe(xyz, 0.15, 0.30), xyz=xyz)
    return _rooms[seed]


# ---- sg_fpfh --------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def _ulps(got, want):
    """the distance in units of the last place between two arrays of non-negative fp32"""
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def _check_fpfh(xyz, nrm, off, idx, stride=3, what=""):
    """one call against the reference -> (spfh, fpfh) as the device wrote them"""
    from seggroup_amd import register
    ref = G.fpfh(xyz, nrm, off, idx)
    rows = xyz if stride == 3 else np.ascontiguousarray(np.concatenate([xyz, np.full((xyz.shape[0], stride - 3), 7.0, np.float32)], 1))
    out, hist = register.fpfh(rows, nrm, None, lists=(off, idx), want_spfh=True, device=DEV)
    out, hist = out.cpu().numpy(), hist.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (xyz.shape[0], 33) and hist.dtype == np.int32 and hist.shape == (xyz.shape[0], 34)
    ok = ~ref["undecided"]
    assert (~ok).mean() <= 0.01 if ok.size else True, (what, int((~ok).sum()))
    assert np.array_equal(hist[ok], ref["spfh"][ok]), what
    worst = int(_ulps(out[ok], ref["fpfh"][ok]).max()) if ok.any() else 0
    assert worst <= 1, (what, worst)
    assert (hist[:, 33] == hist[:, :11].sum(1)).all() and (hist[:, 33] == hist[:, 22:33].sum(1)).all()
    return hist, out


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300])
def test_fpfh_small_clouds(n):
    from seggroup_amd import register
    rng = np.random.RandomState(100 + n)
    xyz = (rng.rand(n, 3) * [0.6, 0.5, 0.4]).astype(np.float32)
    nrm = _unit(rng, n)
    if n == 0:
        out, hist = register.fpfh(xyz, nrm, 0.2, lists=(np.zeros(1, np.int64), np.zeros(0, np.int32)), want_spfh=True, device=DEV)
        assert tuple(out.shape) == (0, 33) and tuple(hist.shape) == (0, 34)
        return
    off, idx = Q.lists(xyz, 0.2)
    hist, out = _check_fpfh(xyz, nrm, off, idx, stride=6 if n % 2 else 3, what=n)
    if n >= 63:
        assert hist[:, 33].max() > 1 and out.any()
    # the radius form makes the same lists itself
    again = register.fpfh(xyz, nrm, 0.2, device=DEV).cpu().numpy()
    assert again.tobytes() == out.tobytes()


def test_fpfh_hand_built_lists():
    """an empty row, a row of one, a row of 130 entries (more than two waves' worth of lanes), coincident points (len == 0), a normal
    parallel to d (|v| == 0), and both strides"""
    rng = np.random.RandomState(7)
    n = 140
    xyz = (rng.rand(n, 3) * 0.3).astype(np.float32)
    nrm = _unit(rng, n)
    xyz[1] = xyz[0]                                                       # coincident with 0
    xyz[2] = xyz[0] + np.array([0, 0, 0.125], np.float32)
    nrm[0] = nrm[2] = (0, 0, 1)                                           # parallel to d between 0 and 2
    rows = [[]] * n
    rows[0] = [1, 2] + list(range(3, 131))                                # 130 entries
    rows[1] = [0]                                                         # one entry, and it is the coincident point: no pair
    rows[2] = [0]                                                         # one entry along both normals: no pair
    rows[3] = []                                                          # empty
    for i in range(4, n):
        rows[i] = sorted(rng.choice(n, size=rng.randint(1, 40), replace=False).tolist())
    rows[5] = [4]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([j for r in rows for j in r], np.int32)
    for stride in (3, 6):
        hist, out = _check_fpfh(xyz, nrm, off, idx, stride, what="hand %d" % stride)
        assert hist[0, 33] == 128 and not hist[1].any() and not hist[2].any() and not hist[3].any()
        assert not out[1].any() and not out[3].any()                      # a neighbour at distance 0 weighs nothing; no neighbour at all
        assert hist[5, 33] == 1 and out[0].any() and out[2].any()         # 2 counts no pair of its own and still reads 0's histogram


def test_fpfh_room_is_deterministic_on_any_stream():
    import torch
    from seggroup_amd import register
    d = _described(1)
    xyz = d["xyz"]
    print("room 1500: rows of %d..%d entries, smallest bin margin %.3g, undecided %d" % (np.diff(d["off"]).min(), np.diff(d["off"]).max(),
                                                                                          d["margin"].min(), d["undecided"].sum()))
    hist, out = _check_fpfh(xyz, d["normals"], d["off"], d["idx"], what="room")
    lists = (d["off"], d["idx"])
    again = register.fpfh(xyz, d["normals"], None, lists=lists, want_spfh=True, device=DEV)
    side = register.fpfh(xyz, d["normals"], None, lists=lists, want_spfh=True, device=DEV, stream=torch.cuda.Stream(device=DEV))
    for got in (again, side):
        assert got[0].cpu().numpy().tobytes() == out.tobytes() and got[1].cpu().numpy().tobytes() == hist.tobytes()
    # the device's own normals are the reference's bytes, so the whole description is the same
    from seggroup_amd.oversegment import pointcloud_normals
    nrm = pointcloud_normals(xyz, radius=0.15, device=DEV).cpu().numpy()
    assert nrm.tobytes() == d["normals"].tobytes()


def test_fpfh_refuses_bad_lists():
    from seggroup_amd import register
    rng = np.random.RandomState(9)
    n = 70
    xyz, nrm = rng.rand(n, 3).astype(np.float32), _unit(rng, n)
    off, idx = Q.lists(xyz, 0.3)
    assert off[-1] > n
    for where, value in ((0, n), (int(off[-1]) - 1, -1), (int(off[n // 2]), 1 << 30)):
        bad = idx.copy()
        bad[where] = value
        with pytest.raises(ValueError, match="outside 0..69"):
            register.fpfh(xyz, nrm, None, lists=(off, bad), device=DEV)
    for change in ((0, 1), (n // 2, int(off[-1]) + 5), (n // 2, -3)):
        bad = off.copy()
        bad[change[0]] = change[1]
        with pytest.raises(ValueError, match="do not ascend"):
            register.fpfh(xyz, nrm, None, lists=(bad, idx), device=DEV)
    with pytest.raises(ValueError):
        register.fpfh(xyz, nrm, None, lists=(off[:-1], idx), device=DEV)
    with pytest.raises(ValueError):
        register.fpfh(xyz, nrm[:-1], None, lists=(off, idx), device=DEV)
    good = register.fpfh(xyz, nrm, None, lists=(off, idx), device=DEV)     # and the call after a refusal is unharmed
    assert int(_ulps(good.cpu().numpy(), G.fpfh(xyz, nrm, off, idx)["fpfh"]).max()) <= 1


# ---- sg_feature_nearest ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 33, 64])
def test_feature_nearest_is_the_numpy_statement_bit_for_bit(c):
    import torch
    from seggroup_amd import register
    rng = np.random.RandomState(c)
    for u, n in ((1, 1), (63, 65), (64, 64), (65, 63), (257, 1025)):
        a = (rng.rand(u, c) * 100).astype(np.float32)
        b = (rng.rand(n, c) * 100).astype(np.float32)
        if n > 2:
            b[n // 2:] = b[:n - n // 2]                                   # every row twice: ties go to the lower index
            a[0] = b[n // 2]                                              # and an exact hit, d2 = 0, on a duplicated row
        idx, d2 = register.feature_nearest(a, b, device=DEV)
        assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (u,) and tuple(d2.shape) == (u,)
        want_idx, want_d2 = G.feature_nearest(a, b)
        assert np.array_equal(idx.cpu().numpy(), want_idx), (u, n)
        assert d2.cpu().numpy().tobytes() == want_d2.tobytes(), (u, n)
        if n > 2:
            assert idx[0] == 0 and d2[0] == 0
    idx, d2 = register.feature_nearest(np.zeros((0, c), np.float32), b, device=DEV)
    assert tuple(idx.shape) == (0,)
    with pytest.raises(ValueError):
        register.feature_nearest(a, np.zeros((0, c), np.float32), device=DEV)
    with pytest.raises(ValueError):
        register.feature_nearest(a, b[:, :-1] if c > 1 else np.zeros((3, 2), np.float32), device=DEV)


def test_feature_nearest_on_the_devices_own_descriptors():
    from seggroup_amd import register
    fa, fb = (register.fpfh(_described(seed)["xyz"], _described(seed)["normals"], None, lists=(_described(seed)["off"], _described(seed)["idx"]),
                            device=DEV).cpu().numpy() for seed in (2, 1))
    for a, b in ((fa, fb), (fb, fb)):
        idx, d2 = register.feature_nearest(a, b, device=DEV)
        want_idx, want_d2 = G.feature_nearest(a, b)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and d2.cpu().numpy().tobytes() == want_d2.tobytes()
    assert not d2.cpu().numpy().any()                                     # a cloud against itself: every row finds a row at distance 0


# ---- sg_ransac_count ------------------------------------------------------------------------------------------------------------------------
QUARTER = np.array([[0.0, -1, 0, 3], [1, 0, 0, -2], [0, 0, 1, 1], [0, 0, 0, 1]])    # a quarter turn about z and whole metres: exact in fp32


def _lattice(rng, n):
    """points on a 1/64 m lattice in a 3 m box: A.apply(., QUARTER) moves them without a rounding"""
    return (rng.randint(0, 192, (n, 3)) / 64.0).astype(np.float32)


def _check_ransac(moving, fixed, ci, cj, h, max_dist, seed, triples=None, **kw):
    from seggroup_amd import register
    ref = G.ransac(moving, fixed, ci, cj, h, max_dist, seed, triples=triples, **kw)
    got, survivors = register.ransac_count(moving, fixed, ci, cj, h, max_dist, seed=seed, triples=triples, device=DEV, want_survivors=True, **kw)
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (h,)
    ok = ~ref.undecided
    assert (~ok).sum() <= 1e-3 * h
    assert np.array_equal((got >= 0)[ok], ref.keep[ok])
    if ok.all():
        assert survivors == ref.survivors.size
    sel = ok[ref.survivors] & (got[ref.survivors] >= 0)
    s = ref.survivors[sel]
    assert (ref.count_lo[sel] <= got[s]).all() and (got[s] <= ref.count_hi[sel]).all()
    assert (got[got < 0] == -1).all()
    return got, ref


@pytest.mark.parametrize("c", [3, 64, 65, 1000, 5000])
def test_ransac_count_against_the_reference(c, sg_lib):
    """5,000 correspondences need five LDS tiles of 1,024.  A third of the correspondences are right (an exactly moved copy), the rest
    name a random fixed point; generated triples are the restatement's (the same bytes come back when they are passed in)"""
    from seggroup_amd import register
    rng = np.random.RandomState(c)
    moving = _lattice(rng, max(c, 40))
    fixed = A.apply(moving, QUARTER)
    ci = rng.randint(0, moving.shape[0], c).astype(np.int32)
    cj = np.where(rng.rand(c) < (1.0 if c == 3 else 0.34), ci, rng.randint(0, moving.shape[0], c)).astype(np.int32)
    if c == 3:
        ci = cj = np.array([0, 1, 2], np.int32)
    kept = 0
    for h in (0, 1, 63, 64, 65, 4097):
        seed = 1000 * c + h
        got, ref = _check_ransac(moving, fixed, ci, cj, h, 0.05, seed, min_edge=0.3 if c > 3 else 0.01)
        kept += int((got >= 0).sum())
        if h:
            passed = register.ransac_count(moving, fixed, ci, cj, h, 0.05, seed=seed + 1, triples=G.triples_of(seed, h, c), device=DEV,
                                           min_edge=0.3 if c > 3 else 0.01)
            assert passed.cpu().numpy().tobytes() == got.tobytes(), (c, h)
            assert sg_lib.sg_ransac_set_tuning(1) == 0                # a thread per survivor instead of a wave: the same bytes
            try:
                alone = register.ransac_count(moving, fixed, ci, cj, h, 0.05, seed=seed, device=DEV, min_edge=0.3 if c > 3 else 0.01)
            finally:
                assert sg_lib.sg_ransac_set_tuning(0) == 0
            assert alone.cpu().numpy().tobytes() == got.tobytes(), (c, h)
    assert kept > 0, "no hypothesis survived at any H: the case checks nothing"


def test_ransac_explicit_triples():
    from seggroup_amd import register
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 0], [0, 2, 0], [1, 1, 1], [0.5, 0.25, 2]], np.float32)
    b = A.apply(a, QUARTER)
    b[5] = A.apply(a[2:3], QUARTER)[0]                                    # correspondence 5: its edge to 0 is half as long in the fixed cloud
    ci = cj = np.arange(8, dtype=np.int32)
    triples = np.array([[0, 0, 1],                                        # a repeated index
                        [0, 4, 1],                                        # a zero-length edge: 4 is 0's twin
                        [0, 1, 3],                                        # collinear
                        [0, 1, 5],                                        # an edge ratio of 0.5
                        [0, 1, 2], [2, 6, 7], [7, 1, 6]], np.int32)       # congruent triangles
    got, ref = _check_ransac(a, b, ci, cj, 7, 0.1, 0, triples=triples, min_edge=0.3)
    assert got.tolist() == [-1, -1, -1, -1, 7, 7, 7] and not ref.undecided.any()
    # an exactly moved copy: a congruent triangle counts every correspondence
    rng = np.random.RandomState(4)
    moving = _lattice(rng, 1500)
    fixed = A.apply(moving, QUARTER)
    ci = cj = np.arange(1500, dtype=np.int32)
    far = np.array([[int(np.argmin(moving.sum(1))), int(np.argmax(moving[:, 0] - moving[:, 1])), int(np.argmax(moving[:, 2]))]], np.int32)
    got, _ = _check_ransac(moving, fixed, ci, cj, 1, 0.01, 0, triples=far, min_edge=0.3)
    assert got.tolist() == [1500]
    again = register.ransac_count(moving, fixed, ci, cj, 1, 0.01, triples=far, min_edge=0.3, device=DEV)
    assert again.cpu().numpy().tobytes() == got.tobytes()
    # refused: a correspondence outside its cloud, a triple outside the correspondences
    for which, bad in ((0, 1500), (0, -1), (1, 1500), (1, -7)):
        i, j = ci.copy(), cj.copy()
        (i, j)[which][700 + 100 * which] = bad
        with pytest.raises(ValueError, match="a correspondence outside"):
            register.ransac_count(moving, fixed, i, j, 64, 0.01, device=DEV)
    for bad in (1500, -1):
        with pytest.raises(ValueError, match="a triple names"):
            register.ransac_count(moving, fixed, ci, cj, 2, 0.01, triples=np.array([[0, 1, 2], [3, bad, 5]], np.int32), device=DEV)
    with pytest.raises(ValueError):
        register.ransac_count(moving, fixed, ci[:2], cj[:2], 4, 0.01, device=DEV)
    with pytest.raises(ValueError):
        register.ransac_count(moving, fixed, ci, cj, 4, 0.01, triples=far, device=DEV)


def test_stage_timer_times_the_call_and_the_tuning_knob_leaves_it_on(sg_lib):
    """hip.stage_timer("ransac") around sg_ransac_count: the same bytes as untimed, three finite times above 0, and sg_ransac_set_tuning
    inside the block does not switch the timer off.  A call that is refused for a correspondence outside its cloud ends before its count, so
    a timed one leaves that stage at 0: the count of the call after the knob was turned is above 0 only if it was timed.  After the block
    an untimed call leaves the record as it was."""
    from seggroup_amd import hip, register
    rng = np.random.RandomState(64)
    moving = _lattice(rng, 64)
    fixed = A.apply(moving, QUARTER)
    ci = rng.randint(0, 64, 64).astype(np.int32)
    cj = np.where(rng.rand(64) < 0.34, ci, rng.randint(0, 64, 64)).astype(np.int32)
    outside = cj.copy()
    outside[5] = 64

    def call(cj=cj):
        count, survivors = register.ransac_count(moving, fixed, ci, cj, 4097, 0.05, seed=68097, device=DEV, min_edge=0.3, want_survivors=True)
        return count.cpu().numpy().tobytes(), survivors

    plain = call()
    assert plain[1] > 0, "no hypothesis survived: the count stage has nothing to run"
    with hip.stage_timer("ransac") as t:
        assert t.names == ["gather", "filter", "count"]
        assert call() == plain
        us = t.read()
        assert len(us) == len(t.names) and all(np.isfinite(u) and u > 0.0 for u in us), us
        with pytest.raises(ValueError, match="a correspondence outside"):
            call(outside)
        assert t.read()[t.names.index("count")] == 0.0
        assert sg_lib.sg_ransac_set_tuning(1) == 0
        try:
            assert call() == plain
        finally:
            assert sg_lib.sg_ransac_set_tuning(0) == 0
        last = t.read()
        assert all(np.isfinite(u) and u > 0.0 for u in last), last
    assert call() == plain
    assert t.read() == last


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------
def _corners(moving):
    return A.box_corners(*A.box_of(moving))


@pytest.mark.parametrize("name", sorted(G.FIXTURES))
def test_global_registration_lands_inside_the_basin_and_icp_finishes(name):
    """(a) 150 degrees and 1.5 m, (b) 75 degrees, 3 m and a cloud that lacks the room's far end.  The reference's own coarse pose is 0.059 m
    (a) and 0.120 m (b) from the truth; the gate is ICP's radius, 0.25 m"""
    from seggroup_amd import align, register
    moving, fixed, P = G.fixture(name)
    ref = G.fixture_reference(name)
    c = register.global_registration(moving, fixed, voxel=None, hypotheses=2 ** 20, verify=16, device=DEV, **G.RADII)
    off = A.corner_shift(_corners(moving), c.T, P)
    print(name, "coarse %.4f m (reference %.4f)" % (off, ref["off"]), "h", c.h, "(%d)" % ref["h"], "count", c.count, "(%d)" % ref["count"],
          "verified", c.verified_inliers, "(%d)" % ref["verified_inliers"], "correspondences", c.correspondences, "survivors", c.survivors,
          "(%d)" % ref["survivors"])
    assert off < G.GATE
    assert c.correspondences == ref["correspondences"] and c.moving_points == moving.shape[0] and c.fixed_points == fixed.shape[0]
    assert c.T.dtype == np.float64 and c.T.shape == (4, 4) and np.linalg.det(c.T[:3, :3]) > 0
    assert set(c.scalars()) == set(register.COARSE_SCALARS) and c.hypotheses == 2 ** 20 and c.min_edge == pytest.approx(0.3)
    again = register.global_registration(moving, fixed, voxel=None, device=DEV, **G.RADII)
    assert again.T.tobytes() == c.T.tobytes() and again.scalars() == c.scalars()
    # ICP from the coarse pose ends where ICP from the true pose ends (two fixed points of one data set may differ: 8p.6's rule)
    from_truth = A.icp(moving, fixed, G.GATE, init=P)
    bound = 2 * (A.corner_shift(_corners(moving), from_truth["T"], P) + ref["off"])
    al = align.icp(moving, fixed, G.GATE, init=c.T, device=DEV)
    end = A.corner_shift(_corners(moving), al.T, P)
    try:
        blind = A.corner_shift(_corners(moving), align.icp(moving, fixed, G.GATE, device=DEV).T, P)
    except ValueError as e:                                               # no pose at all is not reaching it either
        assert "max_dist" in str(e)
        blind = np.inf
    print(name, "icp from the coarse pose ends %.4g m from the truth (bound %.4g), without it %.4g m" % (end, bound, blind))
    assert end <= bound
    assert not blind <= bound


def test_global_registration_refusals():
    from seggroup_amd import register
    moving, fixed, _ = G.fixture("a")
    with pytest.raises(ValueError, match="feature_radius"):                # radii below the spacing: no pairs, no descriptors
        register.global_registration(moving, fixed, normal_radius=1e-4, feature_radius=1e-4, max_dist=0.1, hypotheses=1 << 10, device=DEV)
    with pytest.raises(ValueError, match="hypotheses.*min_edge|min_edge.*hypotheses"):
        register.global_registration(moving, fixed, hypotheses=1 << 10, min_edge=50.0, device=DEV, **G.RADII)
    big = np.zeros(((1 << 18) + 1, 3), np.float32)
    big[:, 0] = np.arange(big.shape[0]) * 0.5
    with pytest.raises(ValueError, match="voxel"):
        register.global_registration(big, fixed, hypotheses=1 << 10, device=DEV, **G.RADII)
    with pytest.raises(ValueError, match="max_dist"):
        register.global_registration(moving, fixed, normal_radius=0.15, feature_radius=0.3, device=DEV)


def _tree(root, scene, xyz):
    os.makedirs(os.path.join(root, scene))
    R.write_vertex_only_ply(os.path.join(root, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))


def test_commands_start_from_the_global_pose(tmp_path):
    """the target is a rigidly moved subset of the source under pose (a), 150 degrees and 1.5 m: `transfer --align icp --align-init global`
    returns the source's values at the subset's indices, which plain ICP cannot; `align --global-init` writes the `global` record.  The
    NumPy pipeline on the clouds thinned at 0.08 lands 0.037 m from the pose."""
    from seggroup_amd import align, pseudo_labels, register, transfer
    scene = "scene0071_00"
    P = A.pose(*G.FIXTURES["a"]["pose"])
    src_xyz = A.room(1, 4096).copy()
    sub = 2 * np.arange(2048)
    dst_xyz = A.apply(src_xyz[sub], A.inverse(P))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tree(a, scene, src_xyz)
    _tree(b, scene, dst_xyz)
    rng = np.random.RandomState(8)
    m, s = src_xyz.shape[0], 23
    tables, sov = rng.randint(-1, 40, (14, s)).astype(np.int32), rng.randint(-1, s, m).astype(np.int32)
    src = os.path.join(str(tmp_path), "results", "e", scene, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    common = dict(root=str(tmp_path), device=DEV)
    refused = str(tmp_path / "refused")
    with pytest.raises(ValueError, match="--align-voxel"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, align="icp", align_max_dist=0.25, align_init="global", **common)
    with pytest.raises(ValueError, match="--align icp"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, align_init="global", align_voxel=0.08, **common)
    argv = ["--from-scans", a, "--to-scans", b, "-n", "e", "--out", refused, "--root", str(tmp_path)]
    for extra in (["--align", "icp", "--align-max-dist", "0.25", "--align-init", "global"], ["--align-init", "global", "--align-voxel", "0.08"],
                  ["--align", "icp", "--align-max-dist", "0.25", "--align-voxel", "0.08"]):
        with pytest.raises(SystemExit) as e:
            transfer.main(argv + extra)
        assert e.value.code == 2
    assert not os.path.exists(refused)

    out = str(tmp_path / "global")
    report, missing = transfer.transfer_results(a, b, "e", "epoch_last", out, align="icp", align_max_dist=0.25, align_init="global",
                                                align_voxel=0.08, **common)
    assert missing == {} and list(report) == [scene]
    dst = os.path.join(out, "results", "e", scene, "epoch_last")
    lab = pseudo_labels.load(dst)
    with np.load(os.path.join(dst, scene + transfer.MAP_SUFFIX)) as z:
        npz = {k: z[k] for k in z.files}
    assert np.array_equal(npz["nearest"], sub) and float(npz["d2"].max()) < 1e-10
    assert lab.V == 2048 and np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[sub])
    assert A.corner_shift(_corners(dst_xyz), npz["T"], P) < 2.0 ** -20 * float(np.abs(src_xyz).max())
    rec = report[scene]["align"]
    assert sorted(rec) == sorted(("source", "global") + align.SCALARS) and rec["converged"] == "fixed point" and rec["inliers"] == 2048
    assert sorted(rec["global"]) == sorted(register.COARSE_SCALARS) and rec["global"]["voxel"] == 0.08 and rec["global"]["hypotheses"] == 2 ** 20
    print("transfer: coarse count", rec["global"]["count"], "verified", rec["global"]["verified_inliers"], "of", rec["global"]["moving_points"],
          "searches", rec["iterations"])
    # plain ICP from 150 degrees away does not carry the labels: this is what the coarse stage is for
    plain = str(tmp_path / "plain")
    try:
        transfer.transfer_results(a, b, "e", "epoch_last", plain, align="icp", align_max_dist=0.25, **common)
        with np.load(os.path.join(plain, "results", "e", scene, "epoch_last", scene + transfer.MAP_SUFFIX)) as z:
            assert not np.array_equal(z["nearest"], sub)
    except ValueError as e:
        assert "max_dist" in str(e)

    poses = str(tmp_path / "poses")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.align", "--moving-scans", b, "--fixed-scans", a, "--max-dist", "0.25", "--out", poses, "--workers", "1",
           "--global-init", "--voxel", "0.08"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 scenes aligned, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(os.path.join(poses, scene + align.ALIGN_SUFFIX)))
    assert sorted(doc["global"]) == sorted(register.COARSE_SCALARS + ("T",)) and doc["global"]["voxel"] == 0.08
    assert {k: doc["global"][k] for k in register.COARSE_SCALARS} == rec["global"]
    assert np.array_equal(np.array(doc["T"]), npz["T"]) and doc["converged"] == "fixed point"
    assert A.corner_shift(_corners(dst_xyz), np.array(doc["global"]["T"]), P) < G.GATE
    head = json.load(open(os.path.join(poses, align.REPORT_NAME)))
    assert head["global_init"] == {"voxel": 0.08} and sorted(head["scenes"][scene]["global"]) == sorted(register.COARSE_SCALARS + ("T",))
