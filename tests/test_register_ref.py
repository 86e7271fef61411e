"""Global registration without a GPU: the NumPy restatement (tests/register_ref.py) against hand-computed splitmix64
values, sg_triangle_pose -- host code, the function the RANSAC kernel runs -- against the NumPy frames, the reference pipeline alone on
the acceptance fixtures, and what the library and the Python layer refuse before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import align_ref as A
import register_ref as G
from test_align_ref import ORTHO_BOUND

# Agreement of sg_triangle_pose with the NumPy frames, 8p.6's method: measured over pose_cases() on the CPU, the largest entry difference
# of the 3x4 transforms is POSE_MEASURED, and the gate is 16 times that.  The measurement is 0: both sides run the same IEEE double
# operations (+, -, *, /, sqrt, each correctly rounded, nothing contracted) in the same order, so the gate is the same bytes.
POSE_MEASURED = 0.0
POSE_BOUND = 16 * POSE_MEASURED


def test_splitmix64_restatement_against_hand_computed_values():
    # the published test vector of splitmix64 seeded with 0: its first three outputs (state = k * golden, k = 1, 2, 3)
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    z = np.array([(k * G.GOLDEN) % 2 ** 64 for k in (1, 2, 3)], np.uint64)
    assert [int(v) for v in G.splitmix64(z)] == want
    # triple 0 of seed 0 over C = 1000 correspondences is ((z >> 32) * 1000) >> 32 of those three
    assert G.triples_of(0, 1, 1000).tolist() == [[((w >> 32) * 1000) >> 32 for w in want]] == [[883, 431, 26]]
    # a seed shifts the state: seed = golden, h = 0 gives the outputs of states 2, 3, 4 x golden
    assert G.triples_of(G.GOLDEN, 1, 1 << 18)[0, :2].tolist() == [((w >> 32) << 18) >> 32 for w in want[1:]]
    from seggroup_amd import register
    for seed, h, c in ((0, 0, 1000), (7, 12345, 3000), (2 ** 64 - 1, (1 << 24) - 1, 1 << 18)):
        assert register.splitmix_triple(seed, h, c) == G.triples_of(seed, h + 1, c)[h].tolist()


def pose_cases():
    """name -> (a, b) float64 [3,3]: random triangles and their images under a random pose (exact to rounding), the same with the corners
    in mirrored order, and at a 1,000 m offset"""
    rng = np.random.RandomState(5)
    out = {}
    for i in range(40):
        a = rng.randn(3, 3) * [3, 2, 1]
        P = A.pose(rng.uniform(5, 175), rng.uniform(0, 2), axis=rng.randn(3), direction=rng.randn(3))
        kind = ("random", "rotated", "mirrored", "far")[i % 4]
        if kind == "far":
            a = a + np.array([1000.0, -1000.0, 500.0])
        b = a @ P[:3, :3].T + P[:3, 3]
        if kind == "mirrored":
            a, b = a[::-1].copy(), b[::-1].copy()
        if kind == "random":
            b = rng.randn(3, 3)                                          # not congruent: the frames still give a proper rotation
        out["%s_%d" % (kind, i)] = (a, b, P if kind != "random" else None)
    return out


def test_triangle_pose_is_a_rotation_and_agrees_with_the_numpy_frames(sg_lib):
    from seggroup_amd import hip, register
    worst = 0.0
    for name, (a, b, P) in pose_cases().items():
        T = register.triangle_pose(a, b)
        R = T[:3, :3]
        assert np.linalg.det(R) > 0, name
        assert np.abs(R.T @ R - np.eye(3)).max() <= ORTHO_BOUND, name
        assert T[3].tolist() == [0, 0, 0, 1]
        diff = float(np.abs(T[:3] - G.triangle_pose(a, b)).max())
        worst = max(worst, diff)
        assert diff <= POSE_BOUND, (name, diff)
        if P is not None:                                                # a congruent pair: the pose is the one that made it
            lever = 1.0 + np.abs(a).max()
            assert np.abs(T - P).max() <= 1e-12 * lever * lever, name
    print("largest |sg_triangle_pose - numpy frames| %.3e; bound %.3e" % (worst, POSE_BOUND))
    line = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for a, b in ((line, tri), (tri, line), (tri[[0, 0, 2]], tri)):
        with pytest.raises(hip.SgError, match="degenerate") as e:
            register.triangle_pose(a, b)
        assert e.value.code == hip.SG_EUNSUP
    bad = tri.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError):
        register.triangle_pose(bad, tri)
    with pytest.raises(ValueError):
        register.triangle_pose(tri[:2], tri)


def test_reference_descriptor_edge_cases():
    """the statement itself on a hand-built cloud: skipped pairs, an empty row, the plane's bin centres"""
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 2], [5, 5, 5]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (6, 1))
    off = np.array([0, 4, 5, 6, 6, 6, 6], np.int64)
    idx = np.array([1, 2, 3, 4, 0, 0], np.int32)                        # row 0: two plane pairs, a coincident point, a pair along the normal
    r = G.fpfh(xyz, nrm, off, idx)
    assert r["spfh"][0, G.HIST] == 2 and r["spfh"][0, [5, 16, 27]].tolist() == [2, 2, 2]        # (0, 0, 0) sits at the bin centres
    assert r["spfh"][3:].sum() == 0 and not r["fpfh"][3:].any()
    assert r["fpfh"][0, [5, 16, 27]].tolist() == [100.0, 100.0, 100.0] and r["fpfh"][0].sum() == 300.0
    assert r["margin"][0] == 0.5 and np.isinf(r["margin"][5]) and not r["undecided"].any()


@pytest.mark.parametrize("name", sorted(G.FIXTURES))
def test_reference_pipeline_lands_inside_half_the_gate(name):
    """the fixtures must be ones the reference itself solves with margin: its coarse pose is below half the gate (0.059 m for (a), 0.120 m
    for (b) -- DESIGN.md 8r), few correspondences are right, and the fences leave nearly everything compared"""
    r = G.fixture_reference(name)
    moving, fixed, P = G.fixture(name)
    right = int((np.sqrt(((A.apply(moving, P)[r["ci"]].astype(np.float64) - fixed[r["cj"]]) ** 2).sum(1)) < G.RADII["max_dist"]).sum())
    print(name, "coarse %.4f m" % r["off"], "h", r["h"], "count", r["count"], "verified", r["verified_inliers"], "of", moving.shape[0],
          "correspondences", r["correspondences"], "right", right, "survivors", r["survivors"], "undecided", int(r["ransac"].undecided.sum()))
    assert r["off"] < 0.5 * G.GATE
    assert r["ransac"].undecided.sum() <= 1e-3 * 2 ** 20
    assert r["survivors"] < 0.01 * 2 ** 20                               # the pre-rejection leaves well under 1 %
    assert right < 0.1 * r["correspondences"]                            # and RANSAC works from a few per cent of inliers


def test_fences_leave_the_fixed_cloud_compared():
    d = G.describe(G.fixed_cloud(), G.RADII["normal_radius"], G.RADII["feature_radius"])
    print("smallest bin margin %.3g, undecided %d of %d" % (d["margin"].min(), d["undecided"].sum(), d["undecided"].size))
    assert d["undecided"].mean() <= 0.01


def test_library_refuses_before_a_device_is_touched(sg_lib):
    from seggroup_amd import hip
    one = C.c_void_p(16)                                                 # never dereferenced: every call below is refused first
    assert sg_lib.sg_fpfh(None, 3, 0, None, None, None, None, None, None, 0, None) == hip.SG_OK          # N = 0 touches nothing
    assert sg_lib.sg_fpfh(one, 2, 10, one, one, one, one, one, one, 1 << 20, None) == hip.SG_EINVAL
    assert sg_lib.sg_fpfh(one, 3, -1, one, one, one, one, one, one, 1 << 20, None) == hip.SG_EINVAL
    assert sg_lib.sg_fpfh(one, 3, (1 << 24) + 1, one, one, one, one, one, one, 1 << 20, None) == hip.SG_EUNSUP
    assert sg_lib.sg_fpfh(one, 3, 10, one, one, one, one, one, one, 0, None) == hip.SG_EINVAL           # no workspace
    assert sg_lib.sg_fpfh_ws_bytes(10) > 0 and sg_lib.sg_fpfh_ws_bytes((1 << 24) + 1) == 0
    assert sg_lib.sg_feature_nearest(None, 0, one, 5, 33, None, None, None) == hip.SG_OK                 # U = 0
    assert sg_lib.sg_feature_nearest(one, 5, one, 0, 33, one, one, None) == hip.SG_EINVAL                # N = 0
    for c in (0, 65):
        assert sg_lib.sg_feature_nearest(one, 5, one, 5, c, one, one, None) == hip.SG_EINVAL
    for u, n in (((1 << 18) + 1, 5), (5, (1 << 18) + 1)):
        assert sg_lib.sg_feature_nearest(one, u, one, n, 33, one, one, None) == hip.SG_EUNSUP
        assert b"thin" in sg_lib.sg_last_error()
    args = lambda c, h, md=0.1, sim=0.9, me=0.3, ws=1 << 30: (one, 3, 10, one, 3, 10, one, one, c, h, 0, None, md, sim, me, one, None, one, ws, None)
    assert sg_lib.sg_ransac_count(*args(3, 0)) == hip.SG_OK                                              # H = 0
    assert sg_lib.sg_ransac_count(*args(2, 10)) == hip.SG_EINVAL
    assert sg_lib.sg_ransac_count(*args((1 << 18) + 1, 10)) == hip.SG_EUNSUP
    assert sg_lib.sg_ransac_count(*args(10, (1 << 24) + 1)) == hip.SG_EUNSUP
    for kw in (dict(md=0.0), dict(md=np.inf), dict(me=0.0), dict(sim=0.0), dict(sim=1.5), dict(ws=16)):
        assert sg_lib.sg_ransac_count(*args(10, 10, **kw)) == hip.SG_EINVAL, kw
    assert sg_lib.sg_ransac_ws_bytes(2, 10) == 0 and sg_lib.sg_ransac_ws_bytes(10, (1 << 24) + 1) == 0
    assert sg_lib.sg_ransac_ws_bytes(1 << 18, 1 << 24) >= 4 * (1 << 24) + 24 * (1 << 18)
    assert sg_lib.sg_ransac_set_tuning(7) == hip.SG_EINVAL and sg_lib.sg_ransac_set_tuning(0) == hip.SG_OK
    assert [sg_lib.sg_ransac_stage_name(i) for i in range(4)] == [b"gather", b"filter", b"count", None]


def test_python_refusals(tmp_path):
    from seggroup_amd import align, register, transfer
    with pytest.raises(ValueError, match="normal_radius, feature_radius and max_dist"):
        register.check_parameters(None, 0.1, None, 0.1, 100, 16)
    with pytest.raises(ValueError, match="voxel"):
        register.check_parameters(0.0, None, None, None, 100, 16)
    with pytest.raises(ValueError, match="hypotheses"):
        register.check_parameters(0.05, None, None, None, 0, 16)
    with pytest.raises(ValueError, match="verify"):
        register.check_parameters(0.05, None, None, None, 100, 0)
    got = register.check_parameters(0.04, None, 0.3, None, 100, 16)
    assert got == (0.08, 0.3, 1.5 * 0.04)
    # the commands: refused before anything runs
    with pytest.raises(ValueError, match="--voxel"):
        align.check_global(True, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="--init"):
        align.check_global(True, 0.05, str(tmp_path), None, None, None, None)
    for extra in (dict(hypotheses=10), dict(seed=1), dict(verify=4), dict(mutual=True), dict(voxel=0.05)):
        kw = dict(dict(voxel=None, init_dir=None, hypotheses=None, seed=None, verify=None, mutual=None), **extra)
        with pytest.raises(ValueError, match="--global-init"):
            align.check_global(False, kw["voxel"], kw["init_dir"], kw["hypotheses"], kw["seed"], kw["verify"], kw["mutual"])
    align.check_global(True, 0.05, None, 1 << 10, 3, 4, True)
    align.check_global(False, None, str(tmp_path), None, None, None, None)
    argv = ["--moving-scans", str(tmp_path), "--fixed-scans", str(tmp_path), "--max-dist", "0.25", "--out", str(tmp_path / "o")]
    for extra in (["--global-init"], ["--global-init", "--voxel", "0.05", "--init", str(tmp_path)], ["--voxel", "0.05"], ["--mutual"]):
        with pytest.raises(SystemExit) as e:
            align.main(argv + extra)
        assert e.value.code == 2
    with pytest.raises(ValueError, match="--align icp"):
        transfer.check_align(None, None, "grid", None, "global", 0.05)
    with pytest.raises(ValueError, match="--align icp"):
        transfer.check_align(str(tmp_path), None, "grid", None, "global", 0.05)
    with pytest.raises(ValueError, match="--align-voxel"):
        transfer.check_align("icp", 0.25, "grid", None, "global", None)
    with pytest.raises(ValueError, match="--align-init global"):
        transfer.check_align("icp", 0.25, "grid", None, None, 0.05)
    with pytest.raises(ValueError, match="--align-init"):
        transfer.check_align("icp", 0.25, "grid", None, "local", 0.05)
    transfer.check_align("icp", 0.25, "grid", None, "global", 0.05)
    assert not (tmp_path / "o").exists()
