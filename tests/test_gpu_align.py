"""Rigid alignment of two clouds on the GPU (seggroup_amd/align.py): sg_rigid_apply bit-equal to the element-wise NumPy
statement; sg_align_moments exact in n, within the summation-order bound of np.sum everywhere else, and the same bytes on every call;
the ICP's fixed point checked against tests/align_ref.py as integers; transfer --align carries labels between two poses of a room."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import pcseg_ref as R
from conftest import ROOT
from test_align_ref import SOLVE_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 256                                                                   # the workgroup size of both kernels
PAIRS = 4 * B                                                             # pairs a workgroup folds into one partial
U_LIST = (0, 1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7)
# the moments also at the edges of a workgroup's 1,024 pairs, and with more partials (258) than a wave and than the folding workgroup
U_MOMENTS = U_LIST + (PAIRS - 1, PAIRS, PAIRS + 1, 3 * PAIRS + 7, 257 * PAIRS + 3)
FAR = np.array([1000.0, -1000.0, 500.0])


def _rows(xyz, stride, rng):
    """xyz as the first columns of [U, stride] rows (stride 6: xyzrgb)"""
    if stride == 3:
        return np.ascontiguousarray(xyz)
    return np.ascontiguousarray(np.concatenate([xyz, rng.rand(xyz.shape[0], stride - 3).astype(np.float32) * 255], 1))


def test_rigid_apply_is_the_numpy_statement_bit_for_bit(sg_lib):
    import torch
    from seggroup_amd import align, hip
    rng = np.random.RandomState(1)
    far = A.pose(37.0, 0.0)
    far[:3, 3] = FAR                                                      # a rotation with a 1,000 m translation
    general = np.vstack([rng.randn(3, 4) * [1, 10, 0.1, 3], [0, 0, 0, 1]])   # any finite matrix, not only a rotation
    for T in (far, A.pose(10.0, 0.15), general):
        for u in U_LIST:
            xyz = (rng.randn(u, 3) * [3, 2, 1]).astype(np.float32)
            for stride in (3, 6):
                got = align.apply(_rows(xyz, stride, rng), T, device=DEV)
                assert got.dtype == torch.float32 and tuple(got.shape) == (u, 3) and got.is_cuda
                assert got.cpu().numpy().tobytes() == A.apply(xyz, T).tobytes(), (u, stride)
    x = torch.zeros((8, 3), device=DEV)
    out = torch.full((8, 3), 7.0, device=DEV)
    bad = np.ascontiguousarray(far[:3].copy())
    bad[1, 2] = np.nan
    assert sg_lib.sg_rigid_apply(x.data_ptr(), 3, 8, bad.ctypes.data, out.data_ptr(), None) == hip.SG_EINVAL
    assert sg_lib.sg_rigid_apply(x.data_ptr(), 2, 8, far.ctypes.data, out.data_ptr(), None) == hip.SG_EINVAL
    assert sg_lib.sg_rigid_apply(None, 3, 0, far.ctypes.data, None, None) == hip.SG_OK      # U = 0 touches nothing
    assert sg_lib.sg_rigid_apply(None, 3, (1 << 27) + 1, far.ctypes.data, None, None) == hip.SG_EUNSUP
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        align.apply(np.zeros((4, 3), np.float32), bad, device=DEV)


@pytest.mark.parametrize("offset", [0.0, 1.0], ids=["origin", "1000m"])
def test_moments_are_exact_in_n_bounded_in_the_sums_and_deterministic(offset):
    import torch
    from seggroup_amd import align
    rng = np.random.RandomState(2)
    side = torch.cuda.Stream(device=DEV)
    n_y = 777
    ox, oy = offset * FAR, offset * FAR[::-1]
    for u in U_MOMENTS:
        stride = 6 if u % 2 else 3
        x = ((rng.randn(u, 3) * [3, 2, 1]) + ox).astype(np.float32)
        y = ((rng.randn(n_y, 3) * [3, 2, 1]) + oy).astype(np.float32)
        idx = rng.randint(0, n_y, u).astype(np.int64)
        d2 = (rng.rand(u) + 1e-3).astype(np.float32)                      # all above 0: max_dist = 0 leaves no inlier
        d2[rng.rand(u) < 0.02] = np.nan                                   # never an inlier, whatever the radius
        xr, yr = _rows(x, stride, rng), _rows(y, 9 - stride, rng)
        for max_dist in (np.inf, 0.0, np.sqrt(0.5)):                      # all in, all out, a mix that cuts inside every wave
            want, mag = A.moments(x, y, idx, d2, max_dist, ox, oy)
            got = align.moments(xr, yr, idx, d2, max_dist, ox, oy, device=DEV)
            assert got.dtype == np.float64 and got.shape == (17,)
            assert got[0] == want[0] == (0 if max_dist == 0.0 else (d2 <= A.max_d2_of(max_dist)).sum()), (u, max_dist)
            if max_dist == 0.0:
                assert got.tobytes() == np.zeros(17).tobytes(), u         # sums exactly 0
            bound = u * 2.0 ** -52 * mag                                  # two summation orders of the same, exactly equal terms
            assert (np.abs(got - want) <= bound).all(), (u, max_dist, np.abs(got - want) / np.maximum(bound, 1e-300))
            again = align.moments(xr, yr, idx, d2, max_dist, ox, oy, device=DEV)
            assert again.tobytes() == got.tobytes(), (u, max_dist)
        other = align.moments(xr, yr, idx, d2, np.sqrt(0.5), ox, oy, device=DEV, stream=side)      # the stream cannot change a byte
        assert other.tobytes() == got.tobytes(), u


def test_moments_refuse_an_index_outside_the_candidates():
    from seggroup_amd import align
    rng = np.random.RandomState(3)
    u, n_y = 3 * B + 7, 50
    x, y = rng.randn(u, 3).astype(np.float32), rng.randn(n_y, 3).astype(np.float32)
    d2 = rng.rand(u).astype(np.float32)
    for where, value in ((0, n_y), (u - 1, -1), (B + 3, 1 << 40)):
        idx = rng.randint(0, n_y, u).astype(np.int64)
        idx[where] = value
        d2[where] = 2.0                                                   # outside the radius: refused all the same
        with pytest.raises(ValueError, match="outside 0..49"):
            align.moments(x, y, idx, d2, 1.0, device=DEV)
    with pytest.raises(ValueError):
        align.moments(x, y, idx[:-1], d2, 1.0, device=DEV)


def _corners(moving):
    return A.box_corners(*A.box_of(moving))


@pytest.mark.parametrize("name", sorted(A.POSES))
def test_icp_exact_case_ends_at_the_true_pose(name):
    """the moving cloud is every second fixed point under the inverse of a pose: the fixed point is the pose itself.  The NumPy reference
    reaches it in 8 (3 degrees, 4 cm) and 17 (10 degrees, 15 cm) searches, 3e-9 m and 1e-9 m from the true pose"""
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    P = A.pose(*A.POSES[name])
    moving = A.apply(fixed[::2], A.inverse(P))
    al = align.icp(moving, fixed, 0.25, device=DEV)
    off = A.corner_shift(_corners(moving), al.T, P)
    print(name, "searches", al.iterations, "converged", al.converged, "inliers", al.inliers, "rms %.3g -> %.3g" % (al.rms_before, al.rms_after),
          "corner displacement %.3g" % off)
    assert al.converged == "fixed point"
    assert np.array_equal(al.idx.cpu().numpy(), 2 * np.arange(2048))
    assert off < 2.0 ** -20 * float(np.abs(fixed).max())
    assert al.inliers == 2048 and bool(al.inlier.all()) and al.iterations <= 50
    assert al.rms_after < 1e-6 < al.rms_before
    assert abs(al.rotation_deg - A.POSES[name][0]) < 1e-3 and al.translation == [float(v) for v in al.T[:3, 3]]


@pytest.mark.parametrize("name", sorted(A.POSES))
def test_icp_resampled_case_ends_at_a_fixed_point_of_the_reference(name):
    """another sampling of the same room: no pose has zero residual.  Trajectories are not compared; the fixed point is checked itself.
    The NumPy reference converges to a fixed point in 28 (3 degrees, 4 cm) and 39 (10 degrees, 15 cm) searches with all 3,000 points
    inliers, 11.5 mm and 12.1 mm from the true pose (rms 0.0404)."""
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    P = A.pose(*A.POSES[name])
    moving = A.apply(A.room(2, 3000), A.inverse(P))
    al = align.icp(moving, fixed, 0.25, device=DEV)
    assert al.converged == "fixed point"
    moved = A.apply(moving, al.T)
    assert align.apply(moving, al.T, device=DEV).cpu().numpy().tobytes() == moved.tobytes()
    idx, d2 = A.search(moved, fixed)
    assert np.array_equal(al.idx.cpu().numpy(), idx) and al.d2.cpu().numpy().tobytes() == d2.tobytes()
    inlier = d2 <= A.max_d2_of(0.25)
    assert np.array_equal(al.inlier.cpu().numpy(), inlier) and al.inliers == int(inlier.sum())
    om, of = (0.5 * (lo + hi) for lo, hi in (A.box_of(moving), A.box_of(fixed)))
    m, _ = A.moments(moving, fixed, idx, d2, 0.25, om, of)
    gap = float(np.abs(al.T - A.solve(m, om, of)).max())
    ref = A.icp(moving, fixed, 0.25)
    off, ref_off = A.corner_shift(_corners(moving), al.T, P), A.corner_shift(_corners(moving), ref["T"], P)
    print(name, "searches", al.iterations, "(reference %d)" % ref["iterations"], "inliers", al.inliers, "rms %.4g -> %.4g" % (al.rms_before, al.rms_after),
          "|T - kabsch| %.3g" % gap, "displacement from the true pose %.6g (reference %.6g)" % (off, ref_off),
          "same fixed point" if np.array_equal(ref["idx"], idx) else "another fixed point")
    assert gap <= SOLVE_BOUND
    assert ref["converged"] == "fixed point"
    assert off <= 2 * ref_off
    assert al.rms_after == pytest.approx(np.sqrt(m[16] / m[0]), rel=1e-12)


def test_icp_refusals():
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    moving = A.apply(fixed[::2], A.inverse(A.pose(*A.POSES["10deg_15cm"])))
    with pytest.raises(ValueError, match="max_dist"):
        align.icp(moving, fixed, 1e-6, device=DEV)                        # no inliers
    line = np.zeros((50, 3), np.float32)
    line[:, 0] = np.linspace(-1, 1, 50)
    with pytest.raises(ValueError, match="max_dist"):
        align.icp(line, line, 0.25, device=DEV)                           # pairs on a line: the rotation about it is free
    with pytest.raises(ValueError):
        align.icp(moving, fixed, 0.25, index="brute", device=DEV)
    with pytest.raises(ValueError):
        align.icp(moving, fixed, 0.25, init=np.eye(3), device=DEV)
    al = align.icp(moving, fixed, 0.25, max_iter=2, device=DEV)
    assert al.converged is False and al.iterations == 2


def _tree(root, scene, xyz):
    os.makedirs(os.path.join(root, scene))
    R.write_vertex_only_ply(os.path.join(root, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))


def test_transfer_align_carries_labels_between_two_poses(tmp_path):
    """the target is a rigidly moved subset of the source (10 degrees, 15 cm): with --align every transferred value is the source's at the
    subset's indices; without it some vertices take another vertex's labels, which is why the option exists"""
    from seggroup_amd import align, pseudo_labels, transfer
    scene = "scene0071_00"
    src_xyz = A.room(1, 4096).copy()
    sub = 2 * np.arange(2048)
    dst_xyz = A.apply(src_xyz[sub], A.inverse(A.pose(*A.POSES["10deg_15cm"])))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tree(a, scene, src_xyz)
    _tree(b, scene, dst_xyz)
    rng = np.random.RandomState(8)
    m, s = src_xyz.shape[0], 23
    tables, sov = rng.randint(-1, 40, (14, s)).astype(np.int32), rng.randint(-1, s, m).astype(np.int32)
    loose = rng.randint(0, 40, m).astype(np.int32)
    src = os.path.join(str(tmp_path), "results", "e", scene, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    np.save(os.path.join(src, "final.sem.npy"), loose)
    common = dict(root=str(tmp_path), device=DEV)

    def outputs(root2):
        dst = os.path.join(root2, "results", "e", scene, "epoch_last")
        with np.load(os.path.join(dst, scene + transfer.MAP_SUFFIX)) as z:
            npz = {k: z[k] for k in z.files}
        return pseudo_labels.load(dst), np.load(os.path.join(dst, "final.sem.npy")), npz, dst

    # refused before anything runs
    refused = str(tmp_path / "refused")
    with pytest.raises(ValueError, match="--index grid"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, index="brute", align="icp", align_max_dist=0.25, **common)
    with pytest.raises(ValueError, match="--align icp"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, align_max_dist=0.25, **common)
    with pytest.raises(ValueError, match="--align-max-dist"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, align="icp", **common)
    argv = ["--from-scans", a, "--to-scans", b, "-n", "e", "--out", refused, "--root", str(tmp_path)]
    for extra in (["--align", "icp", "--align-max-dist", "0.25", "--index", "brute"], ["--align-max-dist", "0.25"], ["--align", "icp"],
                  ["--align", a, "--align-max-dist", "0.25"]):
        with pytest.raises(SystemExit) as e:
            transfer.main(argv + extra)
        assert e.value.code == 2
    assert not os.path.exists(refused)

    plain = str(tmp_path / "plain")
    report, _ = transfer.transfer_results(a, b, "e", "epoch_last", plain, **common)
    lab, sem, npz, _ = outputs(plain)
    assert sorted(npz) == ["d2", "nearest"] and "align" not in report[scene]
    assert (npz["nearest"] != sub).any() and not np.array_equal(lab.seg_of_vertex, sov[sub]) and not np.array_equal(sem, loose[sub])

    icp_root = str(tmp_path / "icp")
    report, missing = transfer.transfer_results(a, b, "e", "epoch_last", icp_root, align="icp", align_max_dist=0.25, **common)
    assert missing == {} and list(report) == [scene]
    lab, sem, npz, icp_dst = outputs(icp_root)
    assert lab.V == 2048 and np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[sub]) and np.array_equal(sem, loose[sub])
    assert sorted(npz) == ["T", "d2", "nearest"] and npz["T"].dtype == np.float64 and npz["T"].shape == (4, 4)
    assert np.array_equal(npz["nearest"], sub) and float(npz["d2"].max()) < 1e-10
    assert A.corner_shift(_corners(dst_xyz), npz["T"], A.pose(*A.POSES["10deg_15cm"])) < 2.0 ** -20 * float(np.abs(src_xyz).max())
    e = report[scene]
    assert e == json.load(open(os.path.join(icp_root, transfer.REPORT_NAME)))["scenes"][scene]
    assert sorted(e["align"]) == sorted(("source",) + align.SCALARS) and e["align"]["source"] == "icp" and e["align"]["converged"] == "fixed point"
    assert e["align"]["inliers"] == 2048 and e["max_distance"] < 1e-5 and e["farther_than"] == {"0.05": 0, "0.1": 0, "0.5": 0}

    # the command writes what --align DIR reads; the same files come out
    poses = str(tmp_path / "poses")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.align", "--moving-scans", b, "--fixed-scans", a, "--max-dist", "0.25", "--out", poses, "--workers", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 scenes aligned, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(os.path.join(poses, scene + align.ALIGN_SUFFIX)))
    assert np.array_equal(np.array(doc["T"]), npz["T"]) and (doc["moving_V"], doc["fixed_V"], doc["max_dist"]) == (2048, 4096, 0.25)
    assert {k: doc[k] for k in align.SCALARS} == {k: e["align"][k] for k in align.SCALARS}
    assert json.load(open(os.path.join(poses, align.REPORT_NAME)))["scenes"][scene]["converged"] == "fixed point"
    dir_root = str(tmp_path / "dir")
    report2, _ = transfer.transfer_results(a, b, "e", "epoch_last", dir_root, align=poses, **common)
    _, _, npz2, dir_dst = outputs(dir_root)
    for f in (pseudo_labels.SGL_NAME, "final.sem.npy"):
        assert open(os.path.join(dir_dst, f), "rb").read() == open(os.path.join(icp_dst, f), "rb").read(), f
    assert sorted(npz2) == sorted(npz) and all(npz2[k].tobytes() == npz[k].tobytes() for k in npz)
    assert report2[scene]["align"] == dict(e["align"], source=os.path.join(poses, scene + align.ALIGN_SUFFIX))
    # --init takes the pose where it ended: the first search finds the same pairs, the second repeats them
    al = align.icp(dst_xyz, src_xyz, 0.25, init=align.read_align(os.path.join(poses, scene + align.ALIGN_SUFFIX))["T"], device=DEV)
    assert al.converged in ("fixed point", "min_delta") and al.iterations <= 2 and np.array_equal(al.idx.cpu().numpy(), sub)

    vote_root = str(tmp_path / "vote")
    report3, _ = transfer.transfer_results(a, b, "e", "epoch_last", vote_root, align="icp", align_max_dist=0.25, vote_k=5, **common)
    _, _, npz3, _ = outputs(vote_root)
    assert sorted(npz3) == ["T", "d2", "nearest", "rep", "tied", "votes"] and np.array_equal(npz3["nearest"], sub)
    assert npz3["T"].tobytes() == npz["T"].tobytes() and report3[scene]["vote"] == 5 and report3[scene]["align"] == e["align"]
