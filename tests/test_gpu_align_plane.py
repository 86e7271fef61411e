"""Point-to-plane ICP on the GPU (seggroup_amd/align.py metric="plane"): sg_align_plane_moments exact in its two counts,
within the summation-order bound of np.sum everywhere else and the same bytes on every call; the loop against tests/align_plane_ref.py
and against metric="point" on the same input; transfer --align-metric plane and python -m seggroup_amd.align --metric plane."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_plane_ref as P
import align_ref as A
import pcseg_ref as R
from conftest import ROOT
from test_align_plane_ref import SOLVE_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 256                                                                   # the workgroup size of both kernels
PAIRS = 4 * B                                                             # pairs a workgroup folds into one partial row
# the edges of a wave, of a workgroup and of its 1,024 pairs, and 258 partial rows: more than a wave and more than the folding workgroup
U_MOMENTS = (0, 1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7, PAIRS - 1, PAIRS, PAIRS + 1, 3 * PAIRS + 7, 257 * PAIRS + 3)
FAR = np.array([1000.0, -1000.0, 500.0])
POSE = "10deg_15cm"


def _rows(xyz, stride, rng):
    """xyz as the first columns of [U, stride] rows"""
    if stride == 3:
        return np.ascontiguousarray(xyz)
    return np.ascontiguousarray(np.concatenate([xyz, rng.rand(xyz.shape[0], stride - 3).astype(np.float32) * 255], 1))


def _test_normals(rng, n):
    """unit normals, 3 % of them unusable: zero, NaN in one component, length 0.4 and length 2.5"""
    nrm = rng.randn(n, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(np.float32)
    bad = np.flatnonzero(rng.rand(n) < 0.03)
    for j, i in enumerate(bad):
        if j % 4 == 0:
            nrm[i] = 0.0
        elif j % 4 == 1:
            nrm[i, j % 3] = np.nan
        else:
            nrm[i] *= np.float32(0.4 if j % 4 == 2 else 2.5)
    return nrm, bad.size


def _corners(moving):
    return A.box_corners(*A.box_of(moving))


@pytest.mark.parametrize("pose", ["identity", POSE])
@pytest.mark.parametrize("offset", [0.0, 1.0], ids=["origin", "1000m"])
def test_plane_moments_are_exact_in_the_counts_bounded_in_the_sums_and_deterministic(offset, pose):
    import torch
    from seggroup_amd import align
    rng = np.random.RandomState(12)
    side = torch.cuda.Stream(device=DEV)
    n_y = 777
    o = offset * FAR
    T = np.eye(4) if pose == "identity" else A.pose(*A.POSES[pose])
    for u in U_MOMENTS:
        stride = 6 if u % 2 else 3
        x = ((rng.randn(u, 3) * [3, 2, 1]) + o).astype(np.float32)
        y = ((rng.randn(n_y, 3) * [3, 2, 1]) + o).astype(np.float32)
        nrm, n_bad = _test_normals(rng, n_y)
        assert n_bad >= 4
        idx = rng.randint(0, n_y, u).astype(np.int64)
        d2 = (rng.rand(u) + 1e-3).astype(np.float32)                      # all above 0: max_dist = 0 leaves no candidate
        d2[rng.rand(u) < 0.02] = np.nan                                   # never a candidate, whatever the radius
        xr, yr, nr = _rows(x, stride, rng), _rows(y, 9 - stride, rng), _rows(nrm, stride, rng)
        for max_dist in (np.inf, 0.0, np.sqrt(0.5)):                      # all in, all out, a mix that cuts inside every wave
            want, mag = P.moments(x, T, y, nrm, idx, d2, max_dist, o)
            got = align.plane_moments(xr, T, yr, nr, idx, d2, max_dist, o, device=DEV)
            assert got.dtype == np.float64 and got.shape == (31,)
            with np.errstate(invalid="ignore"):
                cand = d2 <= A.max_d2_of(max_dist)
            ok = P.usable_normal(nrm[idx[cand]].astype(np.float64))
            assert got[0] == want[0] == ok.sum() and got[1] == want[1] == (~ok).sum(), (u, max_dist)
            if max_dist == 0.0:
                assert got.tobytes() == np.zeros(31).tobytes(), u         # sums exactly 0
            bound = u * 2.0 ** -52 * mag                                  # two summation orders of the same, exactly equal terms
            assert (np.abs(got - want) <= bound).all(), (u, max_dist, np.abs(got - want) / np.maximum(bound, 1e-300))
            again = align.plane_moments(xr, T, yr, nr, idx, d2, max_dist, o, device=DEV)
            assert again.tobytes() == got.tobytes(), (u, max_dist)
        other = align.plane_moments(xr, T, yr, nr, idx, d2, np.sqrt(0.5), o, device=DEV, stream=side)     # the stream cannot change a byte
        assert other.tobytes() == got.tobytes(), u
        if u >= B:
            assert got[1] > 0 and got[0] > got[1], u                      # the unusable normals were met


def test_plane_moments_refuse_an_index_outside_the_candidates(sg_lib):
    import torch
    from seggroup_amd import align, hip
    rng = np.random.RandomState(13)
    u, n_y = 3 * B + 7, 50
    x, y = rng.randn(u, 3).astype(np.float32), rng.randn(n_y, 3).astype(np.float32)
    nrm, _ = _test_normals(rng, n_y)
    d2 = rng.rand(u).astype(np.float32)
    for where, value, dist in ((0, n_y, 0.5), (u - 1, -1, 2.0), (B + 3, 1 << 40, 2.0)):       # inside the radius, and outside it: refused all the same
        idx = rng.randint(0, n_y, u).astype(np.int64)
        idx[where] = value
        d2[where] = dist
        with pytest.raises(ValueError, match="outside 0..49"):
            align.plane_moments(x, np.eye(4), y, nrm, idx, d2, 1.0, device=DEV)
    with pytest.raises(ValueError):
        align.plane_moments(x, np.eye(4), y, nrm, idx[:-1], d2, 1.0, device=DEV)
    with pytest.raises(ValueError):
        align.plane_moments(x, np.eye(4), y, nrm[:-1], idx, d2, 1.0, device=DEV)
    bad_T = np.eye(4)
    bad_T[0, 1] = np.nan
    with pytest.raises(ValueError):
        align.plane_moments(x, bad_T, y, nrm, idx, d2, 1.0, device=DEV)
    # the C entry point: what is refused before the first device call leaves h_out alone
    d = [torch.from_numpy(v).to(DEV) for v in (x, y, nrm, np.zeros(u, np.int64), d2)]
    ws = torch.empty(sg_lib.sg_align_plane_moments_ws_bytes(u), dtype=torch.uint8, device=DEV)
    out, T34, org = np.full(31, 7.0), np.ascontiguousarray(np.eye(4)[:3]), np.zeros(3)

    def call(n_points=u, t=T34, origin=org, max_d2=1.0, ns=3, ws_bytes=ws.numel()):
        return sg_lib.sg_align_plane_moments(d[0].data_ptr(), 3, n_points, t.ctypes.data, d[1].data_ptr(), 3, n_y, d[2].data_ptr(), ns, d[3].data_ptr(),
                                             d[4].data_ptr(), max_d2, origin.ctypes.data, out.ctypes.data, ws.data_ptr(), ws_bytes, None)
    assert call(t=np.ascontiguousarray(bad_T[:3])) == hip.SG_EINVAL and call(origin=np.array([0, np.inf, 0])) == hip.SG_EINVAL
    assert call(max_d2=float("nan")) == hip.SG_EINVAL and call(ns=2) == hip.SG_EINVAL and call(ws_bytes=8) == hip.SG_EINVAL
    assert call(n_points=-1) == hip.SG_EINVAL and call(n_points=(1 << 27) + 1) == hip.SG_EUNSUP
    assert (out == 7.0).all()
    assert sg_lib.sg_align_plane_moments_ws_bytes(-1) == 0 and sg_lib.sg_align_plane_moments_ws_bytes((1 << 27) + 1) == 0
    assert sg_lib.sg_align_plane_moments_ws_bytes(1 << 27) > 0
    assert sg_lib.sg_align_plane_moments(None, 3, 0, T34.ctypes.data, None, 3, n_y, None, 3, None, None, 1.0, org.ctypes.data, out.ctypes.data, None, 0,
                                         None) == hip.SG_OK               # U = 0 touches no device memory
    assert out.tobytes() == np.zeros(31).tobytes()
    assert call() == hip.SG_OK and out[0] + out[1] == (d2 <= 1.0).sum()


def _exact_case(name, normals):
    """room(1, 4096) against every second of its points under the inverse of a pose: both metrics on the same input"""
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    pose = A.pose(*A.POSES[name])
    moving = A.apply(fixed[::2], A.inverse(pose))
    al = align.icp(moving, fixed, 0.25, device=DEV, metric="plane", normals=normals)
    point = align.icp(moving, fixed, 0.25, device=DEV)
    off = A.corner_shift(_corners(moving), al.T, pose)
    print(name, "plane: searches", al.iterations, "converged", al.converged, "inliers", al.inliers, "skipped", al.skipped,
          "rms %.3g -> %.3g" % (al.rms_before, al.rms_after), "plane rms %.3g -> %.3g" % (al.plane_rms_before, al.plane_rms_after),
          "corner displacement %.3g | point: searches %d, %.3g" % (off, point.iterations, A.corner_shift(_corners(moving), point.T, pose)))
    assert al.converged == "min_delta" and al.metric == "plane"
    assert off < 2.0 ** -20 * float(np.abs(fixed).max())
    assert al.iterations < point.iterations
    assert al.inliers == 2048 and al.skipped == 0 and bool(al.inlier.all())
    assert np.array_equal(al.idx.cpu().numpy(), 2 * np.arange(2048))
    assert al.plane_rms_after < 1e-6 < al.plane_rms_before and al.plane_rms_before <= al.rms_before and al.rms_after < 1e-6
    assert abs(al.rotation_deg - A.POSES[name][0]) < 1e-3 and al.translation == [float(v) for v in al.T[:3, 3]]
    assert tuple(al.scalars()) == align.SCALARS + align.PLANE_SCALARS
    R3 = al.T[:3, :3]
    assert np.abs(R3.T @ R3 - np.eye(3)).max() <= 16 * 2.0 ** -52 and np.array_equal(al.T[3], [0, 0, 0, 1])


@pytest.mark.parametrize("name", sorted(A.POSES))
def test_icp_plane_exact_case_ends_at_the_true_pose_in_fewer_searches(name):
    """device kNN-10 normals (normals=None).  The NumPy reference: 4 and 5 searches, 4.1e-9 m and 6.3e-9 m from the true pose"""
    _exact_case(name, None)


@pytest.mark.parametrize("name", sorted(A.POSES))
def test_icp_plane_with_the_callers_normals(name):
    """the analytic face normals of the room as normals=; a [N, 6] array serves as well as a [N, 3] one"""
    nrm = P.room_normals(A.room(1, 4096))
    _exact_case(name, nrm if name == POSE else np.concatenate([nrm, np.ones_like(nrm)], 1))


@pytest.mark.parametrize("name", sorted(A.POSES))
def test_icp_plane_resampled_case_beats_point_to_point(name):
    """another sampling of the same room: no pose has zero residual.  The reference loop runs on the device's own normals (the same
    bytes): 5 searches, 1.79 mm and 1.94 mm from the true pose with NumPy's normals; point-to-point needs 28 and 39 and ends 11.5 mm and
    12.1 mm away."""
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    pose = A.pose(*A.POSES[name])
    moving = A.apply(A.room(2, 3000), A.inverse(pose))
    nrm = align.fixed_normals(fixed, 10, device=DEV).cpu().numpy()
    assert nrm.dtype == np.float32 and nrm.shape == (4096, 3) and P.usable_normal(nrm.astype(np.float64)).all()
    al = align.icp(moving, fixed, 0.25, device=DEV, metric="plane", normals=nrm)
    by_default = align.icp(moving, fixed, 0.25, device=DEV, metric="plane")          # normals=None computes the same normals
    assert by_default.T.tobytes() == al.T.tobytes() and by_default.scalars() == al.scalars()
    point = align.icp(moving, fixed, 0.25, device=DEV)
    ref = P.icp(moving, fixed, nrm, 0.25)
    off, point_off, ref_off = (A.corner_shift(_corners(moving), t, pose) for t in (al.T, point.T, ref["T"]))
    print(name, "plane: searches", al.iterations, "(reference %d)" % ref["iterations"], "converged", al.converged, "inliers", al.inliers,
          "rms %.4g -> %.4g" % (al.rms_before, al.rms_after), "plane rms %.4g -> %.4g" % (al.plane_rms_before, al.plane_rms_after),
          "displacement from the true pose %.6g (reference %.6g) | point: searches %d, %.6g" % (off, ref_off, point.iterations, point_off))
    assert ref["converged"] == "min_delta"
    assert off < point_off
    assert off <= 2 * ref_off
    assert al.iterations < point.iterations
    # the returned pose itself: the reference's apply, search and moments there, the device's moments on them, and the next step
    c, length = 0.5 * (fixed.min(0).astype(np.float64) + fixed.max(0)), 0.5 * float(np.linalg.norm(fixed.max(0).astype(np.float64) - fixed.min(0)))
    idx, d2 = A.search(A.apply(moving, al.T), fixed)
    want, mag = P.moments(moving, al.T, fixed, nrm, idx, d2, 0.25, c)
    got = align.plane_moments(moving, al.T, fixed, nrm, idx, d2, 0.25, c, device=DEV)
    assert got[0] == want[0] and got[1] == want[1] == 0
    assert (np.abs(got - want) <= moving.shape[0] * 2.0 ** -52 * mag).all()
    gap = float(np.abs(align.plane_solve(got, al.T, c, length) - P.solve(got, al.T, c, length)[0]).max())
    print(name, "|next T - reference step| %.3g (gate %.3g)" % (gap, SOLVE_BOUND))
    assert gap <= SOLVE_BOUND


def test_icp_plane_refusals():
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    moving = A.apply(fixed[::2], A.inverse(A.pose(*A.POSES[POSE])))
    rng = np.random.RandomState(14)
    flat = np.concatenate([rng.rand(600, 2) * [2, 1.5], np.zeros((600, 1))], 1).astype(np.float32)      # both clouds on one plane
    up = np.repeat(np.array([[0, 0, 1]], np.float32), 600, 0)
    with pytest.raises(ValueError, match="max_dist") as e:
        align.icp(flat[::2], flat, 0.25, device=DEV, metric="plane", normals=up)
    assert "plane" in str(e.value) and "degenerate" in str(e.value)
    with pytest.raises(ValueError, match="skipped") as e:
        align.icp(moving, fixed, 0.25, device=DEV, metric="plane", normals=np.zeros((4096, 3), np.float32))
    assert "max_dist" in str(e.value) and "every pair" in str(e.value)
    with pytest.raises(ValueError, match="max_dist"):
        align.icp(moving, fixed, 1e-6, device=DEV, metric="plane", normals=P.room_normals(fixed))      # no candidate at all
    with pytest.raises(ValueError, match="metric='plane'"):
        align.icp(moving, fixed, 0.25, device=DEV, metric="point", normals=P.room_normals(fixed))
    with pytest.raises(ValueError, match="metric"):
        align.icp(moving, fixed, 0.25, device=DEV, metric="bogus")
    with pytest.raises(ValueError):
        align.icp(moving, fixed, 0.25, device=DEV, metric="plane", normals=P.room_normals(fixed)[:-1])
    al = align.icp(moving, fixed, 0.25, max_iter=2, device=DEV, metric="plane", normals=P.room_normals(fixed))
    assert al.converged is False and al.iterations == 2


def test_metric_point_is_what_icp_returned_before():
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    moving = A.apply(fixed[::2], A.inverse(A.pose(*A.POSES["3deg_4cm"])))
    plain, point = align.icp(moving, fixed, 0.25, device=DEV), align.icp(moving, fixed, 0.25, device=DEV, metric="point")
    assert plain.T.tobytes() == point.T.tobytes() and plain.scalars() == point.scalars()
    assert tuple(point.scalars()) == align.SCALARS and plain.converged == "fixed point"
    assert np.array_equal(plain.idx.cpu().numpy(), point.idx.cpu().numpy())


def _tree(root, scene, xyz, faces=None):
    from seggroup_amd import prepare
    os.makedirs(os.path.join(root, scene))
    path = os.path.join(root, scene, scene + "_vh_clean_2.ply")
    if faces is None:
        R.write_vertex_only_ply(path, xyz, np.zeros(xyz.shape, np.uint8))
    else:
        prepare.write_ply(path, xyz, np.zeros(xyz.shape, np.uint8), faces)


def _results(root, scene, m, seed=8, s=23):
    from seggroup_amd import pseudo_labels
    rng = np.random.RandomState(seed)
    tables, sov = rng.randint(-1, 40, (14, s)).astype(np.int32), rng.randint(-1, s, m).astype(np.int32)
    loose = rng.randint(0, 40, m).astype(np.int32)
    src = os.path.join(root, "results", "e", scene, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    np.save(os.path.join(src, "final.sem.npy"), loose)
    return tables, sov, loose


def _outputs(root2, scene):
    from seggroup_amd import pseudo_labels, transfer
    dst = os.path.join(root2, "results", "e", scene, "epoch_last")
    with np.load(os.path.join(dst, scene + transfer.MAP_SUFFIX)) as z:
        npz = {k: z[k] for k in z.files}
    return pseudo_labels.load(dst), np.load(os.path.join(dst, "final.sem.npy")), npz, dst


def test_transfer_align_metric_plane_carries_labels_between_two_poses(tmp_path):
    """8p's transfer fixture: the target is the source's every second vertex moved by 10 degrees and 15 cm"""
    from seggroup_amd import align, pseudo_labels, transfer
    scene = "scene0071_00"
    src_xyz = A.room(1, 4096).copy()
    sub = 2 * np.arange(2048)
    pose = A.pose(*A.POSES[POSE])
    dst_xyz = A.apply(src_xyz[sub], A.inverse(pose))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tree(a, scene, src_xyz)
    _tree(b, scene, dst_xyz)
    tables, sov, loose = _results(str(tmp_path), scene, src_xyz.shape[0])
    common = dict(root=str(tmp_path), device=DEV)

    # refused before anything runs
    refused = str(tmp_path / "refused")
    with pytest.raises(ValueError, match="--align icp"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, align_metric="plane", **common)
    poses_dir = str(tmp_path / "empty")
    os.makedirs(poses_dir)
    with pytest.raises(ValueError, match="--align icp"):
        transfer.transfer_results(a, b, "e", "epoch_last", refused, align=poses_dir, align_metric="plane", **common)
    with pytest.raises(ValueError, match="--normals-k"):
        align.align_scans(b, a, 0.25, refused, normals_k=10, device=DEV)
    argv = ["--from-scans", a, "--to-scans", b, "-n", "e", "--out", refused, "--root", str(tmp_path)]
    for extra in (["--align-metric", "plane"], ["--align", poses_dir, "--align-metric", "plane"], ["--align-metric", "point"]):
        with pytest.raises(SystemExit) as e:
            transfer.main(argv + extra)
        assert e.value.code == 2
    for extra in (["--normals-k", "10"], ["--normals-k", "10", "--metric", "point"], ["--metric", "bogus"]):
        with pytest.raises(SystemExit) as e:
            align.main(["--moving-scans", b, "--fixed-scans", a, "--max-dist", "0.25", "--out", refused] + extra)
        assert e.value.code == 2
    assert not os.path.exists(refused)

    plane_root = str(tmp_path / "plane")
    report, missing = transfer.transfer_results(a, b, "e", "epoch_last", plane_root, align="icp", align_max_dist=0.25, align_metric="plane", **common)
    assert missing == {} and list(report) == [scene]
    lab, sem, npz, plane_dst = _outputs(plane_root, scene)
    assert lab.V == 2048 and np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[sub]) and np.array_equal(sem, loose[sub])
    assert sorted(npz) == ["T", "d2", "nearest"] and npz["T"].dtype == np.float64 and npz["T"].shape == (4, 4)
    assert np.array_equal(npz["nearest"], sub) and float(npz["d2"].max()) < 1e-10
    assert A.corner_shift(_corners(dst_xyz), npz["T"], pose) < 2.0 ** -20 * float(np.abs(src_xyz).max())
    e = report[scene]
    assert e == json.load(open(os.path.join(plane_root, transfer.REPORT_NAME)))["scenes"][scene]
    assert sorted(e["align"]) == sorted(("source", "normals") + align.SCALARS + align.PLANE_SCALARS)
    assert e["align"]["metric"] == "plane" and e["align"]["normals"] == "knn-10" and e["align"]["source"] == "icp"
    assert e["align"]["converged"] == "min_delta" and e["align"]["inliers"] == 2048 and e["align"]["skipped"] == 0
    assert e["align"]["plane_rms_after"] < 1e-6 < e["align"]["plane_rms_before"]
    assert e["max_distance"] < 1e-5 and e["farther_than"] == {"0.05": 0, "0.1": 0, "0.5": 0}

    # --align-metric point is --align icp as it was: no new key
    point_root = str(tmp_path / "point")
    report_p, _ = transfer.transfer_results(a, b, "e", "epoch_last", point_root, align="icp", align_max_dist=0.25, align_metric="point", **common)
    assert sorted(report_p[scene]["align"]) == sorted(("source",) + align.SCALARS) and report_p[scene]["align"]["iterations"] > e["align"]["iterations"]

    # the command writes what --align DIR reads; the same label files come out
    poses = str(tmp_path / "poses")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.align", "--moving-scans", b, "--fixed-scans", a, "--max-dist", "0.25", "--out", poses, "--workers", "1",
           "--metric", "plane"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 scenes aligned, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(os.path.join(poses, scene + align.ALIGN_SUFFIX)))
    assert np.array_equal(np.array(doc["T"]), npz["T"]) and (doc["moving_V"], doc["fixed_V"], doc["max_dist"]) == (2048, 4096, 0.25)
    keys = align.SCALARS + align.PLANE_SCALARS + ("normals",)
    assert {k: doc[k] for k in keys} == {k: e["align"][k] for k in keys}
    entry = json.load(open(os.path.join(poses, align.REPORT_NAME)))["scenes"][scene]
    assert entry["metric"] == "plane" and entry["normals"] == "knn-10" and entry["converged"] == "min_delta"
    dir_root = str(tmp_path / "dir")
    report2, _ = transfer.transfer_results(a, b, "e", "epoch_last", dir_root, align=poses, **common)
    _, _, npz2, dir_dst = _outputs(dir_root, scene)
    for f in (pseudo_labels.SGL_NAME, "final.sem.npy"):
        assert open(os.path.join(dir_dst, f), "rb").read() == open(os.path.join(plane_dst, f), "rb").read(), f
    assert sorted(npz2) == sorted(npz) and all(npz2[k].tobytes() == npz[k].tobytes() for k in npz)
    assert report2[scene]["align"] == dict({k: e["align"][k] for k in align.SCALARS}, source=os.path.join(poses, scene + align.ALIGN_SUFFIX))

    vote_root = str(tmp_path / "vote")
    report3, _ = transfer.transfer_results(a, b, "e", "epoch_last", vote_root, align="icp", align_max_dist=0.25, align_metric="plane", vote_k=5, **common)
    _, _, npz3, _ = _outputs(vote_root, scene)
    assert sorted(npz3) == ["T", "d2", "nearest", "rep", "tied", "votes"] and np.array_equal(npz3["nearest"], sub)
    assert npz3["T"].tobytes() == npz["T"].tobytes() and report3[scene]["vote"] == 5 and report3[scene]["align"] == e["align"]


def _sheet(n, origin, u, v, first):
    """an n x n triangulated grid on origin + s u + t v -> (vertices float64 [n*n,3], faces int32 [2(n-1)^2,3] numbered from `first`)"""
    s, t = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    pts = np.asarray(origin, np.float64) + s.reshape(-1, 1) * np.asarray(u, np.float64) + t.reshape(-1, 1) * np.asarray(v, np.float64)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    k = (i * n + j).reshape(-1) + first
    return pts, np.concatenate([np.stack([k, k + n, k + 1], 1), np.stack([k + 1, k + n, k + n + 1], 1)]).astype(np.int32)


def test_a_source_with_faces_gives_face_normals(tmp_path):
    """three triangulated sheets that meet in a corner, of different extents so that no symmetry maps the corner onto itself"""
    from seggroup_amd import align, oversegment, transfer
    scene = "scene0072_00"
    n = 20
    # the sheets stop 5 cm short of each other's planes: no two vertices share a position, so every target vertex has ONE nearest source
    parts = [_sheet(n, (0, 0, 0), (2.0, 0, 0), (0, 1.5, 0), 0), _sheet(n, (0, 0.05, 0.05), (0, 1.45, 0), (0, 0, 0.95), n * n),
             _sheet(n, (0.05, 0, 0.05), (0, 0, 0.95), (1.95, 0, 0), 2 * n * n)]
    src_xyz = (np.concatenate([p for p, _ in parts]) - [1.0, 0.75, 0.5]).astype(np.float32)
    faces = np.concatenate([f for _, f in parts])
    sub = np.arange(0, src_xyz.shape[0], 3)
    pose = A.pose(*A.POSES["3deg_4cm"])
    dst_xyz = A.apply(src_xyz[sub], A.inverse(pose))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tree(a, scene, src_xyz, faces)
    _tree(b, scene, dst_xyz)
    tables, sov, loose = _results(str(tmp_path), scene, src_xyz.shape[0], seed=9)
    nrm, how = align.scan_normals(src_xyz, faces, device=DEV)
    assert how == "faces" and nrm.cpu().numpy().tobytes() == oversegment.vertex_normals(src_xyz, faces, device=DEV).cpu().numpy().tobytes()
    assert align.scan_normals(src_xyz, faces[:0], 5, device=DEV)[1] == "knn-5"
    out = str(tmp_path / "out")
    report, _ = transfer.transfer_results(a, b, "e", "epoch_last", out, align="icp", align_max_dist=0.25, align_metric="plane", root=str(tmp_path),
                                          device=DEV)
    rec = report[scene]["align"]
    print("faces:", rec)
    assert rec["metric"] == "plane" and rec["normals"] == "faces" and rec["converged"] == "min_delta" and rec["skipped"] == 0
    lab, sem, npz, _ = _outputs(out, scene)
    assert np.array_equal(npz["nearest"], sub) and np.array_equal(lab.seg_of_vertex, sov[sub]) and np.array_equal(sem, loose[sub])
    assert A.corner_shift(_corners(dst_xyz), npz["T"], pose) < 2.0 ** -20 * float(np.abs(src_xyz).max())
    poses = str(tmp_path / "poses")
    rep2, _ = align.align_scans(b, a, 0.25, poses, workers=1, device=DEV, metric="plane")
    assert rep2[scene]["normals"] == "faces" and json.load(open(os.path.join(poses, scene + align.ALIGN_SUFFIX)))["normals"] == "faces"
    assert np.array_equal(align.read_align(os.path.join(poses, scene + align.ALIGN_SUFFIX))["T"], npz["T"])
