"""Point-to-plane ICP without a GPU: the NumPy restatement (tests/align_plane_ref.py) reproduces the figures the method was
chosen on, and sg_align_plane_solve -- host code, no device call -- gives a proper rotation, orthogonal to a few units of the last place,
that agrees with the eigh-based reference step on rooms, plane triples and box corners, refuses what leaves a motion free and returns the
pose it was given when the pairs have no residual."""
import json
import os

import numpy as np
import pytest

import align_plane_ref as P
import align_ref as A
from conftest import ROOT

ORTHO_BOUND = 16 * 2.0 ** -52
# Agreement of T_new with the reference step (LAPACK's eigh, SVD re-orthonormalisation) has no derivable bound.  Measured over solve_cases()
# on the CPU: the largest entry difference is 2.3e-13 (a translation entry of a case at the 1,000 m offset, where 1e-16 of rotation
# difference meets a 1,500 m lever; 4.4e-16 over the rotation entries and over all entries at the origin).  The gate is 16 times that.
SOLVE_MEASURED = 2.3e-13
SOLVE_BOUND = 16 * SOLVE_MEASURED
# A residual-free set: the step is exactly zero, so T_new is T with its rotation re-orthonormalised and t_new = ((t - c) + c) + 0.
# Measured over solve_cases() with the 10 degree / 15 cm pose (a product of doubles, orthogonal to 2e-16 itself) as T: 3.2e-14 at the
# 1,000 m offset ((t - c) + c rounds at 1,000 m, 1.1e-13 an ulp), 1.1e-16 over the rotation entries and over all entries at the origin.
UNCHANGED_MEASURED = 3.2e-14
UNCHANGED_BOUND = 16 * UNCHANGED_MEASURED
FAR = np.array([1000.0, -1000.0, 500.0])


def _patch(rng, n, origin, u, v):
    """n points on the parallelogram origin + s u + t v and its unit normal"""
    o, u, v = (np.asarray(t, np.float64) for t in (origin, u, v))
    pts = o + rng.rand(n, 1) * u + rng.rand(n, 1) * v
    nrm = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
    return pts, np.repeat(nrm[None], n, 0)


def _planes(seed, patches, n=300):
    rng = np.random.RandomState(seed)
    parts = [_patch(rng, n, *p) for p in patches]
    return np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts])


THREE_PLANES = (((0, 0, 0), (2.0, 0, 0), (0, 1.5, 0)), ((0, 0, 0), (0, 1.5, 0), (0, 0, 1.0)), ((0, 0, 0), (2.0, 0, 0), (0, 0, 1.0)))
BOX_CORNER = (((0.1, -0.2, -0.3), (0.9, 0, 0), (0, 0.7, 0)), ((1.0, -0.2, -1.0), (0, 0.7, 0), (0, 0, 0.7)), ((0.1, 0.5, -1.0), (0.9, 0, 0), (0, 0, 0.7)))
ONE_PLANE = (((-1, -1, 0.25), (2.0, 0, 0), (0, 2.0, 0)),)
TWO_PLANES = (((0, 0, 0), (2.0, 0, 0), (0, 1.5, 0)), ((0, 0, 0), (2.0, 0, 0), (0, 0, 1.0)))      # both contain the x axis: sliding along it is free


def _pairs(points, normals, offset, deg=2.0, shift=0.03):
    """the fixed cloud (fp32) moved to `offset`, its normals, and the moving cloud: the fixed one under the inverse of a small pose about the
    cloud's middle -> (x, y, n, centre, half diagonal, the pose)"""
    y = (np.asarray(points, np.float64) + offset).astype(np.float32)
    lo, hi = A.box_of(y)
    c, length = 0.5 * (lo + hi), 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))
    to_mid, back = np.eye(4), np.eye(4)
    to_mid[:3, 3], back[:3, 3] = -c, c
    pose = back @ A.pose(deg, shift) @ to_mid
    return A.apply(y, A.inverse(pose)), y, np.asarray(normals, np.float32), c, length, pose


def solve_cases():
    """name -> (x, y, normals, centre, length, pose): the room, three perpendicular planes and a box corner, at the origin and 1,000 m off"""
    room = A.room(1, 4096)
    sets = {"room": (room, P.room_normals(room)), "three_planes": _planes(41, THREE_PLANES), "box_corner": _planes(42, BOX_CORNER)}
    return {"%s_%g" % (k, f): _pairs(p, n, f * FAR) for k, (p, n) in sets.items() for f in (0.0, 1.0)}


def degenerate_cases():
    sets = {"one_plane": _planes(43, ONE_PLANE), "two_planes": _planes(44, TWO_PLANES)}
    return {"%s_%g" % (k, f): _pairs(p, n, f * FAR) for k, (p, n) in sets.items() for f in (0.0, 1.0)}


def _moments(x, y, n, c, T=np.eye(4)):
    u = x.shape[0]
    return P.moments(x, T, y, n, np.arange(u), np.zeros(u, np.float32), np.inf, c)[0]


def _solve(lib, m, c, length, T, step=True):
    m, c, T34 = (np.ascontiguousarray(v, np.float64) for v in (m, c, np.asarray(T, np.float64)[:3]))
    out, s = np.full((4, 4), 7.0), np.full(6, 7.0)
    rc = lib.sg_align_plane_solve(m.ctypes.data, c.ctypes.data, float(length), T34.ctypes.data, out.ctypes.data, s.ctypes.data if step else None)
    return rc, out, s


def test_the_reference_reproduces_the_figures_the_method_was_chosen_on():
    """room(1, 4096) fixed, max_dist 0.25, NumPy kNN-10 covariance normals: searches and distance from the true pose"""
    fixed = A.room(1, 4096)
    nrm = P.knn_normals(fixed, 10)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-12
    analytic = P.room_normals(fixed)
    assert (np.abs((nrm * analytic).sum(1)) > 0.99).mean() > 0.85           # edges and corners of the room mix two or three faces
    want = {("exact", "3deg_4cm"): (4, 4.1e-9), ("exact", "10deg_15cm"): (5, 6.3e-9),
            ("resampled", "3deg_4cm"): (5, 1.79e-3), ("resampled", "10deg_15cm"): (5, 1.94e-3)}
    for (kind, name), (searches, off_want) in want.items():
        pose = A.pose(*A.POSES[name])
        moving = A.apply(fixed[::2] if kind == "exact" else A.room(2, 3000), A.inverse(pose))
        r = P.icp(moving, fixed, nrm, 0.25)
        off = A.corner_shift(A.box_corners(*A.box_of(moving)), r["T"], pose)
        print(kind, name, "searches", r["iterations"], "displacement %.4g" % off, "plane rms %.3g -> %.3g" % (r["plane_rms_before"], r["plane_rms_after"]))
        assert r["converged"] == "min_delta" and r["iterations"] == searches and r["skipped"] == 0
        assert r["inliers"] == moving.shape[0]
        assert off == pytest.approx(off_want, rel=0.02 if kind == "resampled" else 0.5)  # the figures as printed; 1e-9 m is rounding noise
        assert off < (2.0 ** -20 * float(np.abs(fixed).max()) if kind == "exact" else 2.5e-3)


def test_solve_gives_a_proper_rotation_that_agrees_with_the_reference_step(sg_lib):
    worst = worst_rot = worst_ortho = 0.0
    for name, (x, y, n, c, length, pose) in solve_cases().items():
        m = _moments(x, y, n, c)
        lam, _, _ = P.spectrum(m, length)
        rc, T, s = _solve(sg_lib, m, c, length, np.eye(4))
        assert rc == 0, (name, sg_lib.sg_last_error())
        want, s_want = P.solve(m, np.eye(4), c, length)
        R = T[:3, :3]
        ortho, diff, rot = (float(np.abs(v).max()) for v in (R.T @ R - np.eye(3), T - want, R - want[:3, :3]))
        print("%-18s n %5d  lambda_min / lambda_max %.3f  |RtR - I| %.2e  |T - reference| %.2e (rotation %.2e)  |step - reference| %.2e" %
              (name, x.shape[0], lam[0] / lam[-1], ortho, diff, rot, np.abs(s - s_want).max()))
        worst, worst_rot, worst_ortho = max(worst, diff), max(worst_rot, rot), max(worst_ortho, ortho)
        assert np.linalg.det(R) > 0 and np.array_equal(T[3], [0, 0, 0, 1]), name
        assert ortho <= ORTHO_BOUND, name
        assert diff <= SOLVE_BOUND, name
        assert lam[0] / lam[-1] > 0.01, name
        # one step from 2 degrees and 3 cm lands within the second-order term of the true pose
        assert A.corner_shift(A.box_corners(*A.box_of(x)), T, pose) < 0.2 * A.corner_shift(A.box_corners(*A.box_of(x)), np.eye(4), pose), name
        assert np.array_equal(_solve(sg_lib, m, c, length, np.eye(4), step=False)[1], T), name         # the step pointer is optional
    print("largest |T - reference| %.3e, over the rotation entries %.3e, |RtR - I| %.3e; bounds %.3e, %.3e" %
          (worst, worst_rot, worst_ortho, SOLVE_BOUND, ORTHO_BOUND))


def test_fifty_composed_steps_are_still_a_rotation(sg_lib):
    x, y, n, c, length, _ = solve_cases()["room_1"]
    m = _moments(x, y, n, c)
    T = A.pose(37.0, 0.5)
    for _ in range(50):
        rc, T, _ = _solve(sg_lib, m, c, length, T)
        assert rc == 0
    R = T[:3, :3]
    assert np.linalg.det(R) > 0 and float(np.abs(R.T @ R - np.eye(3)).max()) <= ORTHO_BOUND


def test_solve_refuses_what_leaves_a_motion_free(sg_lib):
    for name, (x, y, n, c, length, _) in degenerate_cases().items():
        m = _moments(x, y, n, c)
        lam, _, _ = P.spectrum(m, length)
        print("%-14s lambda_min / lambda_max %.3e" % (name, lam[0] / lam[-1]))
        assert lam[0] / lam[-1] <= 1e-15, name
        rc, T, s = _solve(sg_lib, m, c, length, np.eye(4))
        assert rc == -5 and b"degenerate" in sg_lib.sg_last_error(), (name, rc, sg_lib.sg_last_error())
        assert (T == 7.0).all() and (s == 7.0).all(), name                  # nothing written
        with pytest.raises(A.Degenerate):
            P.solve(m, np.eye(4), c, length)
    x, y, n, c, length, _ = solve_cases()["room_0"]
    for count in (5, 0):
        m = _moments(x[:count], y[:count], n[:count], c)
        assert m[0] == count
        rc, _, _ = _solve(sg_lib, m, c, length, np.eye(4))
        assert rc == -5 and b"degenerate" in sg_lib.sg_last_error(), (count, rc, sg_lib.sg_last_error())
        with pytest.raises(A.Degenerate):
            P.solve(m, np.eye(4), c, length)
    good = _moments(x, y, n, c)
    assert _solve(sg_lib, good, c, length, np.eye(4))[0] == 0
    for slot in (0, 1, 2, 22, 23, 29, 30):
        for bad in (np.nan, np.inf, -np.inf):
            m = good.copy()
            m[slot] = bad
            assert _solve(sg_lib, m, c, length, np.eye(4))[0] == -1, (slot, bad)
    for bad in (np.nan, np.inf):
        assert _solve(sg_lib, good, [bad, 0, 0], length, np.eye(4))[0] == -1
        assert _solve(sg_lib, good, c, bad, np.eye(4))[0] == -1
        T = np.eye(4)
        T[1, 3] = bad
        assert _solve(sg_lib, good, c, length, T)[0] == -1
    assert _solve(sg_lib, good, c, 0.0, np.eye(4))[0] == -1 and _solve(sg_lib, good, c, -1.0, np.eye(4))[0] == -1
    m = good.copy()
    m[0] = -4.0
    assert _solve(sg_lib, m, c, length, np.eye(4))[0] == -1
    p = good.ctypes.data
    assert sg_lib.sg_align_plane_solve(None, p, 1.0, p, p, None) == -1 and sg_lib.sg_align_plane_solve(p, p, 1.0, p, None, None) == -1


def test_residual_free_pairs_return_the_pose_unchanged(sg_lib):
    worst = worst_rot = 0.0
    for name, (x, y, n, c, length, _) in solve_cases().items():
        m = _moments(y, y, n, c)                                            # the fixed cloud against itself at the identity: r = 0 exactly
        assert m[29] == 0.0 and not m[23:29].any(), name
        rc, T, s = _solve(sg_lib, m, c, length, np.eye(4))
        assert rc == 0 and not s.any() and np.array_equal(T, np.eye(4)), name
        held = A.pose(*A.POSES["10deg_15cm"])
        rc, T, s = _solve(sg_lib, m, c, length, held)                       # the same zero step composed onto a general pose
        diff, rot = float(np.abs(T - held).max()), float(np.abs(T[:3, :3] - held[:3, :3]).max())
        print("%-18s |T_new - T| %.2e (rotation %.2e)" % (name, diff, rot))
        worst, worst_rot = max(worst, diff), max(worst_rot, rot)
        assert rc == 0 and not s.any() and diff <= UNCHANGED_BOUND, name
    print("largest |T_new - T| %.3e, over the rotation entries %.3e; bound %.3e" % (worst, worst_rot, UNCHANGED_BOUND))


def test_the_python_layer_runs_the_plane_solve_without_a_device(sg_lib):
    from seggroup_amd import align, hip
    x, y, n, c, length, _ = solve_cases()["box_corner_1"]
    m = _moments(x, y, n, c)
    T = align.plane_solve(m, np.eye(4), c, length)
    assert T.shape == (4, 4) and T.dtype == np.float64 and np.array_equal(T, _solve(sg_lib, m, c, length, np.eye(4))[1])
    assert np.array_equal(align.plane_solve(m, np.eye(4)[:3], c, length), T)
    dx, dy, dn, dc, dl, _ = degenerate_cases()["one_plane_0"]
    with pytest.raises(hip.SgError, match="degenerate") as e:
        align.plane_solve(_moments(dx, dy, dn, dc), np.eye(4), dc, dl)
    assert e.value.code == hip.SG_EUNSUP
    bad = m.copy()
    bad[25] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        align.plane_solve(bad, np.eye(4), c, length)
    with pytest.raises(ValueError):
        align.plane_solve(m[:17], np.eye(4), c, length)
    with pytest.raises(ValueError):
        align.plane_solve(m, np.eye(3), c, length)
    assert align.METRICS == ("point", "plane") and not set(align.PLANE_SCALARS) & set(align.SCALARS)
    al = align.Alignment(T=np.eye(4), iterations=1, converged=False, inliers=1, rms_before=0.0, rms_after=0.0, rotation_deg=0.0, translation=[0, 0, 0])
    assert tuple(al.scalars()) == align.SCALARS                             # a point-to-point Alignment carries no new key


def test_the_design_table_is_the_plane_timing_tools_output():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import time_align
    doc = json.load(open(os.path.join(ROOT, "profiles", "align_plane_time.json")))
    assert [(m["U"], m["N"]) for m in doc["shapes"]] == [(150000, 150000), (1058050, 1058050)]
    assert time_align.plane_table(doc) in open(os.path.join(ROOT, "DESIGN.md")).read()
