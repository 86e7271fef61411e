"""Rigid alignment of two clouds without a GPU: the NumPy restatement (tests/align_ref.py) recovers known poses, and
sg_align_solve -- host code, no device call -- gives a proper rotation, orthogonal to a few units of the last place, that agrees with
NumPy's Kabsch on well-conditioned, planar and mirrored pair sets, and refuses what does not determine a pose."""
import json
import os

import numpy as np
import pytest

import align_ref as A
from conftest import ROOT

ORTHO_BOUND = 16 * 2.0 ** -52
# Agreement with Kabsch on LAPACK's SVD has no derivable bound here.  Measured over solve_cases() on the CPU: the largest entry difference
# of the 4x4 transforms is 5.0e-12 (a translation entry of a case at the 1,000 m offset, where 6e-15 of rotation meets a 1,500 m lever; 6.0e-15 over the rotation entries).  The gate is
# 16 times that, and stays below 1e-9.
SOLVE_MEASURED = 5.0e-12
SOLVE_BOUND = min(16 * SOLVE_MEASURED, 1e-9)


def _pairs(seed, s2, s3, n, offset=0.0, mirrored=False, planar=False):
    """n centred points whose covariance has the singular values 1, s2^2, s3^2 BY CONSTRUCTION (orthonormal columns scaled by 1, s2, s3 and
    turned by a random rotation), their images under a random pose, and the origins the moments are taken about"""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.randn(n, 3) - rng.randn(n, 3).mean(0))
    q -= q.mean(0)
    w = np.eye(3) if planar else np.linalg.qr(rng.randn(3, 3))[0]
    a64 = (q * np.array([1.0, s2, 0.0 if planar else s3])) @ w.T
    P = A.pose(rng.uniform(5, 175), rng.uniform(0, 2), axis=rng.randn(3), direction=rng.randn(3))
    ox = np.array([offset, -offset, 0.5 * offset])
    a = (a64 + ox).astype(np.float32)
    b = A.apply(a, P)
    if mirrored:
        b = b * np.array([-1, 1, 1], np.float32)
    oy = 0.5 * (b.astype(np.float64).min(0) + b.astype(np.float64).max(0))
    return a, b, ox, oy


def solve_cases():
    """name -> (a, b, origin_x, origin_y): well-conditioned sets (second singular value >= 0.1 of the first), a planar set and mirrored
    sets (the unconstrained optimum is a reflection; the third singular value at most half the second, so the flipped direction is
    determined), at the origin and at a 1,000 m offset"""
    cases = {}
    for i, (s2, s3, n) in enumerate(((1.0, 1.0, 3), (0.9, 0.5, 4), (0.6, 0.6, 17), (0.4, 0.05, 200), (0.35, 0.2, 1000), (0.8, 0.01, 64))):
        for off in (0.0, 1000.0):
            cases["well_%d_%g" % (i, off)] = _pairs(10 + i, s2, s3, max(n, 4), off)
    for off in (0.0, 1000.0):
        cases["planar_%g" % off] = _pairs(30, 0.5, 0.0, 300, off, planar=True)
        cases["mirror_a_%g" % off] = _pairs(31, 0.8, 0.4, 300, off, mirrored=True)
        cases["mirror_b_%g" % off] = _pairs(32, 0.4, 0.1, 50, off, mirrored=True)
    return cases


def _moments(a, b, ox, oy):
    n = a.shape[0]
    return A.moments(a, b, np.arange(n), np.zeros(n, np.float32), np.inf, ox, oy)[0]


def _solve(lib, m, ox, oy):
    m, ox, oy = (np.ascontiguousarray(v, np.float64) for v in (m, ox, oy))
    T = np.zeros(12)
    rc = lib.sg_align_solve(m.ctypes.data, ox.ctypes.data, oy.ctypes.data, T.ctypes.data)
    return rc, np.vstack([T.reshape(3, 4), [0, 0, 0, 1]])


def test_the_reference_recovers_known_poses():
    fixed = A.room(1, 4096)
    assert fixed.dtype == np.float32 and fixed.shape == (4096, 3) and A.room(1, 4096) is fixed
    rng = np.random.RandomState(5)
    for deg, shift in ((0.0, 0.0), (3.0, 0.04), (170.0, 3.0)):
        P = A.pose(deg, shift)
        # the helper's own rounding: Rodrigues' formula is about ten operations an entry, the products three more
        assert np.abs(P[:3, :3].T @ P[:3, :3] - np.eye(3)).max() < 1e-14 and np.abs(A.inverse(P) @ P - np.eye(4)).max() < 1e-14
        a = rng.randn(50, 3).astype(np.float32)
        b = A.apply(a, P)
        T = A.solve(_moments(a, b, (0, 0, 0), (0, 0, 0)))
        assert np.abs(T - P).max() < 1e-6                       # b is rounded to fp32: 6e-8 relative on every coordinate
    P = A.pose(3.0, 0.04)
    moving = A.apply(fixed[::8], A.inverse(P))
    r = A.icp(moving, fixed, 0.25)
    assert r["converged"] == "fixed point" and r["inliers"] == 512 and np.array_equal(r["idx"], 8 * np.arange(512))
    assert A.corner_shift(A.box_corners(*A.box_of(moving)), r["T"], P) < 2.0 ** -20 * float(np.abs(fixed).max())
    assert r["rms_after"] < 1e-6 < r["rms_before"]


def test_solve_gives_a_proper_rotation_that_agrees_with_kabsch(sg_lib):
    worst = worst_rot = 0.0
    for name, (a, b, ox, oy) in solve_cases().items():
        m = _moments(a, b, ox, oy)
        H = m[7:16].reshape(3, 3) - np.outer(m[1:4], m[4:7]) / m[0]
        S = np.linalg.svd(H, compute_uv=False)
        if name.startswith("well"):
            assert S[1] >= 0.1 * S[0], name
        if name.startswith("planar"):
            assert S[2] < 1e-6 * S[0] and S[1] >= 0.1 * S[0], name
        rc, T = _solve(sg_lib, m, ox, oy)
        assert rc == 0, (name, sg_lib.sg_last_error())
        want = A.solve(m, ox, oy)
        R = T[:3, :3]
        assert np.linalg.det(R) > 0, name
        ortho = float(np.abs(R.T @ R - np.eye(3)).max())
        diff = float(np.abs(T - want).max())
        print("%-14s n %5d  s2/s1 %.3f  s3/s1 %.2e  |RtR - I| %.2e  |T - kabsch| %.2e (rotation %.2e)" %
              (name, a.shape[0], S[1] / S[0], S[2] / S[0], ortho, diff, np.abs(R - want[:3, :3]).max()))
        worst, worst_rot = max(worst, diff), max(worst_rot, float(np.abs(R - want[:3, :3]).max()))
        assert ortho <= ORTHO_BOUND, name
        assert diff <= SOLVE_BOUND, name
        if name.startswith("mirror"):                           # the unconstrained optimum is a reflection
            U, _, Vt = np.linalg.svd(H)
            assert np.linalg.det(Vt.T @ U.T) < 0, name
        else:                                                   # noise-free pairs: the pose comes back to fp32 rounding of b
            assert float(np.abs(R @ a.astype(np.float64).T + T[:3, 3:] - b.astype(np.float64).T).max()) <= 4 * 2.0 ** -24 * float(np.abs(b).max()), name
    print("largest |T - kabsch| %.3e, over the rotation entries %.3e; bound %.3e" % (worst, worst_rot, SOLVE_BOUND))


def test_solve_refuses_what_does_not_determine_a_pose(sg_lib):
    rng = np.random.RandomState(3)
    t = rng.randn(40, 1).astype(np.float32)
    line = t * np.array([[0.5, -1.0, 2.0]], np.float32)                       # collinear, exactly in fp32 for these factors
    a, b, ox, oy = _pairs(10, 0.9, 0.5, 40)
    for name, (aa, bb) in {"collinear": (line, A.apply(line, A.pose(20.0, 0.3))), "n = 2": (a[:2], b[:2]), "n = 0": (a[:0], b[:0]),
                           "one point": (np.repeat(a[:1], 9, 0), np.repeat(b[:1], 9, 0))}.items():
        rc, _ = _solve(sg_lib, _moments(aa, bb, ox, oy), ox, oy)
        assert rc == -5 and b"degenerate" in sg_lib.sg_last_error(), (name, rc, sg_lib.sg_last_error())
        with pytest.raises(A.Degenerate):
            A.solve(_moments(aa, bb, ox, oy), ox, oy)
    good = _moments(a, b, ox, oy)
    assert _solve(sg_lib, good, ox, oy)[0] == 0
    for slot in (0, 2, 9, 16):
        for bad in (np.nan, np.inf, -np.inf):
            m = good.copy()
            m[slot] = bad
            assert _solve(sg_lib, m, ox, oy)[0] == -1, (slot, bad)
    assert _solve(sg_lib, good, [np.nan, 0, 0], oy)[0] == -1 and _solve(sg_lib, good, ox, [0, np.inf, 0])[0] == -1
    m = good.copy()
    m[0] = -4.0
    assert _solve(sg_lib, m, ox, oy)[0] == -1
    p = good.ctypes.data
    assert sg_lib.sg_align_solve(None, p, p, p) == -1 and sg_lib.sg_align_solve(p, p, p, None) == -1


def test_the_python_layer_runs_the_solve_without_a_device(sg_lib):
    from seggroup_amd import align, hip
    a, b, ox, oy = solve_cases()["well_3_1000"]
    m = _moments(a, b, ox, oy)
    T = align.solve(m, ox, oy)
    assert T.shape == (4, 4) and T.dtype == np.float64 and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.array_equal(T, _solve(sg_lib, m, ox, oy)[1])
    with pytest.raises(hip.SgError, match="degenerate") as e:
        align.solve(_moments(a[:2], b[:2], ox, oy), ox, oy)
    assert e.value.code == hip.SG_EUNSUP
    bad = m.copy()
    bad[5] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        align.solve(bad, ox, oy)
    with pytest.raises(ValueError):
        align.as_transform(np.eye(3))
    with pytest.raises(ValueError):
        align.as_transform(np.full((4, 4), np.nan))
    assert align.rotation_deg(A.pose(10.0, 0.15)) == pytest.approx(10.0, abs=1e-9)
    c = align.box_corners([0, 1, 2], [3, 4, 5])
    assert np.array_equal(c, A.box_corners(np.array([0, 1, 2.0]), np.array([3, 4, 5.0])))
    assert align.corner_shift(c, np.eye(4), A.pose(0.0, 0.25)) == pytest.approx(0.25, abs=1e-15)


def test_the_design_table_is_the_timing_tools_output():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import time_align
    doc = json.load(open(os.path.join(ROOT, "profiles", "align_time.json")))
    assert [(m["U"], m["N"]) for m in doc["shapes"]] == [(150000, 150000), (1058050, 1058050)]
    assert time_align.table(doc) in open(os.path.join(ROOT, "DESIGN.md")).read()
