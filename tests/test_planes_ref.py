"""Plane extraction without a GPU: the NumPy restatement alone on the acceptance fixture, sg_plane_fit (host only) against
numpy.linalg.eigh, level_transform, and what the command refuses before any device call."""
import numpy as np
import pytest

import align_ref as A
import planes_ref as PR

# Agreement of the Jacobi fit with LAPACK's eigh has no derivable bound here.  Measured over fit_cases() on the CPU: the largest
# difference of a normal's component is 4.44e-16, of the offset d 6.25e-13 (a plane 1,000 m from the origin: 4e-16 of direction
# against a 1,000 m lever) and 1.67e-16 over the cases at the origin.  The gates are 16 times that.
NORMAL_MEASURED, OFFSET_MEASURED = 4.44e-16, 6.25e-13
NORMAL_BOUND, OFFSET_BOUND = 16 * NORMAL_MEASURED, 16 * OFFSET_MEASURED


def test_the_restatement_finds_the_six_faces_of_the_fixture():
    """the final rules (min_edge = 10 dist, min_sine = 0.1): six planes of 1115 / 934 / 697 / 100 / 88 / 66 points, nothing unlabelled, no
    fenced compare in any round, every face's corners within 4.8e-4 of a plane (the gate is dist = 5e-3)"""
    xyz, P = PR.fixture()
    d = PR.fixture_reference()
    assert not d.fenced, "a compare of a winning round sits on a fence: the device cannot be held to equality on this fixture"
    assert d.planes.shape == (6, 4) and d.points.tolist() == [1115, 934, 697, 100, 88, 66] and int((d.labels < 0).sum()) == 0
    assert d.ransac_count.tolist() == [1116, 936, 697, 100, 88, 66] and d.h.tolist() == [274, 602, 0, 15, 27, 4]
    assert np.array_equal(np.bincount(d.labels, minlength=6), d.points)
    assert (d.rms < 1.5e-3).all() and (d.rms > 0.5e-3).all()              # the jitter is 1e-3
    corners = PR.face_corners(P)
    worst = []
    for f in range(6):
        off = np.abs(corners[f] @ d.planes[:, :3].T + d.planes[:, 3]).max(0)
        worst.append(off.min())
        assert off.min() <= PR.PARAMS["dist"], (f, off)
    print("largest corner distance per face", ["%.3g" % w for w in worst])
    # H = 256 finds the same six faces
    few = PR.detect(xyz, **dict(PR.PARAMS, hypotheses=256))
    assert sorted(few.points.tolist()) == sorted(d.points.tolist())


def _cloud_on_plane(seed, n, normal, centre, noise, extent=(2.0, 1.0)):
    rng = np.random.RandomState(seed)
    nrm = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    a = np.cross(nrm, [0.3, -0.5, 1.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    s, t = (rng.rand(n) - 0.5) * extent[0], (rng.rand(n) - 0.5) * extent[1]
    return np.asarray(centre, np.float64) + s[:, None] * a + t[:, None] * b + (rng.randn(n) * noise)[:, None] * nrm


def fit_cases():
    far = np.array([600.0, -500.0, 620.0])                                # about 1,000 m from the origin
    cases = {}
    for i, normal in enumerate(([0, 0, 1], [1, 0, 0], [1, 0.8, 0.6],[0.2, -0.9, 0.4], [-0.7, 0.1, 0.6])):
        cases["exact %d" % i] = _cloud_on_plane(i, 500, normal, [0.3, -0.2, 0.1], 0.0)
        cases["noisy %d" % i] = _cloud_on_plane(10 + i, 500, normal, [0.3, -0.2, 0.1], 2e-3)
        cases["far %d" % i] = _cloud_on_plane(20 + i, 500, normal, far, 2e-3)
    cases["three points"] = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], np.float64)
    return cases


def _moments(p, origin):
    q = p - origin
    qq = np.stack([q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]], 1)
    return np.concatenate([[p.shape[0]], q.sum(0), qq.sum(0), [0.0]])


def test_fit_agrees_with_eigh(sg_lib):
    from seggroup_amd import planes
    worst_n = worst_d = worst_d_near = 0.0
    for name, p in fit_cases().items():
        origin = 0.5 * (p.min(0) + p.max(0))
        m = _moments(p, origin)
        got, centroid, rms = planes.plane_fit(m, origin)
        want, want_c, want_rms = PR.fit(m, origin)
        assert abs(np.linalg.norm(got[:3]) - 1.0) <= 4 * 2.0 ** -52, name
        assert got[int(np.argmax(np.abs(got[:3])))] > 0, name
        dn, dd = float(np.abs(got[:3] - want[:3]).max()), abs(got[3] - want[3])
        worst_n, worst_d = max(worst_n, dn), max(worst_d, dd)
        if not name.startswith("far"):
            worst_d_near = max(worst_d_near, dd)
        assert dn <= NORMAL_BOUND and dd <= OFFSET_BOUND, (name, dn, dd)
        assert np.array_equal(centroid, want_c), name
        # both solvers give an eigenvalue to a few units of the last place of the LARGEST one: that, not the value itself, is the scale
        assert abs(rms * rms - want_rms * want_rms) <= 64 * 2.0 ** -52 * (m[4] + m[7] + m[9]) / m[0], (name, rms, want_rms)
        if name.startswith("exact"):
            assert rms < 1e-7 and np.abs(p @ got[:3] + got[3]).max() < 1e-12 * max(1.0, np.abs(p).max()), name
    print("plane_fit against eigh: normal %.3g, offset %.3g (%.3g at the origin)" % (worst_n, worst_d, worst_d_near))


def test_fit_sign_rule(sg_lib):
    """the normal's largest-magnitude component is positive, whichever way the points were generated"""
    from seggroup_amd import planes
    for normal, big in (([-2, 1, 0.5], 0), ([2, -1, -0.5], 0), ([0.1, -3, 1], 1), ([0.5, 0.5, -4], 2), ([0, 0, -1], 2)):
        p = _cloud_on_plane(5, 200, normal, [0.5, 0.25, -1.0], 1e-3)
        got, centroid, _ = planes.plane_fit(_moments(p, np.zeros(3)))
        assert int(np.argmax(np.abs(got[:3]))) == big and got[big] > 0, (normal, got)
        assert abs(got[:3] @ centroid + got[3]) < 1e-15 and np.allclose(centroid, p.mean(0), atol=1e-14)


def test_fit_refuses_what_has_no_plane(sg_lib):
    from seggroup_amd import hip, planes
    t = np.linspace(-1, 1, 50)[:, None]
    line = np.array([0.5, -0.25, 2.0]) + t * np.array([0.3, 0.4, -0.5])
    for name, p in (("two points", np.array([[0, 0, 0], [1, 2, 3]], np.float64)), ("no point", np.zeros((0, 3))), ("a line", line),
                    ("a far line", line + 1000.0), ("one place", np.tile([[1.0, 2.0, 3.0]], (9, 1)))):
        origin = 0.5 * (p.min(0) + p.max(0)) if p.shape[0] else np.zeros(3)
        with pytest.raises(hip.SgError, match="degenerate") as e:
            planes.plane_fit(_moments(p, origin), origin)
        assert e.value.code == hip.SG_EUNSUP, name
        with pytest.raises(PR.Degenerate):
            PR.fit(_moments(p, origin), origin)
    good = _moments(fit_cases()["noisy 2"], np.zeros(3))
    for slot in (0, 2, 7, 10):
        for bad in (np.nan, np.inf):
            m = good.copy()
            m[slot] = bad
            with pytest.raises(ValueError):
                planes.plane_fit(m)
    with pytest.raises(ValueError):
        planes.plane_fit(good, [np.nan, 0, 0])
    with pytest.raises(ValueError):
        planes.plane_fit(good[:10])


def _planes_of(rows, centroids, points):
    from seggroup_amd import planes
    p = len(rows)
    return planes.Planes(labels=np.zeros(0, np.int32), planes=np.array(rows, np.float64).reshape(p, 4), points=np.array(points, np.int64),
                         ransac_count=np.array(points, np.int64), h=np.zeros(p, np.int64), rms=np.zeros(p), centroid=np.array(centroids, np.float64),
                         dist=0.01, max_planes=16, min_points=3, hypotheses=64, seed=0, min_edge=0.1, min_sine=0.1)


def test_level_transform_on_the_fixture_and_by_hand():
    from seggroup_amd import planes
    xyz, P = PR.fixture()
    d = PR.fixture_reference()
    found = _planes_of(d.planes, d.centroid, d.points)
    T = planes.level_transform(found, xyz)
    assert T.dtype == np.float64 and T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1])
    R = T[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 8 * 2.0 ** -52 and np.linalg.det(R) > 0
    assert np.abs(T - PR.level_transform(d.planes, d.centroid, d.points, xyz)).max() < 1e-14
    floor = PR.face_corners(P)[0] @ R.T + T[:3, 3]
    moved = A.apply(xyz, T).astype(np.float64)
    assert np.abs(floor[:, 2]).max() <= PR.PARAMS["dist"]
    assert moved[d.labels != 0, 2].min() > 0.0 and np.abs(moved[d.labels == 0, 2]).max() <= PR.PARAMS["dist"] + 1e-6
    c = d.centroid[0]
    assert np.allclose(R @ c + T[:3, 3], [c[0], c[1], 0.0], atol=1e-14)   # the centroid keeps x and y and lands at z = 0
    # by index, and the refusals
    T3 = planes.level_transform(found, xyz, 3)
    top = PR.face_corners(P)[3] @ T3[:3, :3].T + T3[:3, 3]
    assert np.abs(top[:, 2]).max() <= PR.PARAMS["dist"]
    for bad in (6, -1, "floor", True):
        with pytest.raises(ValueError, match="which"):
            planes.level_transform(found, xyz, bad)
    with pytest.raises(ValueError, match="no plane"):
        planes.level_transform(_planes_of([], np.zeros((0, 3)), []), xyz)
    # a ceiling: the normal +z is stored, the cloud hangs below it, so the normal is turned and the half turn about x applies
    cloud = np.array([[0, 0, 2.0], [1, 0, 2.0], [0, 1, 2.0], [0.5, 0.5, 1.0], [0.2, 0.7, 0.5]])
    up = _planes_of([[0, 0, 1, -2.0]], [[1.0 / 3, 1.0 / 3, 2.0]], [3])
    Th = planes.level_transform(up, cloud)
    assert np.array_equal(Th[:3, :3], np.diag([1.0, -1.0, -1.0]))
    out = cloud @ Th[:3, :3].T + Th[:3, 3]
    assert np.abs(out[:3, 2]).max() == 0.0 and (out[3:, 2] > 0).all()
    # ... and the same plane under a floor is left where it is (the identity), up to the shift to z = 0
    below = cloud * [1, 1, -1] + [0, 0, 4.0]
    Ti = planes.level_transform(up, below)
    assert np.array_equal(Ti[:3, :3], np.eye(3)) and np.array_equal(Ti[:3, 3], [0, 0, -2.0])


def test_what_is_refused_before_a_device_call(tmp_path):
    from seggroup_amd import planes
    cloud = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="min_points"):
        planes.detect_planes(cloud, 0.01)
    for kw in (dict(dist=0.0), dict(dist=float("nan")), dict(min_points=2), dict(max_planes=0), dict(hypotheses=0), dict(hypotheses=2 ** 20 + 1),
               dict(min_edge=0.0), dict(min_sine=0.0), dict(min_sine=1.5), dict(normal_angle=100.0), dict(normal_angle=10.0),
               dict(normals=np.zeros((10, 3), np.float32))):
        with pytest.raises(ValueError, match="detect_planes"):
            planes.detect_planes(cloud, **dict(dict(dist=0.01, min_points=5), **kw))
    argv = ["--scans", str(tmp_path), "--out", str(tmp_path / "out")]
    for extra in (["--dist", "0.01"], ["--min-points", "40"], ["--dist", "0.01", "--min-points", "40", "--level", "--remove"],
                  ["--dist", "0.01", "--min-points", "40", "--level", "2", "--remove"], ["--dist", "0", "--min-points", "40"],
                  ["--dist", "0.01", "--min-points", "2"], ["--dist", "0.01", "--min-points", "40", "--normals-k", "10"],
                  ["--dist", "0.01", "--min-points", "40", "--normal-angle", "20", "--normals-k", "2"],
                  ["--dist", "0.01", "--min-points", "40", "--hypotheses", "2000000"], ["--dist", "0.01", "--min-points", "40", "--level", "walls"],
                  ["--dist", "0.01", "--min-points", "40", "--level", "-1"], ["--dist", "0.01", "--min-points", "40", "--max-planes", "0"],
                  ["--dist", "0.01", "--min-points", "40", "--workers", "99"]):
        with pytest.raises(SystemExit) as e:
            planes.main(argv + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "out").exists()
