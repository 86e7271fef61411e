"""Boxes of labelled points without a GPU: tests/boxes_ref.py on hand cases, sg_box_axes (host) against numpy.linalg.eigh,
Boxes.corners, and everything seggroup_amd/boxes.py and its command refuse before a device call."""
import math

import numpy as np
import pytest

import boxes_ref as BR

# sg_box_axes against numpy.linalg.eigh over axes_cases(), measured on the CPU: the rows of R differ by at most
# AXES_MEASURED in any component, the eigenvalues by at most EIG_MEASURED of the largest one.  The gates are 16 times the measurement.
AXES_MEASURED = 4.45e-16
EIG_MEASURED = 3.83e-16
AXES_BOUND = 16 * AXES_MEASURED
EIG_BOUND = 16 * EIG_MEASURED
# what rounding a coordinate below 4 m to float32 can move it by (half a unit of 2^-22), twice: the two ends of an extent; the double
# arithmetic behind it is 2^-29 of that
SIDE_ROUNDING = 2 * math.sqrt(2.0) * 2.0 ** -23 * (1 + 2.0 ** -20)


def test_label_index_by_hand():
    order, values, start, ignored = BR.label_index([5, -1, 2, 5, 2 ** 31 - 1, -7, 2, 5])
    assert order.tolist() == [2, 6, 0, 3, 7, 4] and values.tolist() == [2, 5, 2 ** 31 - 1] and start.tolist() == [0, 2, 5, 6] and ignored == 2
    order, values, start, ignored = BR.label_index(np.full(4, -3))
    assert order.size == 0 and values.size == 0 and start.tolist() == [0] and ignored == 4
    order, values, start, ignored = BR.label_index(np.zeros(0, np.int32))
    assert order.size == 0 and start.tolist() == [0] and ignored == 0


def test_moments_and_extents_by_hand():
    xyz = np.array([[1, 2, 3], [9, 9, 9], [2, 4, 3], [np.nan, 0, 0], [0, 2, 5]], np.float32)
    labels = [7, 1, 7, -1, 7]
    order, values, start, _ = BR.label_index(labels)
    m, mag, lo, hi = BR.moments(xyz, order, start)
    assert values.tolist() == [1, 7]
    assert m[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]                # one point: q = 0
    # label 7: q = (0,0,0), (1,2,0), (-1,0,2)
    assert m[1].tolist() == [3, 0, 2, 2, 2, 2, -2, 4, 0, 4] and mag[1].tolist() == [3, 2, 2, 2, 2, 2, 2, 4, 0, 4]
    assert lo.tolist() == [[9, 9, 9], [0, 2, 3]] and hi.tolist() == [[9, 9, 9], [2, 4, 5]] and lo.dtype == np.float32
    best, ext, every = BR.yaw_boxes(xyz, order, start, np.array([[1.0, 0.0], [0.0, 1.0]]))
    assert best.tolist() == [0, 0] and ext[1].tolist() == [0, 2, 2, 4] and every[1, 1].tolist() == [2, 4, -2, 0]
    fr = BR.frame_extents(xyz, order, start, np.array([np.eye(3), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]]))
    assert fr[0].tolist() == [9, 9, 9, 9, 9, 9] and fr[1].tolist() == [3, 5, 2, 4, -2, 0]


def test_the_restatement_on_a_turned_lattice_cuboid():
    """3 x 2 x 1 on a quarter-metre lattice: at 0 degrees exactly, at 30 degrees (on the 1-degree sweep) to float32 rounding of the
    coordinates, at 30.5 (half a step) inside the bound that half a step allows"""
    a = 90
    eps = (math.pi / 2) / (2 * a)
    for deg in (0.0, 30.0, 30.5):
        p = BR.lattice_cuboid(angle=math.radians(deg))
        b = BR.label_boxes(p, np.full(p.shape[0], 4), "yaw", a)
        assert b["values"].tolist() == [4] and b["count"].tolist() == [p.shape[0]] == [13 * 9 * 5]
        w, h, d = b["size"][0]
        step = round(b["yaw"][0] / ((math.pi / 2) / a))
        assert b["yaw"][0] == step * ((math.pi / 2) / a)                  # on the sweep's grid
        if deg == 0.0:
            assert (w, h, d) == (3.0, 2.0, 1.0) and step == 0 and b["center"][0].tolist() == [1.5, 1.0, 0.5]
            assert np.array_equal(b["R"][0], np.eye(3))
        elif deg == 30.0:
            assert step == 30 and abs(w - 3.0) <= SIDE_ROUNDING and abs(h - 2.0) <= SIDE_ROUNDING and d == 1.0
            c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
            assert np.abs(b["center"][0] - [c * 1.5 - s * 1.0, s * 1.5 + c * 1.0, 0.5]).max() <= SIDE_ROUNDING
        else:
            assert step in (30, 31)
            assert 3.0 - SIDE_ROUNDING <= w <= 3.0 * math.cos(eps) + 2.0 * math.sin(eps) + SIDE_ROUNDING
            assert 2.0 - SIDE_ROUNDING <= h <= 2.0 * math.cos(eps) + 3.0 * math.sin(eps) + SIDE_ROUNDING
        # every point lies inside the box's corners
        cn = BR.corners(b["center"], b["size"], b["R"])[0]
        local = (p.astype(np.float64) - b["center"][0]) @ b["R"][0].T
        assert (np.abs(local) <= 0.5 * b["size"][0] + 1e-12).all()
        assert np.abs((cn - b["center"][0]) @ b["R"][0].T).max() <= 0.5 * max(w, h, d) + 1e-12
    # aabb of the turned cuboid is larger; a square footprint turned by 45 degrees comes back square
    p = BR.lattice_cuboid(2.0, 2.0, 1.0, angle=math.radians(45.0))
    b = BR.label_boxes(p, np.zeros(p.shape[0], np.int64), "yaw", 90)
    assert b["yaw"][0] == 45 * ((math.pi / 2) / 90) and np.abs(b["size"][0] - [2, 2, 1]).max() <= SIDE_ROUNDING
    assert BR.label_boxes(p, np.zeros(p.shape[0], np.int64), "aabb")["size"][0][0] > 2.8


def axes_cases():
    """name -> float32 cloud: exact and noisy cuboids, turned, at the origin and 1,000 m away"""
    out = {}
    for where, origin in (("origin", (0.0, 0.0, 0.0)), ("far", (600.0, -500.0, 620.0))):
        out["exact_" + where] = BR.lattice_cuboid(origin=origin)
        out["exact_turned_" + where] = BR.lattice_cuboid(angle=0.5, origin=origin)
        out["noisy_" + where] = BR.lattice_cuboid(angle=1.1, origin=origin, noise=0.01, seed=3)
        out["noisy_flat_" + where] = BR.lattice_cuboid(2.0, 1.0, 0.0, angle=0.3, origin=origin, noise=0.002, seed=4)
    return out


def _moments_of(p):
    order, _, start, _ = BR.label_index(np.zeros(p.shape[0], np.int32))
    return BR.moments(p, order, start)[0][0]


def test_box_axes_agrees_with_eigh(sg_lib):
    from seggroup_amd import boxes
    worst_r = worst_e = 0.0
    for name, p in axes_cases().items():
        m = _moments_of(p)
        R, eig = boxes.box_axes(m)
        want_R, want_e = BR.box_axes(m)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * 2.0 ** -52 and np.linalg.det(R) > 0.999999, name
        for r in range(2):
            assert R[r, int(np.argmax(np.abs(R[r])))] > 0, name
        assert eig[0] >= eig[1] >= eig[2], name
        dr, de = float(np.abs(R - want_R).max()), float(np.abs(eig - want_e).max() / want_e[0])
        print("box_axes %-22s R %.3g eig %.3g" % (name, dr, de))
        worst_r, worst_e = max(worst_r, dr), max(worst_e, de)
    print("box_axes against eigh: rows %.3g, eigenvalues %.3g of the largest" % (worst_r, worst_e))
    assert worst_r <= AXES_BOUND and worst_e <= EIG_BOUND, (worst_r, worst_e)
    # the exact cuboid at the origin: the axes are the world's, longest first
    R, eig = boxes.box_axes(_moments_of(BR.lattice_cuboid()))
    assert np.array_equal(R, np.eye(3)) and eig[0] > eig[1] > eig[2] > 0


def test_box_axes_degenerate_and_refused(sg_lib):
    from seggroup_amd import boxes
    one = np.array([1.0] + [0.0] * 9)
    R, eig = boxes.box_axes(one)
    assert np.array_equal(R, np.eye(3)) and not eig.any()
    same = _moments_of(np.tile(np.array([[3.0, 4.0, 5.0]], np.float32), (7, 1)))
    assert np.array_equal(boxes.box_axes(same)[0], np.eye(3))
    # a cube: three equal eigenvalues, nothing to rotate, the identity
    cube = _moments_of(BR.lattice_cuboid(1.0, 1.0, 1.0))
    assert np.array_equal(boxes.box_axes(cube)[0], np.eye(3))
    # the sign rule, whichever way the points run: a line along (-1, -1, 0)
    t = np.linspace(0, 1, 20)[:, None]
    line = _moments_of((t * np.array([[-1.0, -1.0, 0.0]])).astype(np.float32))
    R, _ = boxes.box_axes(line)
    assert R[0, 0] > 0.7 and R[0, 1] > 0.7 and abs(R[0, 2]) < 1e-12
    for bad in (np.zeros(10), np.array([np.nan] + [0.0] * 9), np.array([-1.0] + [0.0] * 9), np.array([2.0, np.inf] + [0.0] * 8)):
        with pytest.raises(ValueError):
            boxes.box_axes(bad)
    with pytest.raises(ValueError, match="10 moments"):
        boxes.box_axes(np.zeros(11))


def test_corners():
    from seggroup_amd import boxes
    c, s = math.cos(0.3), math.sin(0.3)
    R = np.array([np.eye(3), [[c, s, 0], [-s, c, 0], [0, 0, 1]]])
    center = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
    size = np.array([[2.0, 4.0, 6.0], [1.0, 0.5, 0.25]])
    z = np.zeros((2, 3))
    b = boxes.Boxes(values=np.array([1, 2], np.int32), count=np.array([5, 6]), first=np.array([0, 1], np.int32), lo=z.astype(np.float32),
                    hi=z.astype(np.float32), centroid=z, cov=np.zeros((2, 6)), R=R, center=center, size=size, yaw=np.array([0.0, 0.3]), kind="yaw",
                    angles=90, min_points=1)
    got = b.corners()
    assert got.shape == (2, 8, 3) and np.abs(got - BR.corners(center, size, R)).max() <= 4 * 2.0 ** -52 * 8
    assert got[0, 0].tolist() == [0.0, 0.0, 0.0] and got[0, 7].tolist() == [2.0, 4.0, 6.0] and got[0, 1].tolist() == [2.0, 0.0, 0.0]
    local = (got[1] - center[1]) @ R[1].T
    assert np.abs(np.abs(local) - 0.5 * size[1]).max() <= 1e-15
    assert np.abs(got.mean(1) - center).max() <= 1e-15
    assert set(b.arrays()) == {"values", "count", "first", "lo", "hi", "centroid", "cov", "R", "center", "size", "yaw", "kind", "angles", "min_points"}
    xyz, rgb, faces = boxes.box_mesh(b)
    assert xyz.shape == (16, 3) and rgb.shape == (16, 3) and rgb.dtype == np.uint8 and faces.shape == (24, 3) and faces.max() == 15
    assert faces[:12].max() == 7 and faces[12:].min() == 8
    # every triangle of a box faces outwards
    for k in range(2):
        tri = xyz[faces[12 * k:12 * k + 12]].astype(np.float64)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert (np.einsum("ij,ij->i", nrm, tri.mean(1) - center[k]) > 0).all()
    rows = boxes.detector_rows(b, [3, 5])
    assert rows.shape == (2, 7) and rows.dtype == np.float64 and rows[:, 6].tolist() == [3.0, 5.0]


def test_what_is_refused_before_a_device_call(tmp_path):
    """on a machine without a GPU a device call is a RuntimeError: every refusal below is a ValueError (or the parser's exit) before it"""
    from seggroup_amd import boxes
    cloud = np.zeros((10, 3), np.float32)
    lab = np.zeros(10, np.int32)
    for kw, match in ((dict(labels=np.zeros(9, np.int32)), "labels must be"), (dict(labels=np.zeros((10, 1), np.int32)), "labels must be"),
                      (dict(xyz=np.zeros((10, 2), np.float32)), "cloud"), (dict(angles=0), "angles"), (dict(angles=1025), "angles"),
                      (dict(angles=2.5), "angles"), (dict(kind="obb"), "kind"), (dict(kind="aabb", angles=90), "angles"),
                      (dict(kind="pca", angles=4), "angles"), (dict(min_points=0), "min_points")):
        args = dict(xyz=cloud, labels=lab)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            boxes.label_boxes(**args)
    with pytest.raises(ValueError, match="angles"):
        boxes.yaw_boxes(cloud, None, angles=0)
    with pytest.raises(ValueError, match="cs"):
        boxes.yaw_boxes(cloud, None, cs=np.array([[1.0, np.nan]]))
    base = ["--scans", str(tmp_path / "scans"), "--out", str(tmp_path / "out")]
    exp = base + ["-n", "e", "--stage", "s"]
    frm = base + ["--labels-from", str(tmp_path), "--suffix", ".planes.npz", "--key", "labels", "--min-points", "5"]
    for argv in (base,                                                        # no source of labels
                 exp + ["--labels-from", str(tmp_path), "--suffix", ".npy"],  # both
                 exp + ["--key", "labels"], exp + ["--suffix", ".npy"],
                 exp + ["--kind", "obb"], exp + ["--angles", "0"], exp + ["--angles", "1025"], exp + ["--kind", "aabb", "--angles", "90"],
                 exp + ["--min-points", "0"], exp + ["--classes", "nyu40"], exp + ["--workers", "0"],
                 base + ["--labels-from", str(tmp_path), "--suffix", ".planes.npz", "--key", "labels"],                # --min-points has no default
                 base + ["--labels-from", str(tmp_path), "--min-points", "5"],                                         # no --suffix
                 base + ["--labels-from", str(tmp_path), "--suffix", ".planes.npz", "--min-points", "5"],              # an .npz without --key
                 base + ["--labels-from", str(tmp_path), "--suffix", ".comp.npy", "--key", "a", "--min-points", "5"],  # a .npy with --key
                 base + ["--labels-from", str(tmp_path), "--suffix", ".txt", "--min-points", "5"],
                 frm + ["--classes", "all"], frm + ["--classes", "scannet18"], frm + ["--detector-files"], frm + ["--stage", "s"],
                 frm + ["--layer", "final"]):
        with pytest.raises(SystemExit) as e:
            boxes.main(argv)
        assert e.value.code == 2, argv
    assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="--min-points"):                       # the message names the parameter
        boxes.check_command(None, "d", ".npy", None, "yaw", None, None, None, False)
    assert boxes.check_command("e", None, None, None, "yaw", None, None, None, True) == ("yaw", 90, 100, "scannet18")
    assert boxes.check_command(None, "d", ".npy", None, "pca", None, 7, None, False) == ("pca", 0, 7, None)
