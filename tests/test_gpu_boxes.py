"""Boxes of labelled points on the GPU (seggroup_amd/boxes.py) against tests/boxes_ref.py: the label index, the minima and
maxima, the yaw sweep and the frame extents EQUAL, the ten sums inside sg_align_moments' gate and the same bytes on every call; the
geometry of a turned cuboid, the project's room, and the command on both of its routes."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import boxes_ref as BR
import pcseg_ref as R
import register_ref as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
ANGLES = (1, 63, 64, 65, 90, 256)
PATTERNS = ("one", "own", "negative", "sparse", "interleaved")
# A lattice cuboid 3 x 2 (x 1) turned by an angle ON the sweep's grid: how far the recovered sides are from 3 and 2, measured with the
# restatement on the CPU over _grid_cases() (the device equals the restatement): 1.85e-7 -- the float32 rounding of the turned
# coordinates, at most half a unit of 2^-22 below 4 m, on either end of a side.  The gate is 16 times the measurement.
SIDE_MEASURED = 1.85e-7
SIDE_BOUND = 16 * SIDE_MEASURED
PCA_BOUND = 4.2e-5


def _rows(xyz, stride):
    return xyz if stride == 3 else np.ascontiguousarray(np.concatenate([xyz, np.full((xyz.shape[0], stride - 3), 7.0, np.float32)], 1))


def _cloud(seed, n, offset=0.0):
    p = np.random.RandomState(seed).rand(n, 3) * 2.0 + offset * np.array([0.6, -0.5, 0.62])
    return p.astype(np.float32)


def _labels(pattern, n, seed=0):
    rng = np.random.RandomState(seed + 17)
    i = np.arange(n)
    if pattern == "one":
        return np.full(n, 3, np.int32)
    if pattern == "own":
        return (rng.permutation(n) * 7 + 1).astype(np.int32)
    if pattern == "negative":
        return (-1 - (i % 3)).astype(np.int32)
    if pattern == "sparse":
        return rng.choice(np.array([0, 5, 2 ** 31 - 1, 10 ** 6, -1, -2 ** 31, 2 ** 30], np.int64), n).astype(np.int32)
    if pattern == "interleaved":
        return (i % 3).astype(np.int32)
    raise KeyError(pattern)


def _frames(l, seed):
    """a turned orthonormal frame per label (any 3 x 3 doubles would do)"""
    q = np.linalg.qr(np.random.RandomState(seed).standard_normal((max(l, 1), 3, 3)))[0]
    return np.ascontiguousarray(q[:l])


def _index(labels, **kw):
    from seggroup_amd import boxes
    idx = boxes.label_index(labels, device=DEV, **kw)
    want = BR.label_index(labels)
    got = (idx.order.cpu().numpy(), idx.values.cpu().numpy(), idx.start.cpu().numpy(), idx.ignored)
    for g, w, name in zip(got[:3], want[:3], ("order", "values", "start")):
        assert g.dtype == np.int32 and np.array_equal(g, w), name
    assert got[3] == want[3]
    return idx, want


def _check(xyz, labels, angles, stride=3, what=""):
    """index, moments, sweep and frame extents of one cloud against the restatement -> the device's results as arrays"""
    from seggroup_amd import boxes
    idx, (order, values, start, ignored) = _index(labels)
    rows = _rows(xyz, stride)
    mom = boxes.label_moments(rows, idx, device=DEV)
    m, lo, hi = mom.moments.cpu().numpy(), mom.lo.cpu().numpy(), mom.hi.cpu().numpy()
    want_m, mag, want_lo, want_hi = BR.moments(xyz, order, start)
    l = values.size
    assert m.shape == (l, 10) and m.dtype == np.float64 and lo.shape == (l, 3) and lo.dtype == np.float32, what
    assert np.array_equal(m[:, 0], np.diff(start)), what
    assert lo.tobytes() == want_lo.tobytes() and hi.tobytes() == want_hi.tobytes(), what
    bound = np.maximum(m[:, 0:1], 1.0) * 2.0 ** -52 * mag
    assert (np.abs(m - want_m) <= bound).all(), (what, float((np.abs(m - want_m) / np.maximum(bound, 1e-300)).max()))
    out = dict(m=m, lo=lo, hi=hi)
    for a in angles:
        cs = BR.angle_table(a)
        best, ext, every = boxes.yaw_boxes(rows, idx, a, all_extents=True, device=DEV)
        best, ext, every = best.cpu().numpy(), ext.cpu().numpy(), every.cpu().numpy()
        wb, we, wa = BR.yaw_boxes(xyz, order, start, cs)
        assert best.dtype == np.int32 and np.array_equal(best, wb), (what, a)
        assert np.array_equal(ext, we) and np.array_equal(every, wa), (what, a)
        plain = boxes.yaw_boxes(rows, idx, a, device=DEV)
        assert plain[2] is None and np.array_equal(plain[0].cpu().numpy(), wb) and np.array_equal(plain[1].cpu().numpy(), we), (what, a)
        out[a] = (best, ext)
    fr = _frames(l, 5 + l)
    got = boxes.frame_extents(rows, idx, fr, device=DEV).cpu().numpy()
    assert got.shape == (l, 6) and np.array_equal(got, BR.frame_extents(xyz, order, start, fr)), what
    return out


@pytest.mark.parametrize("n", SIZES)
def test_index_and_reductions_against_the_restatement(n):
    """every pattern at every size; all six sweep widths on two of the patterns, two of them (rotating) on the rest.  Odd sizes run on
    rows of six floats."""
    xyz = _cloud(n, n)
    for k, pattern in enumerate(PATTERNS):
        angles = ANGLES if pattern in ("one", "interleaved") else (ANGLES[(k + n) % 6], ANGLES[(k + n + 3) % 6])
        _check(xyz, _labels(pattern, n, n), angles, 6 if n % 2 else 3, "%s N %d" % (pattern, n))


def test_the_chunk_edge_and_a_long_label_beside_short_ones():
    """a label of exactly 1,024 points is one chunk and one of 1,025 is two; 3,000 points are three chunks beside fifty labels of one
    chunk each"""
    rng = np.random.RandomState(8)
    lab = rng.permutation(np.concatenate([np.full(1024, 11), np.full(1025, 4), np.full(10, -1)])).astype(np.int32)
    xyz = _cloud(81, lab.size)
    out = _check(xyz, lab, (1, 65, 90), what="chunk edge")
    assert out["m"][:, 0].tolist() == [1025, 1024]
    small = np.concatenate([np.full(1 + (k * 7) % 40, 100 + k) for k in range(50)])
    lab = rng.permutation(np.concatenate([np.full(3000, 7), small])).astype(np.int32)
    xyz = _cloud(82, lab.size)
    out = _check(xyz, lab, (64, 90, 256), stride=6, what="3000 + fifty")
    assert out["m"][0, 0] == 3000 and out["m"].shape[0] == 51 and 1 <= out["m"][1:, 0].min() and out["m"][1:, 0].max() <= 40


@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["origin", "1000m"])
def test_sums_are_deterministic_and_independent_of_where_the_cloud_lies(offset):
    """the same bytes on repeated calls and on another stream; every output the same; the sums conditioned on the label's own first point"""
    import torch
    from seggroup_amd import boxes
    n = 4500
    xyz = _cloud(31, n, offset)
    lab = np.where(np.arange(n) % 11 == 0, -1, np.minimum(np.arange(n) % 5, 3)).astype(np.int32)       # label 3: 1,636 points, two chunks
    first = _check(xyz, lab, (90,), what="offset %g" % offset)
    side = torch.cuda.Stream(device=DEV)
    for stride, stream in ((3, None), (6, side), (3, side)):
        idx = boxes.label_index(lab, device=DEV, stream=stream)
        mom = boxes.label_moments(_rows(xyz, stride), idx, device=DEV, stream=stream)
        assert mom.moments.cpu().numpy().tobytes() == first["m"].tobytes(), (stride, stream)
        assert mom.lo.cpu().numpy().tobytes() == first["lo"].tobytes() and mom.hi.cpu().numpy().tobytes() == first["hi"].tobytes()
        best, ext, _ = boxes.yaw_boxes(_rows(xyz, stride), idx, 90, device=DEV, stream=stream)
        assert best.cpu().numpy().tobytes() == first[90][0].tobytes() and ext.cpu().numpy().tobytes() == first[90][1].tobytes()
    # the second central moments stay at the cloud's own scale: sum q q^T of a 2 m box is at most 4 per point, wherever it lies
    assert (np.abs(first["m"][:, 4:]) <= 4.0 * first["m"][:, 0:1] * (1 + 1e-3)).all()


def test_a_nan_is_refused_only_where_it_is_labelled():
    from seggroup_amd import boxes
    n = 3000
    xyz = _cloud(41, n)
    lab = _labels("interleaved", n)
    lab[[5, 1500]] = -4
    bad = xyz.copy()
    bad[5] = np.nan
    bad[1500, 1] = np.inf
    want = _check(xyz, lab, (90,), what="clean")
    idx = boxes.label_index(lab, device=DEV)
    mom = boxes.label_moments(bad, idx, device=DEV)                           # ignored points may hold anything
    assert mom.moments.cpu().numpy().tobytes() == want["m"].tobytes()
    assert np.array_equal(boxes.yaw_boxes(bad, idx, 90, device=DEV)[1].cpu().numpy(), want[90][1])
    b = boxes.label_boxes(bad, lab, "pca", device=DEV)
    assert np.isfinite(b.center).all() and b.count.sum() == n - 2
    for where, value in ((6, np.nan), (2999, np.inf), (1024, -np.inf)):
        worse = bad.copy()
        worse[where, where % 3] = value
        fr = _frames(3, 1)
        for call in (lambda: boxes.label_moments(worse, idx, device=DEV), lambda: boxes.yaw_boxes(worse, idx, 64, device=DEV),
                     lambda: boxes.frame_extents(worse, idx, fr, device=DEV), lambda: boxes.label_boxes(worse, lab, device=DEV)):
            with pytest.raises(ValueError, match="not finite"):
                call()
    again = boxes.label_moments(xyz, idx, device=DEV)                         # and the call after a refusal is unharmed
    assert again.moments.cpu().numpy().tobytes() == want["m"].tobytes()
    # an index of another cloud, an offset table that is not one
    with pytest.raises(ValueError, match="index"):
        boxes.label_moments(xyz[:100], idx, device=DEV)
    broken = boxes.LabelIndex(idx.order, idx.values, idx.start.flip(0).contiguous(), idx.ignored)
    with pytest.raises(ValueError, match="label index"):
        boxes.label_moments(xyz, broken, device=DEV)


def test_ties_go_to_the_first_angle():
    from seggroup_amd import boxes
    side = np.arange(0.0, 1.01, 0.125)
    square = np.stack(np.meshgrid(side, side, [0.0, 0.5], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    xyz = np.concatenate([square, [[0.3, 0.7, 0.2]], square + np.float32(4.0)]).astype(np.float32)
    lab = np.concatenate([np.full(square.shape[0], 2), [9], np.full(square.shape[0], 5)]).astype(np.int32)
    for a in ANGLES:
        b = boxes.label_boxes(xyz, lab, "yaw", a, device=DEV)
        assert b.values.tolist() == [2, 5, 9] and not b.yaw.any(), a
        assert np.array_equal(b.R, np.tile(np.eye(3), (3, 1, 1)))
        assert b.size.tolist() == [[1.0, 1.0, 0.5], [1.0, 1.0, 0.5], [0.0, 0.0, 0.0]]
        assert b.center.tolist() == [[0.5, 0.5, 0.25], [4.5, 4.5, 4.25], [float(np.float32(0.3)), float(np.float32(0.7)), float(np.float32(0.2))]]
        assert b.first.tolist() == [0, square.shape[0] + 1, square.shape[0]] and b.count.tolist() == [162, 162, 1]


def test_all_extents_has_a_size_limit_and_the_widest_sweep_runs():
    """[L,A,4] above 2^24 rows is refused (SG_EUNSUP); the same call without it runs A = 1,024, sixteen turns of the angle loop"""
    from seggroup_amd import boxes, hip
    n = 20000
    xyz = _cloud(51, n)
    idx = boxes.label_index(np.arange(n, dtype=np.int32), device=DEV)
    with pytest.raises(hip.SgError) as e:
        boxes.yaw_boxes(xyz, idx, 1024, all_extents=True, device=DEV)
    assert e.value.code == hip.SG_EUNSUP
    best, ext, every = boxes.yaw_boxes(xyz, idx, 1024, device=DEV)
    assert every is None and not best.cpu().numpy().any()                    # a single point: every area is 0, the first angle wins
    assert np.array_equal(ext.cpu().numpy(), xyz[:, [0, 0, 1, 1]].astype(np.float64))
    few = xyz[:3000]                                                          # one label of three chunks
    one = boxes.label_index(np.zeros(3000, np.int32), device=DEV)
    wb, we, _ = BR.yaw_boxes(few, *BR.label_index(np.zeros(3000, np.int32))[0:3:2], BR.angle_table(1024))
    best, ext, _ = boxes.yaw_boxes(few, one, 1024, device=DEV)
    assert np.array_equal(best.cpu().numpy(), wb) and np.array_equal(ext.cpu().numpy(), we)


def test_stage_timer_times_every_entry():
    """hip.stage_timer("label") around one call of each entry point: the same bytes as untimed and four finite times above 0; after the
    block an untimed call leaves the record as it was"""
    from seggroup_amd import boxes, hip
    xyz, lab = _cloud(5, 1025), _labels("interleaved", 1025)
    frames = _frames(3, 1)

    def calls():
        idx = boxes.label_index(lab, device=DEV)
        mom = boxes.label_moments(xyz, idx, device=DEV)
        best, ext, _ = boxes.yaw_boxes(xyz, idx, 63, device=DEV)
        fr = boxes.frame_extents(xyz, idx, frames, device=DEV)
        return [v.cpu().numpy().tobytes() for v in (idx.order, idx.values, idx.start, mom.moments, mom.lo, mom.hi, best, ext, fr)]

    plain = calls()
    with hip.stage_timer("label") as t:
        assert t.names == ["index", "moments", "yaw", "frame"]
        assert calls() == plain
        last = t.read()
        assert len(last) == len(t.names) and all(np.isfinite(u) and u > 0.0 for u in last), last
    assert calls() == plain
    assert t.read() == last


def _grid_cases():
    """(A, step a, cloud): 3 x 2 x 1 lattice cuboids turned by a * (pi/2)/A, two of them in one cloud with a third label on a half step"""
    for a_count, steps in ((90, (0, 1, 30, 45, 89)), (64, (7, 33)), (256, (100, 255)), (65, (13,))):
        for a in steps:
            yield a_count, a, BR.lattice_cuboid(angle=a * ((math.pi / 2) / a_count), origin=(0.5, -1.0, 0.25))


def test_a_turned_cuboid_comes_back():
    from seggroup_amd import boxes
    worst = 0.0
    for a_count, a, p in _grid_cases():
        eps = (math.pi / 2) / (2 * a_count)
        ha = a if a + 1 < a_count else a - 1                                # the half step stays inside the quarter turn
        half = BR.lattice_cuboid(angle=(ha + 0.5) * ((math.pi / 2) / a_count), origin=(-6.0, 3.0, 0.0))
        xyz = np.concatenate([p, half])
        lab = np.concatenate([np.full(p.shape[0], 1), np.full(half.shape[0], 0)]).astype(np.int32)
        b = boxes.label_boxes(xyz, lab, "yaw", a_count, device=DEV)
        ref = BR.label_boxes(xyz, lab, "yaw", a_count)
        for k in ("values", "count", "first", "lo", "hi", "R", "center", "size", "yaw"):
            assert np.array_equal(getattr(b, k), ref[k]), (a_count, a, k)
        assert b.yaw[1] == a * ((math.pi / 2) / a_count), (a_count, a)
        err = float(np.abs(b.size[1] - [3.0, 2.0, 1.0]).max())
        worst = max(worst, err)
        print("A %d step %d: sides off by %.3g; half a step %s" % (a_count, a, err, b.size[0].tolist()))
        assert err <= SIDE_BOUND, (a_count, a, err)
        # turned by half a step: no side below the true one (but for rounding), none above what half a step of turn adds
        w, h, d = b.size[0]
        assert 3.0 - SIDE_BOUND <= w <= 3.0 * math.cos(eps) + 2.0 * math.sin(eps) + SIDE_BOUND, (a_count, a, w)
        assert 2.0 - SIDE_BOUND <= h <= 2.0 * math.cos(eps) + 3.0 * math.sin(eps) + SIDE_BOUND, (a_count, a, h)
        assert round(b.yaw[0] / (2 * eps)) in (ha, ha + 1) and d == 1.0
        # pca on the same cloud: the library's frames in the restatement give the same extents.  The cuboid's sides to PCA_BOUND: float32
        # rounding moves a coordinate below 8 m by e <= 2^-22, an entry of the covariance by at most 2 r e with r <= 2 m the reach of
        # the cuboid from its centre, an eigenvector by at most 3 * that over the smallest gap of the variances (0.26 m^2 between the
        # sides of 2 and 1) = 1.1e-5 rad, and a side by that angle times the other half sides (3.7 m) plus 2 e: 4.2e-5
        pc = boxes.label_boxes(xyz, lab, "pca", device=DEV)
        rp = BR.label_boxes(xyz, lab, "pca", frames=pc.R)
        assert np.array_equal(pc.size, rp["size"]) and np.array_equal(pc.center, rp["center"])
        assert np.abs(pc.size - [3.0, 2.0, 1.0]).max() <= PCA_BOUND and np.abs(pc.center - b.center).max() <= PCA_BOUND
    print("worst side error on the grid %.3g" % worst)


_room = {}


def _room_components():
    """the project's room without its three largest planes, as components of the 0.2 m radius graph -> (xyz, component of every vertex or
    -1 on a plane, the planes)"""
    if not _room:
        from seggroup_amd import components, planes
        xyz = G.jittered_room(1, 3000, 1e-3)
        found = planes.detect_planes(xyz, dist=0.005, min_points=40, hypotheses=1024, seed=0, max_planes=3, device=DEV)
        left = np.flatnonzero(found.labels < 0)
        comp, size, count = components.components(left.size, radius=0.2, xyz=xyz[left], device=DEV)
        comp = comp.cpu().numpy() if hasattr(comp, "cpu") else np.asarray(comp)
        lab = np.full(xyz.shape[0], -1, np.int32)
        lab[left] = left[comp]                                            # a component is named by its lowest raw vertex
        _room.update(xyz=xyz, lab=lab, found=found, count=count)
    return _room["xyz"], _room["lab"], _room["found"], _room["count"]


def test_the_rooms_furniture_is_one_box():
    from seggroup_amd import boxes
    xyz, lab, found, count = _room_components()
    assert found.planes.shape[0] == 3 and count == 1
    a = 90
    b = boxes.label_boxes(xyz, lab, "yaw", a, device=DEV)
    ref = BR.label_boxes(xyz, lab, "yaw", a)
    print("room: %d points left in %d component(s); box centre %s size %s yaw %g" % (int((lab >= 0).sum()), count, b.center.tolist(),
                                                                                   b.size.tolist(), float(b.yaw[0])))
    assert b.values.shape == (1,) and b.count[0] == int((lab >= 0).sum()) >= 200
    for k in ("values", "count", "first", "lo", "hi", "R", "center", "size", "yaw"):
        assert np.array_equal(getattr(b, k), ref[k]), k
    m = b.count[0] * 2.0 ** -52
    assert np.abs(b.centroid - ref["centroid"]).max() <= 4 * m and np.abs(b.cov - ref["cov"]).max() <= 4 * m
    # inside the true furniture box (align_ref._FACES rows 3-5: 0.9 x 0.7 x 0.7) grown by 5 mm, five sigma of the jitter
    faces = np.array([[o, np.add(o, u), np.add(o, v), np.add(np.add(o, u), v)] for o, u, v in A._FACES[3:6]]).reshape(-1, 3)
    lo, hi = faces.min(0) - 0.005, faces.max(0) + 0.005
    assert np.allclose(faces.max(0) - faces.min(0), [0.9, 0.7, 0.7])
    cn = b.corners()[0]
    assert (cn >= lo).all() and (cn <= hi).all(), (cn.min(0), cn.max(0), lo, hi)
    step = round(float(b.yaw[0]) / ((math.pi / 2) / a))
    assert b.yaw[0] == step * ((math.pi / 2) / a) and 0 <= step < a
    assert (b.size[0] > [0.8, 0.6, 0.6]).all()


def _tree(root, scene, xyz):
    os.makedirs(os.path.join(root, scene))
    R.write_vertex_only_ply(os.path.join(root, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "seggroup_amd.boxes"] + args, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_command_on_an_experiment(tmp_path):
    """three cuboids and a speck as instances 1..4 of a tiny .sgl: a chair, a wall (not a benchmark class), a table, and a chair of 27
    points (below AP's 100); segment 4 has no instance"""
    from seggroup_amd import boxes, pseudo_labels
    from seggroup_amd.prepare import mesh_arrays, read_ply
    scene = "scene0007_00"
    parts = [BR.lattice_cuboid(angle=0.4, origin=(0, 0, 0)), BR.lattice_cuboid(angle=0.0, origin=(5, 0, 0)),
             BR.lattice_cuboid(2.0, 1.0, 0.5, angle=1.0, origin=(0, 6, 0)), BR.lattice_cuboid(0.5, 0.5, 0.5, origin=(9, 9, 0)),
             _cloud(3, 50) + np.float32(20.0)]
    xyz = np.concatenate(parts).astype(np.float32)
    sov = np.concatenate([np.full(p.shape[0], k) for k, p in enumerate(parts)]).astype(np.int32)
    perm = np.random.RandomState(2).permutation(xyz.shape[0])
    xyz, sov = np.ascontiguousarray(xyz[perm]), sov[perm]
    tables = np.zeros((pseudo_labels.INS_NVEC, 5), np.int32)
    tables[12] = [1, 2, 3, 4, 0]
    tables[13] = [5, 1, 7, 5, 5]
    scans_dir = str(tmp_path / "scans")
    _tree(scans_dir, scene, xyz)
    src = os.path.join(str(tmp_path), "results", "e", scene, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    out = str(tmp_path / "out")
    _run(["--scans", scans_dir, "--out", out, "-n", "e", "--stage", "epoch_last", "--root", str(tmp_path), "--detector-files", "--ply",
          "--workers", "1"])
    ins = tables[12][sov]
    lab = np.where(ins > 0, ins, -1)
    ref = BR.label_boxes(xyz, lab, "yaw", 90, min_points=100)
    keep = np.isin(ref["values"], [1, 3])                                   # instance 2 is a wall, 4 is too small
    with np.load(os.path.join(out, scene + boxes.NPZ_SUFFIX)) as z:
        npz = {k: z[k] for k in z.files}
    assert npz["values"].tolist() == [1, 3] and npz["sem"].tolist() == [5, 7] and str(npz["kind"]) == "yaw" and int(npz["angles"]) == 90
    assert int(npz["min_points"]) == 100
    for k in ("count", "first", "lo", "hi", "R", "center", "size", "yaw"):
        assert np.array_equal(npz[k], ref[k][keep]), k
    bbox = np.load(os.path.join(out, scene + "_bbox.npy"))
    assert bbox.shape == (2, 7) and bbox.dtype == np.float64
    assert np.array_equal(bbox, BR.detector_rows(ref["lo"][keep], ref["hi"][keep], [5, 7]))
    pv, _, pf = mesh_arrays(read_ply(os.path.join(out, scene + ".boxes.ply")))
    assert pv.shape == (16, 3) and pf.shape == (24, 3)
    assert np.array_equal(pv, BR.corners(ref["center"][keep], ref["size"][keep], ref["R"][keep]).reshape(-1, 3).astype(np.float32))
    doc = json.load(open(os.path.join(out, boxes.REPORT_NAME)))
    assert doc["kind"] == "yaw" and doc["angles"] == 90 and doc["min_points"] == 100 and doc["classes"] == "scannet18"
    assert doc["scenes"][scene] == {"V": int(xyz.shape[0]), "instances": 4, "kept": 2, "ignored": 50}
    # --classes all keeps the wall; a second run skips what is there
    rep, skipped = boxes.boxes_scans(scans_dir, out, workers=1, device=DEV, exp="e", stage="epoch_last", root=str(tmp_path))
    assert rep == {} and skipped == [scene]
    rep, _ = boxes.boxes_scans(scans_dir, str(tmp_path / "all"), workers=1, device=DEV, exp="e", stage="epoch_last", root=str(tmp_path),
                               classes="all", kind="aabb", min_points=1)
    assert rep[scene]["kept"] == 4


def test_command_on_any_label_vector(tmp_path):
    """--labels-from over <scene>.planes.npz: the three planes of the room as boxes; a wall is as thin as the plane's dist allows"""
    from seggroup_amd import boxes, planes
    from seggroup_amd.prepare import mesh_arrays, read_ply
    scene = "scene0042_00"
    xyz, _, found, _ = _room_components()
    scans_dir, lab_dir, out = str(tmp_path / "scans"), str(tmp_path / "planes"), str(tmp_path / "out")
    _tree(scans_dir, scene, xyz)
    os.makedirs(lab_dir)
    np.savez(os.path.join(lab_dir, scene + planes.NPZ_SUFFIX), **found.arrays())
    _run(["--scans", scans_dir, "--out", out, "--labels-from", lab_dir, "--suffix", planes.NPZ_SUFFIX, "--key", "labels", "--min-points", "40",
          "--kind", "aabb", "--ply", "--workers", "1"])
    ref = BR.label_boxes(xyz, found.labels, "aabb", min_points=40)
    with np.load(os.path.join(out, scene + boxes.NPZ_SUFFIX)) as z:
        npz = {k: z[k] for k in z.files}
    assert npz["values"].tolist() == [0, 1, 2] and "sem" not in npz and np.isnan(npz["yaw"]).all() and int(npz["angles"]) == 0
    assert npz["count"].tolist() == found.points.tolist()
    for k in ("count", "first", "lo", "hi", "R", "center", "size"):
        assert np.array_equal(npz[k], ref[k]), k
    assert (npz["size"].min(1) <= 2 * 0.005 + 1e-6).all()
    assert not os.path.exists(os.path.join(out, scene + "_bbox.npy"))
    pv, _, pf = mesh_arrays(read_ply(os.path.join(out, scene + ".boxes.ply")))
    assert pv.shape == (24, 3) and pf.shape == (36, 3)
    doc = json.load(open(os.path.join(out, boxes.REPORT_NAME)))
    assert doc["scenes"][scene] == {"V": 3000, "instances": 3, "kept": 3, "ignored": int((found.labels < 0).sum())}
    assert doc["key"] == "labels" and doc["classes"] is None
