"""Plane extraction on the GPU (seggroup_amd/planes.py) against tests/planes_ref.py: sg_plane_ransac's rejections exactly,
its planes to the last bit the reference's own operations leave, its counts between the reference's two fences and its best; the moments
within the bound of two summation orders, the labelling as a mask, and the loop: the six faces of the rotated room, integer for integer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import pcseg_ref as R
import planes_ref as PR
import register_ref as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# d_plane against the restatement, in units of 2^-52 of max(1, |value|) for a normal's component and of max(1, largest |coordinate|) for
# the offset.  Measured on the MI355X over the whole grid below: 0 -- the device's double divide and square root round as NumPy's do and
# nothing contracts.  16 times the measurement is still 0: the planes are held to equality.
PLANE_MEASURED_ULPS = 0.0
PLANE_BOUND_ULPS = 16 * PLANE_MEASURED_ULPS


def _rows(xyz, stride):
    return xyz if stride == 3 else np.ascontiguousarray(np.concatenate([xyz, np.full((xyz.shape[0], stride - 3), 7.0, np.float32)], 1))


def _cloud(seed, n):
    """half of the points near the plane z = 0.5 x + 0.25 (2 mm of noise), the rest anywhere in a 2 m box"""
    rng = np.random.RandomState(seed)
    p = rng.rand(n, 3) * 2.0
    on = rng.rand(n) < 0.5
    p[on, 2] = 0.5 * p[on, 0] + 0.25 + rng.randn(int(on.sum())) * 0.002
    return p.astype(np.float32)


def _plane_ulps(got, want, scale):
    unit = 2.0 ** -52 * np.maximum(1.0, np.abs(want))
    unit[:, 3] = 2.0 ** -52 * max(1.0, scale)
    return float((np.abs(got - want) / unit).max()) if got.size else 0.0


def _check(xyz, h, dist, seed, stride=3, what="", **kw):
    """one call against the reference -> (count, plane, free, best) as the device wrote them, and the reference"""
    from seggroup_amd import planes
    ref = PR.ransac(xyz, dist, h, seed, **kw)
    count, plane, free, best = planes.plane_ransac(_rows(xyz, stride), dist, h, seed, device=DEV, **kw)
    count, plane = count.cpu().numpy(), plane.cpu().numpy()
    assert count.dtype == np.int32 and count.shape == (h,) and plane.dtype == np.float64 and plane.shape == (h, 4)
    assert free == ref.free.size, what
    ok = ~ref.undecided
    assert (~ok).sum() <= 1e-3 * h, what
    assert np.array_equal((count >= 0)[ok], ref.keep[ok]), what
    assert (count[count < 0] == -1).all() and not plane[count < 0].any(), what
    sel = ok & ref.keep & (count >= 0)
    assert (ref.count_lo[sel] <= count[sel]).all() and (count[sel] <= ref.count_hi[sel]).all(), what
    ulps = _plane_ulps(plane[sel], ref.plane[sel], float(np.abs(xyz).max()) if xyz.size else 1.0)
    print("%s: %d kept of %d, %d undecided, plane %.3g ulps, best %d (%d)" % (what, int((count >= 0).sum()), h, int((~ok).sum()), ulps, best, ref.best))
    assert ulps <= PLANE_BOUND_ULPS, (what, ulps)
    assert best == (int(np.argmax(count)) if (count >= 0).any() else -1), what
    if ok.all() and np.array_equal(ref.count_lo, ref.count_hi):
        assert best == ref.best and np.array_equal(count, ref.count), what
    return (count, plane, free, best), ref


@pytest.mark.parametrize("n", [0, 2, 3, 63, 64, 65, 1000, 5000])
def test_ransac_against_the_restatement(n, sg_lib):
    """5,000 free points are five LDS tiles and, below 2,048 waves of hypotheses, five segments.  Generated triples are the restatement's:
    the same bytes come back when register_ref.triples_of is passed in under another seed; walking all H hypotheses instead of the
    compacted kept ones gives the same bytes too"""
    from seggroup_amd import planes
    xyz = _cloud(n, n)
    kept = 0
    for h in (0, 1, 63, 64, 65, 4097):
        seed = 1000 * n + h
        kw = dict(min_edge=0.2, min_sine=0.1)
        (count, plane, free, best), ref = _check(xyz, h, 0.02, seed, stride=6 if n % 2 else 3, what="N %d H %d" % (n, h), **kw)
        kept += int((count >= 0).sum())
        if n < 3:
            assert best == -1 and (count == -1).all() and free == n
        if h and n >= 3:
            passed = planes.plane_ransac(xyz, 0.02, h, seed + 1, triples=G.triples_of(seed, h, n), device=DEV, **kw)
            assert passed[0].cpu().numpy().tobytes() == count.tobytes() and passed[1].cpu().numpy().tobytes() == plane.tobytes(), (n, h)
            assert passed[2:] == (free, best)
            assert sg_lib.sg_plane_set_tuning(0) == 0
            try:
                walked = planes.plane_ransac(xyz, 0.02, h, seed, device=DEV, **kw)
            finally:
                assert sg_lib.sg_plane_set_tuning(1) == 0
            assert walked[0].cpu().numpy().tobytes() == count.tobytes() and walked[1].cpu().numpy().tobytes() == plane.tobytes(), (n, h)
            assert walked[2:] == (free, best)
    if n >= 63:
        assert kept > 0, "no hypothesis was kept at any H: the case checks nothing"


def test_ransac_explicit_triples_and_every_rejection_rule():
    from seggroup_amd import planes
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 0], [0.05, 0, 0], [1, 0.05, 0], [0, 0.5, 0.5], [1, 1, 0], [0.5, 0.25, 0]],
                 np.float32)
    triples = np.array([[0, 0, 1],                                        # a repeated position
                        [0, 4, 1],                                        # a zero-length first edge: 4 is 0's twin
                        [0, 1, 5],                                        # the second edge is 0.05 < min_edge
                        [1, 2, 8], [0, 1, 9],                             # two kept triangles in z = 0
                        [5, 0, 1],                                        # the FIRST edge 5-0 is short
                        [0, 1, 3],                                        # collinear: |c| = 0
                        [0, 3, 6],                                        # a sliver: every edge is 1 m or more, the sine is 0.05 < min_sine
                        [0, 1, 2], [0, 2, 7], [2, 1, 0]], np.int32)       # z = 0; x = 0; z = 0 seen from below
    (count, plane, free, best), ref = _check(p, len(triples), 0.01, 0, what="rules", triples=triples, min_edge=0.1, min_sine=0.1)
    assert not ref.undecided.any() and free == 10
    assert (count >= 0).tolist() == [False, False, False, True, True, False, False, False, True, True, True]
    z0 = int((np.abs(p[:, 2]) <= 0.01).sum())
    assert count[8] == count[10] == count[3] == count[4] == z0 == 9 and best == 3
    assert np.array_equal(plane[8], [0, 0, 1, 0]) and np.array_equal(np.abs(plane[10]), [0, 0, 1, 0]) and plane[10][2] == -1
    assert np.array_equal(plane[9], [1, 0, 0, 0]) and count[9] == int((np.abs(p[:, 0]) <= 0.01).sum())
    # points of a 1/64 m lattice on the plane x + y = 2: the coordinates are exact, so a triple of them counts every point at a distance
    # of a nanometre (the residual is rounding of products of 0.7071.., not 0)
    rng = np.random.RandomState(4)
    a, b = rng.randint(0, 128, 1500) / 64.0, rng.randint(0, 128, 1500) / 64.0
    lat = np.stack([a, 2.0 - a, b], 1).astype(np.float32)
    far = np.array([[int(np.argmin(a + b)), int(np.argmax(a - b)), int(np.argmax(b))]], np.int32)
    (count, plane, _, best), _ = _check(lat, 1, 1e-9, 0, what="lattice", triples=far, min_edge=0.3)
    assert count.tolist() == [1500] and best == 0
    # refused: a position outside the free list (nothing is read through it), a triple table of the wrong shape
    for bad in (1500, -1, 1 << 30):
        with pytest.raises(ValueError, match="a triple names a free point outside 0..1499"):
            planes.plane_ransac(lat, 0.01, 2, triples=np.array([[0, 1, 2], [3, bad, 5]], np.int32), device=DEV)
    with pytest.raises(ValueError):
        planes.plane_ransac(lat, 0.01, 4, triples=far, device=DEV)
    again = planes.plane_ransac(lat, 1e-9, 1, triples=far, min_edge=0.3, device=DEV)    # and the call after a refusal is unharmed
    assert again[0].cpu().numpy().tolist() == [1500]


def test_ransac_label_mask_strides_streams_and_determinism():
    """only every third point is free: triples index the compacted list (explicit ones too), the count runs over the free points alone"""
    import torch
    from seggroup_amd import planes
    n, h = 3001, 515
    xyz = _cloud(77, n)
    labels = np.where(np.arange(n) % 3 == 1, -1 - (np.arange(n) % 5), np.arange(n) % 7).astype(np.int32)
    m = int((labels < 0).sum())
    kw = dict(labels=labels, min_edge=0.2)
    first, ref = _check(xyz, h, 0.02, 5, what="masked", **kw)
    assert first[2] == m == 1000 and ref.free.tolist() == list(range(1, n, 3))
    assert 0 < first[0].max() <= m
    # the same hypotheses on the free points as a cloud of their own
    alone = planes.plane_ransac(xyz[labels < 0], 0.02, h, 5, min_edge=0.2, device=DEV)
    assert alone[0].cpu().numpy().tobytes() == first[0].tobytes() and alone[1].cpu().numpy().tobytes() == first[1].tobytes()
    tri = np.random.RandomState(3).randint(0, m, (h, 3)).astype(np.int32)
    _check(xyz, h, 0.02, 0, what="masked, explicit", triples=tri, **kw)
    with pytest.raises(ValueError, match="outside 0..999"):                # position 1000 exists in the cloud, not in the free list
        planes.plane_ransac(xyz, 0.02, 1, triples=np.array([[0, 1, m]], np.int32), device=DEV, **kw)
    side = torch.cuda.Stream(device=DEV)
    for stride, stream in ((3, None), (6, None), (6, side), (3, side)):
        got = planes.plane_ransac(_rows(xyz, stride), 0.02, h, 5, device=DEV, stream=stream, **kw)
        assert got[0].cpu().numpy().tobytes() == first[0].tobytes() and got[1].cpu().numpy().tobytes() == first[1].tobytes(), (stride, stream)
        assert got[2:] == first[2:]
    # every point labelled: nothing is free
    none = planes.plane_ransac(xyz, 0.02, 64, labels=np.zeros(n, np.int32), device=DEV)
    assert none[2:] == (0, -1) and (none[0].cpu().numpy() == -1).all()


def test_ransac_with_normals_and_a_nan_row():
    from seggroup_amd import planes
    n, h = 2000, 300
    xyz = _cloud(9, n)
    rng = np.random.RandomState(10)
    nrm = rng.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    on = np.abs(xyz[:, 2] - (0.5 * xyz[:, 0] + 0.25)) < 0.01
    nrm[on] = (np.array([-0.5, 0.0, 1.0]) / np.sqrt(1.25)).astype(np.float32)
    nrm[::97] = np.nan
    nrm[5::97, 1] = np.inf
    nrm[7::97] = 0.0
    min_cos = float(np.cos(np.radians(20.0)))
    kw = dict(normals=nrm, min_cos=min_cos, min_edge=0.2)
    (count, plane, _, best), ref = _check(xyz, h, 0.02, 2, what="normals", **kw)
    plain = PR.ransac(xyz, 0.02, h, 2, min_edge=0.2)
    assert np.array_equal(plain.keep, ref.keep) and (ref.count <= plain.count).all() and (ref.count[ref.keep] < plain.count[ref.keep]).any()
    # the best plane is the planted one; its points with a NaN, an infinite or a zero normal are not counted
    usable = on & np.isfinite(nrm).all(1) & (np.abs(nrm).sum(1) > 0)
    assert 0 < ref.count[ref.best] <= int(usable.sum()) + 5 < int(on.sum())
    m = planes.plane_moments(xyz, plane[best], 0.02, normals=nrm, min_cos=min_cos, device=DEV)
    assert m[0] == count[best]                                            # the moments' test is the count's


@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["origin", "1000m"])
def test_moments_are_exact_in_n_bounded_in_the_sums_and_deterministic(offset):
    """sg_align_moments' gate (tests/test_gpu_align.py): the count exact, every sum within N * 2^-52 * the sum of the terms' magnitudes
    of np.sum over the same terms, the same bytes on every call and stream"""
    import torch
    from seggroup_amd import planes
    side = torch.cuda.Stream(device=DEV)
    pl = np.array([-0.5, 0.0, 1.0, -0.25]) / np.sqrt(1.25)
    for n in (0, 1, 255, 1024, 1025, 4 * 1024 + 7, 20000):
        xyz = (_cloud(n + 1, n).astype(np.float64) + offset * np.array([0.6, -0.5, 0.62])).astype(np.float32)
        shifted = np.array([pl[0], pl[1], pl[2], pl[3] - offset * (pl[0] * 0.6 + pl[1] * -0.5 + pl[2] * 0.62)])
        labels = np.where(np.arange(n) % 4 == 3, 2, -1).astype(np.int32)
        origin = 0.5 * (xyz.min(0).astype(np.float64) + xyz.max(0).astype(np.float64)) if n else np.zeros(3)
        for dist, lab in ((0.05, None), (0.05, labels), (0.0, None), (1e9, labels)):
            want, mag = PR.moments(xyz, shifted, dist, origin, lab)
            got = planes.plane_moments(_rows(xyz, 6 if n % 2 else 3), shifted, dist, origin, lab, device=DEV)
            assert got.dtype == np.float64 and got.shape == (11,)
            assert got[0] == want[0], (n, dist)
            if dist == 1e9 and n:
                assert got[0] == int((labels < 0).sum())
            bound = max(n, 1) * 2.0 ** -52 * mag
            assert (np.abs(got - want) <= bound).all(), (n, dist, np.abs(got - want) / np.maximum(bound, 1e-300))
            again = planes.plane_moments(xyz, shifted, dist, origin, lab, device=DEV)
            other = planes.plane_moments(xyz, shifted, dist, origin, lab, device=DEV, stream=side)
            assert again.tobytes() == got.tobytes() and other.tobytes() == got.tobytes(), (n, dist)
    with pytest.raises(ValueError):
        planes.plane_moments(xyz, [0, 0, np.nan, 0], 0.05, device=DEV)
    with pytest.raises(ValueError):
        planes.plane_moments(xyz, pl, -1.0, device=DEV)


def test_assign_labels_the_reference_mask_and_returns_its_size():
    import torch
    from seggroup_amd import planes
    n = 5003
    xyz = _cloud(21, n)
    nrm = np.tile((np.array([-0.5, 0.0, 1.0]) / np.sqrt(1.25)).astype(np.float32), (n, 1))
    nrm[::3] = (1.0, 0.0, 0.0)
    nrm[4::50] = np.nan
    pl = np.array([-0.5, 0.0, 1.0, -0.25]) / np.sqrt(1.25)
    start = np.where(np.arange(n) % 5 == 0, 3, -1 - (np.arange(n) % 2)).astype(np.int32)
    x64 = xyz.astype(np.float64)
    for normals, min_cos in ((None, 0.0), (nrm, 0.9)):
        free = PR.free_of(n, start)
        mask = np.zeros(n, bool)
        mask[free] = PR.inliers(x64[free], pl, 0.004, None if normals is None else normals.astype(np.float64)[free], min_cos)
        want = start.copy()
        want[mask] = 9
        got, done = planes.plane_assign(_rows(xyz, 6), start, pl, 0.004, 9, normals, min_cos, device=DEV)
        assert done == int(mask.sum()) > 100 and np.array_equal(got.cpu().numpy(), want)
        m = planes.plane_moments(xyz, pl, 0.004, labels=start, normals=normals, min_cos=min_cos, device=DEV)
        assert m[0] == done                                               # ... the count's and the moments' test again
    # a device tensor is updated in place; a second call finds nothing left to label
    d_lab = torch.from_numpy(start).to(DEV)
    out, done = planes.plane_assign(xyz, d_lab, pl, 0.004, 0, device=DEV)
    assert out.data_ptr() == d_lab.data_ptr() and done > 0
    assert planes.plane_assign(xyz, d_lab, pl, 0.004, 1, device=DEV)[1] == 0
    with pytest.raises(ValueError, match="id"):
        planes.plane_assign(xyz, start, pl, 0.004, -1, device=DEV)
    assert planes.plane_assign(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), pl, 0.004, 1, device=DEV)[1] == 0


def test_stage_timer_times_every_entry_and_the_tuning_knob_leaves_it_on(sg_lib):
    """hip.stage_timer("plane") around one call of each entry point: the same bytes as untimed, five finite times with the stages that ran
    above 0, and sg_plane_set_tuning inside the block does not switch the timer off.  A call on two points ends before its count (M < 3), so a
    timed one leaves that stage at 0: the count of the call after the knob was turned is above 0 only if it was timed.  After the block an
    untimed call leaves the record as it was."""
    from seggroup_amd import hip, planes
    xyz, two = _cloud(63, 63), _cloud(2, 2)
    pl = np.array([-0.5, 0.0, 1.0, -0.25]) / np.sqrt(1.25)
    free = np.full(63, -1, np.int32)

    def calls(cloud=xyz):
        count, plane, _, best = planes.plane_ransac(cloud, 0.02, 65, 7, min_edge=0.2, device=DEV)
        m = planes.plane_moments(xyz, pl, 0.05, device=DEV)
        lab, done = planes.plane_assign(xyz, free, pl, 0.05, 4, device=DEV)
        return [count.cpu().numpy().tobytes(), plane.cpu().numpy().tobytes(), m.tobytes(), lab.cpu().numpy().tobytes()], best, done

    plain = calls()
    assert plain[1] >= 0 and plain[2] > 0, "nothing was kept or labelled: the case checks nothing"
    with hip.stage_timer("plane") as t:
        assert t.names == ["compact", "generate", "count", "moments", "assign"]
        assert calls() == plain
        us = t.read()
        assert len(us) == len(t.names) and all(np.isfinite(u) and u > 0.0 for u in us), us
        calls(two)
        assert t.read()[t.names.index("count")] == 0.0
        assert sg_lib.sg_plane_set_tuning(0) == 0
        try:
            assert calls() == plain
        finally:
            assert sg_lib.sg_plane_set_tuning(1) == 0
        last = t.read()
        assert all(np.isfinite(u) and u > 0.0 for u in last), last
    assert calls(two)[0][2:] == plain[0][2:] and calls() == plain
    assert t.read() == last


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
_found = {}


def _detected():
    from seggroup_amd import planes
    if "d" not in _found:
        _found["d"] = planes.detect_planes(PR.fixture()[0], device=DEV, **PR.PARAMS)
    return _found["d"]


def test_detect_planes_equals_the_restatement_on_the_rotated_room():
    from seggroup_amd import planes
    xyz, P = PR.fixture()
    ref = PR.fixture_reference()
    assert not ref.fenced
    got = _detected()
    print("planes", got.points.tolist(), "ransac", got.ransac_count.tolist(), "h", got.h.tolist(), "rms", ["%.3g" % r for r in got.rms])
    assert got.planes.shape == (6, 4) and got.labels.dtype == np.int32
    assert np.array_equal(got.labels, ref.labels) and np.array_equal(got.h, ref.h)
    assert np.array_equal(got.ransac_count, ref.ransac_count) and np.array_equal(got.points, ref.points)
    assert np.abs(got.planes - ref.planes).max() < 1e-9 and np.abs(got.centroid - ref.centroid).max() < 1e-9
    assert np.abs(got.rms - ref.rms).max() < 1e-9
    corners = PR.face_corners(P)
    for f in range(6):
        off = np.abs(corners[f] @ got.planes[:, :3].T + got.planes[:, 3]).max(0)
        assert off.min() <= PR.PARAMS["dist"], (f, off)
    assert (got.dist, got.min_points, got.hypotheses, got.seed, got.min_edge, got.min_sine) == (0.005, 40, 1024, 0, 0.05, 0.1)
    again = planes.detect_planes(xyz, device=DEV, **PR.PARAMS)
    for k, v in got.arrays().items():
        assert np.asarray(again.arrays()[k]).tobytes() == np.asarray(v).tobytes(), k
    # a small cloud, and one without a plane that large, find nothing
    assert planes.detect_planes(xyz[:2], device=DEV, **PR.PARAMS).planes.shape == (0, 4)
    none = planes.detect_planes(xyz, 0.005, min_points=2000, hypotheses=256, device=DEV)
    assert none.planes.shape == (0, 4) and (none.labels == -1).all() and none.centroid.shape == (0, 3)


def test_level_transform_puts_the_floor_at_zero():
    from seggroup_amd import align, planes
    xyz, P = PR.fixture()
    got = _detected()
    T = planes.level_transform(got, xyz, "largest")
    moved = align.apply(xyz, T, device=DEV).cpu().numpy().astype(np.float64)
    floor = PR.face_corners(P)[0] @ T[:3, :3].T + T[:3, 3]
    assert np.abs(floor[:, 2]).max() <= PR.PARAMS["dist"]
    assert moved[got.labels != 0, 2].min() > 0.0


def _tree(root, scene, xyz):
    os.makedirs(os.path.join(root, scene))
    R.write_vertex_only_ply(os.path.join(root, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))


def test_command_levels_and_removes(tmp_path):
    """the command in a child process writes the .npz, the report and the levelled scan; --remove leaves nothing of a room that is all
    planes, and with --max-planes 3 it leaves the box, whose three faces are one component of the radius graph (their points' longest
    single-linkage edge is 0.137 m; the radius is 0.2)"""
    from seggroup_amd import components, planes
    from seggroup_amd.prepare import mesh_arrays, read_ply
    scene = "scene0042_00"
    xyz, P = PR.fixture()
    ref = PR.fixture_reference()
    src = str(tmp_path / "scans")
    _tree(src, scene, xyz)
    with open(os.path.join(src, scene, scene + ".aggregation.json"), "w") as f:
        f.write("{}")
    out = str(tmp_path / "level")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.planes", "--scans", src, "--out", out, "--dist", "0.005", "--min-points", "40", "--hypotheses", "1024",
           "--workers", "1", "--level"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    with np.load(os.path.join(out, scene + planes.NPZ_SUFFIX)) as z:
        npz = {k: z[k] for k in z.files}
    assert np.array_equal(npz["labels"], ref.labels) and np.array_equal(npz["points"], ref.points) and npz["planes"].shape == (6, 4)
    assert float(npz["dist"]) == 0.005 and int(npz["hypotheses"]) == 1024 and np.isnan(npz["normal_angle"])
    doc = json.load(open(os.path.join(out, planes.REPORT_NAME)))
    e = doc["scenes"][scene]
    assert doc["dist"] == 0.005 and doc["level"] == "largest" and e["V"] == 3000 and e["unlabelled"] == 0 and e["level"] == 0
    assert [p["points"] for p in e["planes"]] == ref.points.tolist() and np.allclose([p["equation"] for p in e["planes"]], npz["planes"])
    T = np.array(e["T"])
    moved = mesh_arrays(read_ply(os.path.join(out, scene, scene + "_vh_clean_2.ply")))[0]
    assert moved.tobytes() == A.apply(xyz, T).tobytes()
    assert moved[ref.labels != 0, 2].min() > 0.0 and np.abs(moved[ref.labels == 0, 2]).max() <= 0.005 + 1e-6
    assert os.path.exists(os.path.join(out, scene, scene + ".aggregation.json"))
    # a second run skips what is there
    rep, skipped = planes.planes_scans(src, out, 0.005, 40, hypotheses=1024, level="largest", workers=1, device=DEV)
    assert rep == {} and skipped == [scene]

    gone = str(tmp_path / "gone")
    rep, _ = planes.planes_scans(src, gone, 0.005, 40, hypotheses=1024, remove=True, workers=1, device=DEV)
    assert rep[scene]["M"] == 0 and rep[scene]["unlabelled"] == 0
    assert mesh_arrays(read_ply(os.path.join(gone, scene, scene + "_vh_clean_2.ply")))[0].shape == (0, 3)
    box = str(tmp_path / "box")
    rep, _ = planes.planes_scans(src, box, 0.005, 40, hypotheses=1024, max_planes=3, remove=True, workers=1, device=DEV)
    assert rep[scene]["M"] == int((ref.labels >= 3).sum()) == 254 and len(rep[scene]["planes"]) == 3
    left = mesh_arrays(read_ply(os.path.join(box, scene, scene + "_vh_clean_2.ply")))[0]
    with np.load(os.path.join(box, scene, scene + components.MAP_SUFFIX)) as z:
        assert np.array_equal(z["kept"], np.nonzero(ref.labels >= 3)[0]) and np.array_equal(z["plane"], np.where(ref.labels < 3, ref.labels, -1))
        assert np.array_equal(left, xyz[z["kept"]])
    comp, size, count = components.components(left.shape[0], radius=0.2, xyz=left, device=DEV)
    assert count == 1 and int(size.max()) == 254
    # with the floor and the walls still in, the box is one component with them: this is what the removal is for
    comp, size, count = components.components(xyz.shape[0], radius=0.2, xyz=xyz, device=DEV)
    assert int(size.max()) == 3000
