"""The radius graph without a GPU: the NumPy statement (tests/radius_ref.py) against the committed fixture and against a
float64 kd-tree on every case of the fixture, its two forms against each other, the arguments the library and the module refuse before the
first device call, the command line's new parser errors and the old ones, which are unchanged."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import components_ref as CR
import radius_ref as R
from conftest import GOLDEN

_cases, _solved = {}, {}
NAMES = sorted(R.fixture_cases())


def _case(name):
    if not _cases:
        _cases.update(R.fixture_cases())
    return _cases[name]


def _solve(name):
    if name not in _solved:
        _solved[name] = R.solve(*_case(name))
    return _solved[name]


def _expected():
    return json.load(open(os.path.join(GOLDEN, "radius_expected.json")))


def test_fixture_holds_exactly_the_cases():
    e = _expected()
    assert sorted(e) == NAMES
    for name in NAMES:
        assert e[name]["radius"] == _case(name)[1] and e[name]["N"] == _case(name)[0].shape[0]
        assert e[name]["nearest_pair_to_radius"] > 1e-6, "no pair of a committed case lies on the radius"


@pytest.mark.parametrize("name", NAMES)
def test_statement_against_the_fixture_and_the_kdtree(name):
    pytest.importorskip("scipy")
    xyz, radius = _case(name)
    cnt, comp, size, c = _solve(name)
    assert cnt.dtype == comp.dtype == size.dtype == np.int32
    e = _expected()[name]
    assert (e["C"], e["sizes"], e["comp_sha256"], e["count_sha256"]) == (c, CR.sizes_desc(comp)[:10], R.digest(comp), R.digest(cnt))
    assert e["pairs"] * 2 == int(cnt.astype(np.int64).sum())
    k_cnt, k_comp, k_c, nearest = R.kdtree(xyz, radius)
    assert nearest > 1e-6
    assert np.array_equal(cnt, k_cnt) and np.array_equal(comp, k_comp) and c == k_c
    assert np.array_equal(size, np.bincount(comp, minlength=comp.shape[0])[comp])


def test_what_the_cases_are_for():
    e = _expected()
    for n in R.SIZES:
        assert e["line_%d_none" % n]["C"] == n and e["line_%d_none" % n]["pairs"] == 0
        assert e["line_%d_path" % n]["C"] == 1 and e["line_%d_path" % n]["pairs"] == n - 1, "a single path"
        assert e["line_%d_all" % n]["C"] == 1 and e["line_%d_all" % n]["pairs"] == n * (n - 1) // 2, "everything joined"
    assert e["two_clumps"]["C"] == 1 and e["two_clumps"]["pairs"] == 24 * 23 // 2
    assert e["specks_0.04"]["sizes"][:3] == [15, 8, 3] and e["specks_0.04"]["C"] > 5000, "below the lattice spacing: the room in points"
    assert e["specks_0.06"]["sizes"][-3:] == [15, 8, 3] and e["specks_0.06"]["C"] == 6
    assert e["cloud_all_equal"]["C"] == 1 and e["cloud_all_equal"]["pairs"] == 32 * 31 // 2, "coincident points are neighbours"


def test_two_clumps_in_the_knn_graph_and_in_the_radius_graph():
    """why the radius graph exists: at k = 10 every point's ten nearest are its eleven siblings, so the kNN graph cut at 0.02 has two
    components although every pair of the 24 points is within 0.02"""
    import pcseg_ref
    xyz = R.two_clumps()
    table = pcseg_ref.knn_table(xyz, R.CLUMP_K)
    assert CR.from_knn(xyz, table, R.CLUMP_RADIUS)[2] == 2
    cnt, comp, size, c = R.solve(xyz, R.CLUMP_RADIUS)
    assert c == 1 and (cnt == 23).all() and (comp == 0).all() and (size == 24).all()


def test_the_two_forms_of_the_statement_agree():
    xyz, tag = CR.speck_cloud()
    for radius in R.SPECK_RADII:
        plain = R.count(xyz, radius)
        a, b = R.pairs(xyz, radius)
        for labels in (None, R.stripes(xyz.shape[0]), (tag > 0).astype(np.int32)):
            cnt, comp, size, c = R.solve(xyz, radius, labels)
            p_comp, p_size, p_c = CR.components(xyz.shape[0], a, b, labels=labels)
            assert np.array_equal(comp, p_comp) and np.array_equal(size, p_size) and c == p_c
            assert np.array_equal(cnt, plain), "the filter does not touch count"
    a, b = R.pairs(xyz, 0.06)
    assert (a < b).all() and a.shape[0] == _expected()["specks_0.06"]["pairs"]


def test_the_join_radius_joins_the_nearest_speck_alone():
    xyz, tag = CR.speck_cloud()
    cnt, comp, size, c = R.solve(xyz, R.SPECK_JOIN_RADIUS)
    assert c == 3 and sorted(set(size.tolist())) == [3, 8, 5307 - 11]
    assert (size[tag == 15] == 5307 - 11).all() and (size[tag == 8] == 8).all() and (size[tag == 3] == 3).all()


def test_statement_refuses_what_the_library_refuses():
    x = np.zeros((4, 3), np.float32)
    for bad in (0.0, -1.0, np.nan, np.inf, 1e30, 1e-30):
        with pytest.raises(ValueError):
            R.solve(x, bad)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[2, 1] = bad
        with pytest.raises(ValueError):
            R.count(y, 0.1)
    with pytest.raises(ValueError):
        R.solve(x, 0.1, labels=np.zeros(3, np.int32))


# ---- the library and the module, before a device call --------------------------------------------------------------------------------
def test_library_refuses_before_the_first_device_call(sg_lib):
    from seggroup_amd import hip
    cap = hip.MAX_GRID_POINTS
    ws = sg_lib.sg_radius_grid_ws_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(cap + 1) == 0
    assert ws(1) >= 4 * (1 << 22) and ws(257) > ws(1) and ws(cap) > 13 * 4 * cap
    buf = (C.c_char * 64)()                                     # never read: every call below is refused on its arguments
    p, c = C.addressof(buf), C.c_int(-1)
    big = 1 << 40
    count, comps = sg_lib.sg_radius_count_grid, sg_lib.sg_components_radius
    nan, inf = float("nan"), float("inf")
    calls = {
        "count: null points": (count(None, 3, 4, 0.1, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: null count": (count(p, 3, 4, 0.1, 0.0, None, p, big, None), hip.SG_EINVAL),
        "count: null workspace": (count(p, 3, 4, 0.1, 0.0, p, None, big, None), hip.SG_EINVAL),
        "count: stride 2": (count(p, 2, 4, 0.1, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: no point": (count(p, 3, 0, 0.1, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: radius 0": (count(p, 3, 4, 0.0, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: radius negative": (count(p, 3, 4, -0.1, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: radius NaN": (count(p, 3, 4, nan, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: radius inf": (count(p, 3, 4, inf, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: r2 overflows": (count(p, 3, 4, 1e30, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: r2 underflows": (count(p, 3, 4, 1e-30, 0.0, p, p, big, None), hip.SG_EINVAL),
        "count: cell negative": (count(p, 3, 4, 0.1, -1.0, p, p, big, None), hip.SG_EINVAL),
        "count: cell NaN": (count(p, 3, 4, 0.1, nan, p, p, big, None), hip.SG_EINVAL),
        "count: cell inf": (count(p, 3, 4, 0.1, inf, p, p, big, None), hip.SG_EINVAL),
        "count: short workspace": (count(p, 3, 1000, 0.1, 0.0, p, p, ws(1000) - 1, None), hip.SG_ENOMEM),
        "count: N above the cap": (count(p, 3, cap + 1, 0.1, 0.0, p, p, big, None), hip.SG_EUNSUP),
        "components: null points": (comps(None, 3, 4, 0.1, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: null comp": (comps(p, 3, 4, 0.1, 0.0, None, None, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: null C": (comps(p, 3, 4, 0.1, 0.0, None, p, None, None, p, big, None), hip.SG_EINVAL),
        "components: null workspace": (comps(p, 3, 4, 0.1, 0.0, None, p, None, C.byref(c), None, big, None), hip.SG_EINVAL),
        "components: stride 2": (comps(p, 2, 4, 0.1, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: no point": (comps(p, 3, 0, 0.1, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: radius 0": (comps(p, 3, 4, 0.0, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: radius NaN": (comps(p, 3, 4, nan, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: cell negative": (comps(p, 3, 4, 0.1, -2.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "components: short workspace": (comps(p, 3, 1000, 0.1, 0.0, None, p, None, C.byref(c), p, 16, None), hip.SG_ENOMEM),
        "components: N above the cap": (comps(p, 3, cap + 1, 0.1, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EUNSUP),
    }
    for what, (rc, want) in calls.items():
        assert rc == want, what
    assert count(p, 3, 1000, 0.1, 0.0, p, p, 16, None) == hip.SG_ENOMEM and b"workspace too small" in sg_lib.sg_last_error()
    assert count(p, 3, 4, 0.0, 0.0, p, p, big, None) == hip.SG_EINVAL and b"radius" in sg_lib.sg_last_error()
    assert [sg_lib.sg_radius_grid_stage_name(i) for i in range(8)] == [b"box", b"cells", b"sort", b"table", b"init", b"search", b"finish", None]
    assert sg_lib.sg_radius_grid_stage_times(None, 7) == hip.SG_EINVAL and sg_lib.sg_radius_grid_stats(None, 9) == hip.SG_EINVAL
    h = (C.c_int64 * 9)()
    assert sg_lib.sg_radius_grid_stats(h, 8) == hip.SG_EINVAL and sg_lib.sg_radius_grid_stats(h, 9) == 9
    assert sg_lib.sg_radius_grid_set_timing(0) == hip.SG_OK


def test_module_refuses_before_a_device_call():
    from seggroup_amd import components as M
    e, t = np.zeros((2, 2), np.int32), np.zeros((4, 11), np.int32)
    x = np.zeros((4, 3), np.float32)
    bad = [dict(radius=0.1), dict(radius=0.1, xyz=x, edges=e), dict(radius=0.1, xyz=x, knn=t), dict(radius=0.1, xyz=x, faces=np.zeros((1, 3), np.int32)),
           dict(radius=0.1, xyz=x, max_edge=0.1), dict(radius=0.0, xyz=x), dict(radius=-1.0, xyz=x), dict(radius=float("nan"), xyz=x),
           dict(radius=float("inf"), xyz=x), dict(radius=0.1, xyz=x[:3]), dict(radius=0.1, xyz=x[:, :2]), dict(radius=0.1, xyz=x.reshape(-1)),
           dict(radius=0.1, xyz=x, cell=-1.0), dict(radius=0.1, xyz=x, cell=float("inf")), dict(radius=0.1, xyz=x, labels=np.zeros(3, np.int32)),
           dict(edges=e, cell=0.5), dict(edges=e, xyz=x)]
    for kw in bad:
        with pytest.raises(ValueError):
            M.components(4, **kw)
    for args in ((x, 0.0), (x, float("nan")), (x[:, :2], 0.1), (x[:0], 0.1), (x.reshape(-1), 0.1)):
        with pytest.raises(ValueError):
            M.neighbour_counts(*args)
    with pytest.raises(ValueError):
        M.neighbour_counts(x, 0.1, cell=-1.0)
    for kw in (dict(min_neighbours=3), dict(min_neighbours=0, radius=0.1), dict(min_neighbours=3, radius=0.1, min_verts=2, largest=True),
               dict(radius=0.1), dict()):
        with pytest.raises(ValueError):
            M.clean_scan("nowhere/scene0000_00", "out", **kw)
        with pytest.raises(ValueError):
            M.clean_scans("nowhere", "out", **kw)


def _two_scans(tmp_path):
    from seggroup_amd.prepare import write_ply
    isl = CR.island_mesh()
    scans = tmp_path / "scans"
    for scene, faces in (("mesh0000_00", isl["faces"]), ("cloud0000_00", np.zeros((0, 3), np.int32))):
        os.makedirs(scans / scene)
        write_ply(str(scans / scene / (scene + "_vh_clean_2.ply")), isl["xyz"], isl["rgb"], faces)
    (tmp_path / "mesh.txt").write_text("mesh0000_00\n")
    (tmp_path / "cloud.txt").write_text("cloud0000_00\n")
    return str(scans), str(tmp_path / "mesh.txt"), str(tmp_path / "cloud.txt")


def test_command_line_new_parser_errors(tmp_path, capsys):
    from seggroup_amd import components as M
    scans, only_mesh, only_cloud = _two_scans(tmp_path)
    base = ["--scans", scans, "--out", str(tmp_path / "out")]
    cloud = base + ["--scenes", only_cloud]
    wrong = {
        "--radius with --max-edge": cloud + ["--min-verts", "20", "--radius", "0.1", "--max-edge", "0.1"],
        "--radius on a mesh": base + ["--scenes", only_mesh, "--min-verts", "20", "--radius", "0.1"],
        "--radius with a mesh in the list": base + ["--min-verts", "20", "--radius", "0.1"],
        "--radius 0": cloud + ["--min-verts", "20", "--radius", "0"],
        "--radius inf": cloud + ["--min-verts", "20", "--radius", "inf"],
        "--min-neighbours without --radius": cloud + ["--min-neighbours", "3", "--max-edge", "0.1"],
        "--min-neighbours alone": cloud + ["--min-neighbours", "3"],
        "--min-neighbours 0": cloud + ["--radius", "0.1", "--min-neighbours", "0"],
        "--radius without a rule": cloud + ["--radius", "0.1"],
        "both size rules beside --min-neighbours": cloud + ["--radius", "0.1", "--min-neighbours", "3", "--min-verts", "20", "--largest"],
        "--fragments with --min-neighbours": ["--fragments", "--scans", scans, "-n", "exp", "--radius", "0.1", "--min-neighbours", "3"],
        "--fragments --radius with --max-edge": ["--fragments", "--scans", scans, "-n", "exp", "--scenes", only_cloud, "--radius", "0.1", "--max-edge", "0.1"],
        "--fragments --radius on a mesh": ["--fragments", "--scans", scans, "-n", "exp", "--scenes", only_mesh, "--radius", "0.1"],
    }
    for what, argv in wrong.items():
        with pytest.raises(SystemExit) as ei:
            M.main(argv)
        assert ei.value.code == 2, what
    err = capsys.readouterr().err
    assert "--radius" in err and "--min-neighbours" in err
    assert not (tmp_path / "out").exists()


def test_command_line_old_parser_errors_are_unchanged(tmp_path, capsys):
    from seggroup_amd import components as M
    scans, only_mesh, _ = _two_scans(tmp_path)
    base = ["--scans", scans, "--out", str(tmp_path / "out")]
    wrong = [(base, "exactly one of --min-verts M and --largest is needed"),
             (base + ["--min-verts", "20", "--largest"], "exactly one of --min-verts M and --largest is needed"),
             (base + ["--min-verts", "0"], "--min-verts must be at least 1"),
             (base + ["--min-verts", "20"], "cloud0000_00 has no faces and needs --max-edge R (the scan's unit; there is no default)"),
             (base + ["--min-verts", "20", "--scenes", only_mesh, "--pointcloud"], "--pointcloud needs --max-edge R (the scan's unit; there is no default)"),
             (base + ["--min-verts", "20", "--scenes", only_mesh, "--max-edge", "0.1"],
              "--max-edge belongs to the kNN graph: every scan here is a mesh (--pointcloud ignores the faces)"),
             (["--scans", scans, "--largest"], "cleaning needs --out DIR"),
             (["--fragments", "--scans", scans], "--fragments needs -n EXP")]
    for argv, message in wrong:
        with pytest.raises(SystemExit) as ei:
            M.main(argv)
        assert ei.value.code == 2, argv
        assert capsys.readouterr().err.rstrip().endswith("error: " + message), argv
    assert not (tmp_path / "out").exists()
