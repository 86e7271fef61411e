"""The radius graph on the GPU: count, comp, size and C of sg_radius_count_grid / sg_components_radius BIT-EQUAL to the NumPy
statement (tests/radius_ref.py) and to the committed digests -- jittered lines at the tile edges with no edge, a single path and everything
joined; the two clumps that the kNN graph splits; the speck cloud at three radii, each at the library's cell, at two forced cells that need
a block of two or more rings, and as one cell; every cloud of the point-cloud segmenter's cases; the label filter; rows of 4 and 6 floats;
the refusals on the device; two streams in flight; the Python forms; a face-less scan directory through clean_scan and the command line in
child processes; fragments on the radius graph."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import components_ref as CR
import pcseg_ref
import radius_ref as R
from conftest import GOLDEN, ROOT
from test_gpu_pcseg import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cases, _solved, _specks = {}, {}, {}
# per speck radius: two forced cells whose block needs R >= 2 rings (the table of 5,307 points holds 2^22 cells: no edge below 0.0264)
FORCED = {0.04: ((0.035, 2), (0.028, 2)), 0.06: ((0.04, 2), (0.028, 3)), R.SPECK_JOIN_RADIUS: ((1.0, 2), (0.5, 4))}
ONE_CELL = 100.0


def _case(name):
    if not _cases:
        _cases.update(R.fixture_cases())
    return _cases[name]


def _ref(name):
    if name not in _solved:
        _solved[name] = R.solve(*_case(name))
    return _solved[name]


def _speck_ref(radius):
    """the speck cloud and the statement at one radius: computed once"""
    if "xyz" not in _specks:
        _specks["xyz"], _specks["tag"] = CR.speck_cloud()
    if radius not in _specks:
        _specks[radius] = R.solve(_specks["xyz"], radius)
    return _specks["xyz"], _specks[radius]


def _expected():
    return json.load(open(os.path.join(GOLDEN, "radius_expected.json")))


def _run(xyz, radius, cell=0.0, labels=None, stream=None):
    """-> (count, comp, size, C) as arrays, and the statistics of the components call"""
    from seggroup_amd import components as M
    n = xyz.shape[0]
    comp, size, c = M.components(n, radius=radius, xyz=xyz, cell=cell, labels=labels, device=DEV, stream=stream)
    stats = M.radius_stats()
    cnt = M.neighbour_counts(xyz, radius, cell=cell, device=DEV, stream=stream)
    assert M.radius_stats()["R"] == stats["R"] and M.radius_stats()["cells"] == stats["cells"], "one index for both entry points"
    for t in (cnt, comp, size):
        assert str(t.dtype) == "torch.int32" and t.is_cuda and t.shape == (n,)
    return (cnt.cpu().numpy(), comp.cpu().numpy(), size.cpu().numpy(), c), stats


def _same(got, want, what):
    assert got[3] == want[3], f"{what}: C = {got[3]}, the statement has {want[3]}"
    assert np.array_equal(got[0], want[0]), f"{what}: count"
    assert np.array_equal(got[1], want[1]), f"{what}: comp"
    assert np.array_equal(got[2], want[2]), f"{what}: size"


def _fixture(got, name):
    e = _expected()[name]
    assert (e["C"], e["sizes"], e["comp_sha256"], e["count_sha256"]) == (got[3], CR.sizes_desc(got[1])[:10], R.digest(got[1]), R.digest(got[0])), name


@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_with_no_edge_a_single_path_and_everything_joined(n):
    for tag in R.LINE_RADII:
        name = "line_%d_%s" % (n, tag)
        xyz, radius = _case(name)
        got, stats = _run(xyz, radius)
        _same(got, _ref(name), name)
        _fixture(got, name)
        assert stats["R"] == 1
    assert _ref("line_%d_none" % n)[3] == n and _ref("line_%d_path" % n)[3] == 1
    assert (_ref("line_%d_all" % n)[0] == n - 1).all()


def test_two_clumps_are_one_component_where_the_knn_graph_has_two():
    from seggroup_amd import components as M
    from seggroup_amd import prepare
    xyz = R.two_clumps()
    table = prepare.pointcloud_knn(xyz, R.CLUMP_K, device=DEV)
    _, _, c_knn = M.components(24, knn=table, xyz=xyz, max_edge=R.CLUMP_RADIUS, device=DEV)
    assert c_knn == 2, "sg_components_knn at k = 10: every point's ten nearest are its eleven siblings"
    got, _ = _run(xyz, R.CLUMP_RADIUS)
    assert got[3] == 1 and (got[0] == 23).all() and (got[1] == 0).all() and (got[2] == 24).all()
    _same(got, _ref("two_clumps"), "two_clumps")
    _fixture(got, "two_clumps")


@pytest.mark.parametrize("radius", R.SPECK_RADII + (R.SPECK_JOIN_RADIUS,))
def test_speck_cloud_at_every_cell_edge(radius):
    xyz, want = _speck_ref(radius)
    assert xyz.shape[0] == 5307
    got, stats = _run(xyz, radius)
    _same(got, want, "the library's cell")
    assert stats["R"] == 1 and stats["cell"] > radius
    if radius in R.SPECK_RADII:
        _fixture(got, "specks_%g" % radius)
    else:
        assert got[3] == 3 and CR.sizes_desc(got[1]) == [5307 - 11, 8, 3], "the speck of 15 has joined the room, the others have not"
    for cell, rings in FORCED[radius]:
        forced, stats = _run(xyz, radius, cell=cell)
        assert stats["R"] == rings and abs(stats["cell"] - cell) < 1e-6 * cell, (cell, stats)
        _same(forced, want, "a forced cell of %g" % cell)
    one, stats = _run(xyz, radius, cell=ONE_CELL)
    assert stats["cells"] == [1, 1, 1] and stats["R"] == 1 and stats["largest_cell"] == 5307 and stats["occupied"] == 1
    _same(one, want, "one cell")
    for other in (got, forced):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:3], other[:3])), "the same bytes at every cell edge"


@pytest.mark.parametrize("name", CASES)
def test_clouds_of_the_point_cloud_segmenter(name):
    xyz, radius = _case("cloud_" + name)
    got, stats = _run(xyz, radius)
    _same(got, _ref("cloud_" + name), name)
    _fixture(got, "cloud_" + name)
    n = xyz.shape[0]
    if name == "all_equal":
        assert stats["cells"] == [1, 1, 1] and (got[0] == n - 1).all() and got[3] == 1
    if name == "room_dup":
        assert int((got[0] == 0).sum()) == 0 and got[3] == _ref("cloud_room_j5e-4")[3], "a point and its copy are neighbours"
    if name == "room_20k":
        wide, stats = _run(xyz, radius, cell=0.5)
        assert stats["largest_cell"] > 256 and stats["R"] == 1, "a cell of more than one tile of candidates"
        _same(wide, _ref("cloud_" + name), name + " at a cell of 0.5")


def test_label_filter():
    xyz, want = _speck_ref(0.06)
    n = xyz.shape[0]
    stripes = R.stripes(n)
    got, _ = _run(xyz, 0.06, labels=stripes)
    ref = R.solve(xyz, 0.06, labels=stripes)
    _same(got, ref, "stripes")
    assert ref[3] > want[3] and np.array_equal(got[0], want[0]), "the filter cuts the graph and does not touch count"
    _same(_run(xyz, 0.06, labels=np.full(n, -7, np.int32))[0], want, "all labels equal")
    distinct, _ = _run(xyz, 0.06, labels=(np.arange(n) - n // 2).astype(np.int32))
    assert distinct[3] == n and np.array_equal(distinct[1], np.arange(n)) and (distinct[2] == 1).all() and np.array_equal(distinct[0], want[0])


def test_rows_of_4_and_6_floats():
    xyz, want = _speck_ref(0.06)
    rng = np.random.RandomState(2)
    for extra in (1, 3):
        rows = np.concatenate([xyz, rng.uniform(-9, 9, (xyz.shape[0], extra)).astype(np.float32)], 1)
        _same(_run(rows, 0.06)[0], want, "rows of %d floats" % (3 + extra))


def test_size_may_be_null_and_stage_times_and_counters(sg_lib):
    import torch
    from seggroup_amd import hip
    xyz, want = _speck_ref(0.06)
    n = xyz.shape[0]
    d_x = torch.from_numpy(xyz).to(DEV)
    comp = torch.empty(n, dtype=torch.int32, device=DEV)
    cnt = torch.empty(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(sg_lib.sg_radius_grid_ws_bytes(n), dtype=torch.uint8, device=DEV)
    c = C.c_int(0)
    sg_lib.sg_radius_grid_set_timing(1)
    try:
        hip.check(sg_lib.sg_components_radius(d_x.data_ptr(), 3, n, 0.06, 0.0, None, comp.data_ptr(), None, C.byref(c), ws.data_ptr(), ws.numel(), None))
        us, h = (C.c_float * 7)(), (C.c_int64 * 9)()
        assert sg_lib.sg_radius_grid_stage_times(us, 7) == 7 and sg_lib.sg_radius_grid_stats(h, 9) == 9
        assert all(0.0 < t < 1e6 for t in us), list(us)
        pairs = int(want[0].astype(np.int64).sum())
        assert h[8] == pairs and pairs <= h[7] <= n * n, "pairs passed (ordered) and pair tests evaluated"
        hip.check(sg_lib.sg_radius_count_grid(d_x.data_ptr(), 3, n, 0.06, 0.0, cnt.data_ptr(), ws.data_ptr(), ws.numel(), None))
        assert sg_lib.sg_radius_grid_stats(h, 9) == 9 and h[8] == pairs
    finally:
        sg_lib.sg_radius_grid_set_timing(0)
    assert c.value == want[3] and np.array_equal(comp.cpu().numpy(), want[1]) and np.array_equal(cnt.cpu().numpy(), want[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_leave_the_library_usable():
    from seggroup_amd import components as M
    from seggroup_amd import hip
    xyz, want = _speck_ref(0.06)
    n = xyz.shape[0]
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[n - 1, 1] = bad
        for call in (lambda: M.components(n, radius=0.06, xyz=x, device=DEV), lambda: M.neighbour_counts(x, 0.06, device=DEV)):
            with pytest.raises(hip.SgError) as ei:
                call()
            assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
        _same(_run(xyz, 0.06)[0], want, "after a refusal")
    with pytest.raises(hip.SgError) as ei:
        M.components(n, radius=1.0, xyz=xyz, cell=0.05, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "more than 16 rings" in str(ei.value), "a forced cell that needs R = 21"
    with pytest.raises(hip.SgError) as ei:
        M.neighbour_counts(xyz, 0.04, cell=0.021, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "cells; the table" in str(ei.value), "a forced cell past the table bound"
    with pytest.raises(hip.SgError) as ei:
        M.neighbour_counts(xyz, 1e-6, cell=1e-6, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "cell too small" in str(ei.value), "an axis of 2^21 cells or more"
    _same(_run(xyz, 0.06)[0], want, "after the refusals")


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
def test_two_streams_in_flight_give_the_same_bytes_as_alone():
    import torch
    jobs = {0.06: None, R.SPECK_JOIN_RADIUS: None}
    for radius in jobs:
        _speck_ref(radius)
    errors = []

    def work(radius):
        try:
            stream = torch.cuda.Stream(device=DEV)
            jobs[radius] = [_run(_specks["xyz"], radius, stream=stream)[0] for _ in range(4)]
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(r,)) for r in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for radius, runs in jobs.items():
        for got in runs:
            _same(got, _specks[radius], "radius %g beside another stream" % radius)


# ---- Python ------------------------------------------------------------------------------------------------------------------------------
def test_python_forms():
    import torch
    from seggroup_amd import components as M
    xyz, want = _speck_ref(0.06)
    n = xyz.shape[0]
    a, b = R.pairs(xyz, 0.06)
    edges = np.stack([a, b], 1).astype(np.int32)
    by_edges = M.components(n, edges=edges, device=DEV)
    by_radius = M.components(n, radius=0.06, xyz=torch.from_numpy(xyz).to(DEV), device=DEV)
    assert by_edges[2] == by_radius[2] == want[3]
    assert torch.equal(by_edges[0], by_radius[0]) and torch.equal(by_edges[1], by_radius[1])
    cnt = M.neighbour_counts(torch.from_numpy(xyz), np.float32(0.06), cell=None, device=DEV)
    assert np.array_equal(cnt.cpu().numpy(), want[0]) and np.array_equal(want[0], np.bincount(np.concatenate([a, b]), minlength=n))
    lab = (_specks["tag"] > 0).astype(np.int32)
    got = M.fragments(lab, n, radius=0.06, xyz=xyz, device=DEV)
    assert got["instances"] == 2 and got["fragmented"] == 2 and got["pieces"] == {0: [2081, 1600, 1600], 1: [15, 8, 3]}


# ---- scan directories ------------------------------------------------------------------------------------------------------------------
PLY = "_vh_clean_2.ply"


def _speck_scan(scans_dir, name):
    """a face-less scan directory of the speck cloud (as the island scan's face-less twin of 8j's test)"""
    xyz, _ = _speck_ref(0.06)
    sp = os.path.join(scans_dir, name)
    os.makedirs(sp)
    rgb = np.stack([_specks["tag"] * 7 + 30] * 3, 1).astype(np.uint8)
    pcseg_ref.write_vertex_only_ply(os.path.join(sp, name + PLY), xyz, rgb)
    return xyz, _specks["tag"], rgb


def _check_cleaned(dst, name, xyz, rgb, keep, want, entry, min_verts, min_neighbours, dropped):
    from seggroup_amd import prepare
    kept, new_of_old, _ = CR.clean_arrays(keep, np.zeros((0, 3), np.int32))
    got_xyz, got_rgb, faces = prepare.mesh_arrays(prepare.read_ply(os.path.join(dst, name + PLY)))
    assert got_xyz.tobytes() == xyz[kept].tobytes() and np.array_equal(got_rgb, rgb[kept]) and faces.shape[0] == 0
    with np.load(os.path.join(dst, name + ".clean.npz")) as z:
        assert np.array_equal(z["kept"], kept) and np.array_equal(z["new_of_old"], new_of_old)
        assert z["comp"].dtype == np.int32 and np.array_equal(z["comp"], want[1])
        assert z["count"].dtype == np.int32 and np.array_equal(z["count"], want[0])
        assert str(z["source"]) == "radius" and float(z["radius"]) == np.float32(0.06) and int(z["min_neighbours"]) == min_neighbours
        assert int(z["min_verts"]) == min_verts
    assert entry["V"] == xyz.shape[0] and entry["M"] == kept.shape[0] and entry["components"] == want[3] and entry["source"] == "radius"
    assert entry["kept_components"] == np.unique(want[1][keep]).shape[0] and entry["largest_sizes"] == CR.sizes_desc(want[1])[:10]
    assert entry["radius"] == 0.06 and entry["R"] == 1 and 0.06 < entry["cell"] < 0.0605 and entry["dropped"] == dropped


def test_faceless_scan_is_cleaned_with_radius_and_min_neighbours(tmp_path):
    from seggroup_amd import components as M
    name = "scene0061_00"
    raw = str(tmp_path / "raw")
    xyz, tag, rgb = _speck_scan(raw, name)
    want = _specks[0.06]
    # every room point has two neighbours or more at 0.06; the size rule on the radius graph over ALL points takes the three specks
    out = str(tmp_path / "clean")
    entry = M.clean_scan(os.path.join(raw, name), out, min_verts=20, radius=0.06, min_neighbours=2, device=DEV)
    keep = (want[0] >= 2) & (want[2] >= 20)
    assert np.array_equal(keep, tag == 0), "exactly the specks are gone"
    _check_cleaned(os.path.join(out, name), name, xyz, rgb, keep, want, entry, 20, 2, {"size": 26, "min_neighbours": 0})
    # the count rule alone: the speck of 3 and the 12 room points with two neighbours
    out3 = str(tmp_path / "clean3")
    entry = M.clean_scan(os.path.join(raw, name), out3, radius=0.06, min_neighbours=3, device=DEV)
    keep = want[0] >= 3
    assert int((~keep).sum()) == 15 and not keep[tag == 3].any() and keep[tag == 8].all() and keep[tag == 15].all()
    _check_cleaned(os.path.join(out3, name), name, xyz, rgb, keep, want, entry, -1, 3, {"size": 0, "min_neighbours": 15})
    # without min_neighbours the radius graph is one more graph source: no count in the file
    out_r = str(tmp_path / "clean_r")
    entry = M.clean_scan(os.path.join(raw, name), out_r, largest=True, radius=0.06, device=DEV)
    assert entry["M"] == 2081 and entry["dropped"] == {"size": 5307 - 2081}
    with np.load(os.path.join(out_r, name, name + ".clean.npz")) as z:
        assert "count" not in z.files and str(z["source"]) == "radius"


def test_command_line_in_child_processes(tmp_path):
    from seggroup_amd import pseudo_labels
    name = "scene0062_00"
    raw = str(tmp_path / "raw")
    xyz, tag, rgb = _speck_scan(raw, name)
    want = _specks[0.06]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.components"]

    def run(*args):
        return subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)

    out = str(tmp_path / "clean")
    r = run("--scans", raw, "--out", out, "--radius", "0.06", "--min-neighbours", "2", "--min-verts", "20")
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "cleaned %s 5307 -> 5281 vertices, 6 -> 3 components" % name in r.stdout
    report = json.load(open(os.path.join(out, "clean_report.json")))
    assert report["radius"] == 0.06 and report["min_neighbours"] == 2 and report["min_verts"] == 20 and report["max_edge"] is None
    _check_cleaned(os.path.join(out, name), name, xyz, rgb, tag == 0, want, report["scenes"][name], 20, 2, {"size": 26, "min_neighbours": 0})
    # parser errors, not silent defaults
    for args in (("--scans", raw, "--out", out, "--radius", "0.06"), ("--scans", raw, "--out", out, "--min-neighbours", "2"),
                 ("--scans", raw, "--out", out, "--min-verts", "20", "--radius", "0.06", "--max-edge", "0.06")):
        r = run(*args)
        assert r.returncode == 2 and "error:" in r.stderr, args
    # --fragments --radius: one instance over the room (three pieces at 0.06), one over the specks (three pieces)
    sov = (tag > 0).astype(np.int32)
    tables = np.zeros((pseudo_labels.INS_NVEC, 2), np.int32)
    tables[12] = [1, 2]
    src = os.path.join(str(tmp_path), "results", "e", name, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    path = str(tmp_path / "fragments.json")
    r = run("--fragments", "--scans", raw, "-n", "e", "--stage", "epoch_last", "--root", str(tmp_path), "--radius", "0.06", "--json", path)
    assert r.returncode == 0 and "2 in pieces" in r.stdout, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(path))["scenes"][name]
    assert doc["source"] == "radius" and doc["pieces"] == {"1": [2081, 1600, 1600], "2": [15, 8, 3]} and doc["outside_largest"] == 3200 + 11
