"""The exact grid-indexed kNN on the GPU: sg_pointcloud_knn_grid's table EQUAL to the brute-force statement
(tests/pcseg_ref.knn_table) and to the brute-force kernel on every cloud of test_gpu_pcseg.CASES at the library's cell, at a cell so
small that the points sit (nearly) alone and at one so large that the cloud is one cell; k; the staging tile's edges; a cell larger than
a tile; the shifted room that needs the score margin; outliers that the rings cannot settle; the segmenter's later stages and ids
through index="grid"; two streams; the refusals; one cloud above 2^20 points; the command line in a child process.

The statistics of the last call (oversegment.knn_grid_stats) show that each run took the path it aims at."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_grid_ref as G
import pcseg_ref as R
import test_gpu_pcseg as P
import thin_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, WAVE = 256, 64                            # candidates per LDS tile of the search, queries per block
# a forced cell that leaves the points (nearly) alone in their cells, small enough a grid that the rings still settle somebody
SMALL = {"room_j0": 0.04, "room_j5e-4": 0.04, "room_j2e-3": 0.04, "room_dup": 0.04, "n_k_plus_1": 0.3, "n255": 0.04, "n256": 0.04, "n257": 0.04,
         "line": 0.5, "all_equal": 0.04, "room_20k": 0.02}
ONE_CELL = 100.0
_extra = {}


def _shifted():
    if "shifted" not in _extra:
        _extra["shifted"] = G.shifted(P._cloud("room_j5e-4"), G.MARGIN_SHIFT)
    return _extra["shifted"]


def _grid(xyz, k=10, cell=None):
    from seggroup_amd import oversegment, prepare
    t = prepare.pointcloud_knn(xyz, k, device=DEV, index="grid", cell=cell)
    return t, oversegment.knn_grid_stats()


def _brute(xyz, k=10):
    from seggroup_amd import prepare
    return prepare.pointcloud_knn(xyz, k, device=DEV)


def _equal(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, what
    bad = (got != want).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first {np.flatnonzero(bad)[:5].tolist()}: " \
                          f"{got[bad][0].tolist()} != {want[bad][0].tolist()}"


@pytest.mark.parametrize("name", P.CASES)
def test_table_equals_brute_force_at_every_cell(name):
    xyz, want = P._cloud(name), P._ref(name)["knn"]
    assert np.array_equal(_brute(xyz).cpu().numpy(), want)
    t, st = _grid(xyz)
    print(f"{name} default: {st}")
    _equal(t, want, f"{name}, the library's cell")
    assert st["cell"] > 0 and st["occupied"] >= 1 and np.prod(st["cells"]) >= st["occupied"]
    t, st = _grid(xyz, cell=SMALL[name])
    print(f"{name} small: {st}")
    _equal(t, want, f"{name}, cell = {SMALL[name]}")
    assert st["cell"] == np.float32(SMALL[name])
    grid = G.Grid(xyz, SMALL[name])
    assert st["cells"] == tuple(grid.nc.tolist()) and st["occupied"] == grid.occupied() and st["largest_cell"] == grid.largest_cell()
    if name == "all_equal":
        assert st["occupied"] == 1 and st["max_ring"] == 1, "one point 32 times is one cell at any edge"
    else:
        assert st["largest_cell"] <= 2 and st["max_ring"] >= 2, "more than one ring was walked"
    t, st = _grid(xyz, cell=ONE_CELL)
    print(f"{name} one cell: {st}")
    _equal(t, want, f"{name}, one cell")
    assert st["occupied"] == 1 and st["cells"] == (1, 1, 1) and st["largest_cell"] == xyz.shape[0] and st["max_ring"] == 1 and st["fallback"] == 0


@pytest.mark.parametrize("k", [5, 10, 20])
def test_k(k):
    xyz, want = P._cloud(P.SWEEP_CASE), P._ref(P.SWEEP_CASE, k)["knn"]
    for cell in (None, SMALL[P.SWEEP_CASE], ONE_CELL):
        t, st = _grid(xyz, k, cell)
        _equal(t, want, f"k = {k}, cell = {cell}")
        assert tuple(t.shape) == (xyz.shape[0], k + 1)
    assert np.array_equal(_brute(xyz, k).cpu().numpy(), want)


@pytest.mark.parametrize("n", [WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_the_tile_edges(n):
    """N at the edge of a wave of queries and of a staging tile: in one cell every query walks the whole cloud tile by tile"""
    xyz = np.ascontiguousarray(P._cloud("room_20k")[:n])
    want = R.knn_table(xyz)
    assert np.array_equal(_brute(xyz).cpu().numpy(), want)
    for cell in (None, 0.2, ONE_CELL):
        t, st = _grid(xyz, cell=cell)
        _equal(t, want, f"N = {n}, cell = {cell}")
    assert st["largest_cell"] == n


def test_a_cell_larger_than_a_tile():
    xyz, want = P._cloud("room_20k"), P._ref("room_20k")["knn"]
    t, st = _grid(xyz, cell=0.5)
    print(st)
    _equal(t, want, "room_20k, cell = 0.5")
    assert st["largest_cell"] > TILE and st["largest_cell"] == G.Grid(xyz, 0.5).largest_cell()


def test_the_shifted_room_needs_the_margin_and_gets_it():
    """room_j5e-4 + (300, 200, 10): the scores' rounding error is ~0.03, the squared spacing 0.0025 (tests/test_knn_grid_ref.py shows an
    unguarded search going wrong here).  The table equals the brute-force statement, the brute-force kernel and the grid statement."""
    xyz = _shifted()
    want = R.knn_table(xyz)
    assert np.array_equal(_brute(xyz).cpu().numpy(), want)
    rows = np.sort(np.random.RandomState(13).choice(xyz.shape[0], 300, replace=False))
    stated, rings, _ = G.knn_table_grid(xyz, 10, 0.05, ring_limit=40, rows=rows)
    assert np.array_equal(stated, want[rows]) and (rings > 0).all()
    for cell in (None, 0.05):
        t, st = _grid(xyz, cell=cell)
        print(f"cell = {cell}: {st}")
        _equal(t, want, f"shifted room, cell = {cell}")
    assert st["fallback"] > 0, "at 0.05 the margin spans more rings than the limit: the queue finished those rows"


def test_outliers_are_finished_by_the_fallback():
    xyz = G.with_outliers(P._cloud("room_j5e-4"))
    want = R.knn_table(xyz)
    for cell in (None, 0.1):
        t, st = _grid(xyz, cell=cell)
        print(f"cell = {cell}: {st}")
        _equal(t, want, f"outliers, cell = {cell}")
        assert 1 <= st["fallback"] < xyz.shape[0] // 2 and st["max_ring"] >= 1
    assert np.array_equal(_brute(xyz).cpu().numpy(), want)


@pytest.mark.parametrize("name", ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup"])
def test_the_segmenter_through_the_grid(name):
    """table, normals, edge set, weights and sorted order bit-equal to the statement; the ids equal R.merge and the committed sha256"""
    from seggroup_amd import oversegment
    xyz, ref = P._cloud(name), P._ref(name)
    n = xyz.shape[0]
    exp = json.load(open(os.path.join(P.GOLDEN, "pcseg_expected.json")))[name]
    for cell in (None, SMALL[name]):
        got_e, got_w = P._check_stages(oversegment.pointcloud_edges(xyz, device=DEV, index="grid", cell=cell), ref, n, f"{name} cell = {cell}")
        assert got_e.shape[0] == exp["edges"]
        seg = oversegment.segment_pointcloud(xyz, device=DEV, index="grid", cell=cell)
        assert seg.dtype == np.int32 and np.array_equal(seg, R.merge(ref["edges"], ref["w"], n)) and R.digest(seg) == exp["sha256"]
    assert oversegment.knn_grid_stats()["cell"] == np.float32(SMALL[name])
    seg = oversegment.segment_pointcloud(xyz, device=DEV, index="grid", viewpoint=tuple(R.default_viewpoint(xyz).tolist()), k_thresh=0.01, seg_min_verts=20)
    assert R.digest(seg) == exp["sha256"]


@pytest.mark.parametrize("name", ["room_dup", "room_20k"])
def test_two_streams_give_identical_bytes(name):
    import torch
    from seggroup_amd import oversegment
    xyz = P._cloud(name)
    a = oversegment.pointcloud_edges(xyz, device=DEV, index="grid")
    b = oversegment.pointcloud_edges(xyz, device=DEV, index="grid", stream=torch.cuda.Stream(device=DEV))
    c = oversegment.pointcloud_edges(xyz, device=DEV, index="grid", cell=0.11, stream=torch.cuda.Stream(device=DEV))
    for key in ("knn", "normals", "edges", "w"):
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes() == c[key].cpu().numpy().tobytes(), key
    s1 = oversegment.segment_pointcloud(xyz, device=DEV, index="grid")
    s2 = oversegment.segment_pointcloud(xyz, device=DEV, index="grid", stream=torch.cuda.Stream(device=DEV))
    assert s1.tobytes() == s2.tobytes() == oversegment.segment_pointcloud(xyz, device=DEV).tobytes()


def test_refusals():
    import torch
    from seggroup_amd import hip, oversegment, prepare
    xyz = P._cloud("n257")
    calls = (lambda x, **kw: prepare.pointcloud_knn(x, kw.pop("k", 10), device=DEV, index="grid", **kw),
             lambda x, **kw: oversegment.pointcloud_edges(x, kw.pop("k", 10), device=DEV, index="grid", **kw),
             lambda x, **kw: oversegment.segment_pointcloud(x, kw.pop("k", 10), device=DEV, index="grid", **kw))
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[xyz.shape[0] - 1, 2] = bad
        for call in calls:
            with pytest.raises(hip.SgError) as ei:
                call(x)
            assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    x = xyz.copy()
    x[3] = (1e19, -1e19, 1e19)
    for call in calls:
        with pytest.raises(hip.SgError) as ei:
            call(x)
        assert ei.value.code == hip.SG_EUNSUP and "brute-force path" in str(ei.value) and "sg_pointcloud_knn" in str(ei.value)
    for call in calls:
        with pytest.raises(hip.SgError) as ei:
            call(xyz[:10])
        assert ei.value.code == hip.SG_EINVAL and "points for k =" in str(ei.value)
        with pytest.raises(hip.SgError) as ei:
            call(xyz, k=7)
        assert ei.value.code == hip.SG_EUNSUP
        with pytest.raises(hip.SgError) as ei:
            call(P._cloud("line"), cell=1e-9)
        assert ei.value.code == hip.SG_EUNSUP and "cell too small" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        calls[0](P._cloud("line"), cell=0.04)                    # 198 x 394 x 99 cells: beyond the dense table of 64 points
    assert ei.value.code == hip.SG_EUNSUP and "table" in str(ei.value)
    # a workspace one byte short, and N above the cap (the check comes first: nothing is allocated for it)
    lib = hip.lib()
    n = xyz.shape[0]
    d_x = torch.from_numpy(xyz).to(DEV)
    out = torch.empty((n, 11), dtype=torch.int32, device=DEV)
    need = lib.sg_pointcloud_knn_grid_ws_bytes(n, 10)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.sg_pointcloud_knn_grid(d_x.data_ptr(), 3, n, 10, 0.0, out.data_ptr(), ws.data_ptr(), need - 1, None) == hip.SG_ENOMEM
    assert b"workspace too small" in lib.sg_last_error()
    assert lib.sg_pointcloud_knn_grid(d_x.data_ptr(), 3, n, 10, 0.0, out.data_ptr(), ws.data_ptr(), need, None) == hip.SG_OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.knn_table(xyz))
    assert lib.sg_pointcloud_knn_grid(d_x.data_ptr(), 3, (1 << 24) + 1, 10, 0.0, out.data_ptr(), ws.data_ptr(), need, None) == hip.SG_EUNSUP
    need = lib.sg_pcseg_ws_bytes_indexed(n, 10, hip.KNN_GRID)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    nrm, e, w = torch.empty_like(d_x), torch.empty((n * 10, 2), dtype=torch.int32, device=DEV), torch.empty(n * 10, device=DEV)
    n_e = C.c_int(0)
    assert lib.sg_pcseg_edges_indexed(d_x.data_ptr(), n, 10, None, hip.KNN_GRID, 0.0, None, nrm.data_ptr(), e.data_ptr(), w.data_ptr(), C.byref(n_e),
                                      ws.data_ptr(), need - 1, None) == hip.SG_ENOMEM
    assert lib.sg_pcseg_edges_indexed(d_x.data_ptr(), n, 10, None, 2, 0.0, None, nrm.data_ptr(), e.data_ptr(), w.data_ptr(), C.byref(n_e),
                                      ws.data_ptr(), need, None) == hip.SG_EINVAL
    assert lib.sg_pcseg_edges_indexed(d_x.data_ptr(), (1 << 24) + 1, 10, None, hip.KNN_GRID, 0.0, None, nrm.data_ptr(), e.data_ptr(), w.data_ptr(),
                                      C.byref(n_e), ws.data_ptr(), need, None) == hip.SG_EUNSUP


def test_a_cloud_above_the_brute_force_limit():
    """thin_ref.big_cloud(): 1,058,050 points.  64 seeded rows against the statement over the whole cloud; on the first 1,000,000 points the
    table and the ids equal the brute-force path's; on the full cloud the ids are the chain over the grid's edges and a valid id vector;
    without `index` the cloud is still refused."""
    import torch
    from seggroup_amd import hip, oversegment, prepare
    big = thin_ref.big_cloud()[0]
    n = big.shape[0]
    assert n == 1058050 > 1 << 20
    t = prepare.pointcloud_knn(big, 10, device=DEV, index="grid")
    st = oversegment.knn_grid_stats()
    print(st)
    assert tuple(t.shape) == (n, 11)
    rows = np.sort(np.random.RandomState(17).choice(n, 64, replace=False))
    got = t[torch.from_numpy(rows).to(DEV)].cpu().numpy()
    for i in range(0, 64, 8):
        assert np.array_equal(got[i:i + 8], R._top(R.pair_scores(big[rows[i:i + 8]], big), 11)), f"rows {rows[i:i + 8].tolist()}"
    del t
    part = np.ascontiguousarray(big[:1000000])
    tg, tb = prepare.pointcloud_knn(part, 10, device=DEV, index="grid"), prepare.pointcloud_knn(part, 10, device=DEV)
    assert torch.equal(tg, tb)
    del tg, tb
    assert np.array_equal(oversegment.segment_pointcloud(part, device=DEV, index="grid"), oversegment.segment_pointcloud(part, device=DEV))
    seg = oversegment.segment_pointcloud(big, device=DEV, index="grid")
    r = oversegment.pointcloud_edges(big, device=DEV, index="grid")
    assert np.array_equal(seg, oversegment.merge_edges(r["edges"].cpu().numpy(), r["w"].cpu().numpy(), n))
    assert seg.shape == (n,) and np.array_equal(seg[seg], seg) and (seg <= np.arange(n)).all()
    with pytest.raises(hip.SgError) as ei:
        oversegment.segment_pointcloud(big, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP


def test_command_line_index_grid(tmp_path):
    """--pointcloud --index grid in a child process writes the bytes that the default index writes"""
    from seggroup_amd import oversegment
    scan, xyz = P._cloud_scan("scene0033_00")
    scans = str(tmp_path / "scans")
    os.makedirs(os.path.join(scans, scan.name))
    R.write_vertex_only_ply(os.path.join(scans, scan.name, scan.name + "_vh_clean_2.ply"), xyz, scan.rgb)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.oversegment", "--workers", "1", "--scans", scans, "--pointcloud", "--force"]
    path = os.path.join(scans, scan.name, oversegment.segs_json_name(scan.name))
    r = subprocess.run(cmd + ["--index", "grid"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    from_grid = open(path, "rb").read()
    os.remove(path)
    p = oversegment.oversegment_scan(os.path.join(scans, scan.name), device=DEV, pointcloud=True)
    assert p == path and open(p, "rb").read() == from_grid
    assert oversegment.oversegment_scan(os.path.join(scans, scan.name), device=DEV, pointcloud=True, index="grid", voxel=0.05, force=True) == path
