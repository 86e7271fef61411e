"""The exact grid-indexed nearest point between two clouds on the GPU: sg_nearest_point_grid's indices EQUAL to
sg_nearest_point's and to the plain statement (tests/nearest_grid_ref.brute) on the pairs that each catch one mistake, at the library's
cell, at a small forced cell and as one cell; the wave, tile and sort-tile edges of both counts; a cell larger than a tile; strides; d2;
two streams; the shifted pair that needs the score margin; queries the rings cannot settle; the refusals; one cloud above 2^20 points;
the opt-in of get_unmapper and sample_points; and sg_pointcloud_knn_grid, whose stages are now shared, against the committed digests."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nearest_grid_ref as NG
import pcseg_ref as R
import test_gpu_pcseg as P
import thin_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, WAVE = 256, 64
PAIRS = ["plain", "lattice", "dup", "all_equal", "half_room", "outliers", "shifted"]
ONE_CELL = 1000.0
_want, _stated = {}, {}


def _grid(x, y, cell=None, **kw):
    from seggroup_amd import prepare
    idx, d2 = prepare.nearest_point_grid(x, y, cell=cell, device=DEV, **kw)
    return idx.cpu().numpy(), (d2.cpu().numpy() if d2 is not None else None), prepare.nearest_grid_stats()


def _kernel_brute(x, y):
    from seggroup_amd import prepare
    return prepare.get_unmapper(np.ascontiguousarray(x[:, :3]), y, device=DEV).cpu().numpy()


def _statement(name):
    """the statement at the pair's small cell over ALL queries, and brute's answer, computed once and shared"""
    if name not in _stated:
        x, y = NG.case_pairs()[name]
        idx, rings, grid = NG.nearest_grid(x, y, NG.CELLS[name][0], threads=8)
        _stated[name] = (idx, NG.stats_of(grid, rings))
        _want[name] = grid.whole
    return _stated[name]


def _brute(name):
    _statement(name)
    return _want[name]


def _equal(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first {np.flatnonzero(bad)[:5].tolist()}: " \
                          f"{got[bad][:5].tolist()} != {want[bad][:5].tolist()}"


@pytest.mark.parametrize("name", PAIRS)
def test_indices_equal_brute_force_at_every_cell(name):
    x, y = NG.case_pairs()[name]
    want = _brute(name)
    _equal(_kernel_brute(x, y), want, f"{name}: sg_nearest_point against the statement")
    got, d2, st = _grid(x, y)
    print(f"{name} default: {st}")
    _equal(got, want, f"{name}, the library's cell")
    assert d2.dtype == np.float32 and d2.tobytes() == NG.d2_of(x, y, want).tobytes(), "d2 bit for bit"
    assert st["cell"] > 0 and st["occupied"] >= 1 and np.prod(st["cells"]) >= st["occupied"]
    small = NG.CELLS[name][0]
    stated, sst = _statement(name)
    assert np.array_equal(stated, want)
    got, d2, st = _grid(x, y, cell=small)
    print(f"{name} small: {st} statement: {sst}")
    _equal(got, want, f"{name}, cell = {small}")
    assert d2.tobytes() == NG.d2_of(x, y, want).tobytes()
    assert st["cell"] == np.float32(small)
    assert (st["cells"], st["occupied"], st["largest_cell"]) == (sst["cells"], sst["occupied"], sst["largest_cell"])
    assert st["fallback"] == sst["fallback"], "the queue holds the queries the statement leaves unsettled at the ring limit"
    if sst["fallback"] < x.shape[0]:
        assert st["max_ring"] == sst["max_ring"]
    if name == "outliers":
        assert st["fallback"] == 2
    if name == "half_room":
        assert 0 < st["fallback"] < x.shape[0] and st["max_ring"] > 1
    if name == "shifted":
        assert st["fallback"] == x.shape[0], "at 0.05 the margin spans more rings than the limit: every row through the queue"
    got, _, st = _grid(x, y, cell=ONE_CELL, want_d2=False)
    _equal(got, want, f"{name}, one cell")
    assert st["cells"] == (1, 1, 1) and st["occupied"] == 1 and st["largest_cell"] == y.shape[0] and st["max_ring"] == 1 and st["fallback"] == 0


def test_the_shifted_pair_settled_by_the_rings():
    """at a cell of 0.3 the margin of the shifted pair is two rings: every row settled by the rule, none queued, all equal to brute"""
    x, y = NG.case_pairs()["shifted"]
    got, _, st = _grid(x, y, cell=0.3)
    print(st)
    _equal(got, _brute("shifted"), "shifted, cell = 0.3")
    assert st["fallback"] == 0 and st["max_ring"] == 2


EDGES = [1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


@pytest.mark.parametrize("u", EDGES)
def test_the_wave_tile_and_sort_tile_edges(u):
    """U and N from room_20k's prefixes: the queries are the LAST u points, so they are not among the candidates"""
    big = P._cloud("room_20k")
    x = np.ascontiguousarray(big[-u:])
    for n in EDGES:
        y = np.ascontiguousarray(big[:n])
        want = _kernel_brute(x, y)
        if u * n <= 65 * 65:
            assert np.array_equal(want, NG.brute(x, y))
        for cell in (None, 0.2, ONE_CELL):
            got, _, st = _grid(x, y, cell=cell, want_d2=False)
            _equal(got, want, f"U = {u}, N = {n}, cell = {cell}")
        assert st["largest_cell"] == n


def test_a_cell_larger_than_a_tile():
    big = P._cloud("room_20k")
    x, y = np.ascontiguousarray(big[1::2]), np.ascontiguousarray(big[::2])
    got, d2, st = _grid(x, y, cell=0.5)
    print(st)
    want = _kernel_brute(x, y)
    _equal(got, want, "room_20k halves, cell = 0.5")
    assert st["largest_cell"] > TILE and st["largest_cell"] == NG.Grid(x, y, 0.5).largest_cell()
    assert d2.tobytes() == NG.d2_of(x, y, want).tobytes()


def test_strides_and_no_d2():
    """candidate rows of 6 floats, query rows of 4; d2 = NULL is accepted"""
    x, y = NG.case_pairs()["plain"]
    rng = np.random.RandomState(3)
    x4 = np.ascontiguousarray(np.concatenate([x, rng.standard_normal((x.shape[0], 1)).astype(np.float32)], 1))
    y6 = np.ascontiguousarray(np.concatenate([y, rng.standard_normal((y.shape[0], 3)).astype(np.float32)], 1))
    want = _brute("plain")
    for cell in (None, 0.04):
        got, d2, _ = _grid(x4, y6, cell=cell)
        _equal(got, want, f"strides 4 / 6, cell = {cell}")
        assert d2.tobytes() == NG.d2_of(x, y, want).tobytes()
        got, d2, _ = _grid(x4, y6, cell=cell, want_d2=False)
        _equal(got, want, "d2 = NULL")
        assert d2 is None


@pytest.mark.parametrize("name", ["dup", "half_room"])
def test_two_streams_and_two_cells_give_identical_bytes(name):
    import torch
    x, y = NG.case_pairs()[name]
    a = _grid(x, y)
    b = _grid(x, y, stream=torch.cuda.Stream(device=DEV))
    c = _grid(x, y, cell=0.11, stream=torch.cuda.Stream(device=DEV))
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()


def test_refusals():
    import torch
    from seggroup_amd import hip, prepare
    x, y = NG.case_pairs()["plain"]
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            xx, yy = x.copy(), y.copy()
            (xx, yy)[which][-1, 2] = bad
            with pytest.raises(hip.SgError) as ei:
                prepare.nearest_point_grid(xx, yy, device=DEV)
            assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    yy = y.copy()
    yy[3] = (1e19, -1e19, 1e19)
    with pytest.raises(hip.SgError) as ei:
        prepare.nearest_point_grid(x, yy, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "brute-force path" in str(ei.value) and "sg_nearest_point" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        prepare.nearest_point_grid(x, y, cell=1e-9, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "cell too small" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        prepare.nearest_point_grid(x, y, cell=0.005, device=DEV)          # 401^3 cells: beyond the dense table
    assert ei.value.code == hip.SG_EUNSUP and "table" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        prepare.nearest_point_grid(x, y[:0], device=DEV)
    assert ei.value.code == hip.SG_EINVAL
    idx, d2 = prepare.nearest_point_grid(x[:0], y, device=DEV)
    assert tuple(idx.shape) == (0,) and tuple(d2.shape) == (0,)
    lib = hip.lib()
    u, n = x.shape[0], y.shape[0]
    d_x, d_y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = torch.full((u,), -7, dtype=torch.int64, device=DEV)
    need = lib.sg_nearest_point_grid_ws_bytes(u, n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    call = lambda uu=u, nn=n, nb=need: lib.sg_nearest_point_grid(d_x.data_ptr(), 3, uu, d_y.data_ptr(), 3, nn, 0.0, out.data_ptr(), None,   # noqa: E731
                                                                 ws.data_ptr(), nb, None)
    assert call(nb=need - 1) == hip.SG_EINVAL and b"workspace too small" in lib.sg_last_error()
    assert call(nn=0) == hip.SG_EINVAL
    assert call(nn=(1 << 24) + 1) == hip.SG_EUNSUP
    assert call(uu=0) == hip.SG_OK
    torch.cuda.synchronize()
    assert (out == -7).all(), "nothing was touched"
    assert call() == hip.SG_OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _brute("plain"))


def test_a_cloud_above_the_brute_force_limit():
    """Queries: thin_ref.big_cloud(), 1,058,050 points.  Candidates big[rep] at a voxel of 0.05 (5,403 points), then big[::3] (352,684
    points): the whole table equals sg_nearest_point's, the second in one brute-force call of 3.7e11 scores."""
    import torch
    from seggroup_amd import prepare, thin
    big = thin_ref.big_cloud()[0]
    assert big.shape[0] == 1058050 > 1 << 20
    d_big = torch.from_numpy(big).to(DEV)
    rep = thin.thin_cloud(d_big, 0.05, device=DEV)[0]
    assert rep.shape[0] == 5403
    for cand in (d_big[rep.long()].contiguous(), d_big[::3].contiguous()):
        idx, d2 = prepare.nearest_point_grid(d_big, cand, device=DEV)
        st = prepare.nearest_grid_stats()
        print(int(cand.shape[0]), st)
        want = prepare.get_unmapper(d_big, cand, device=DEV)
        assert torch.equal(idx, want)
        d = d_big - cand[want]
        assert torch.equal(d2, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        del idx, d2, want, d
    assert int(cand.shape[0]) == 352684


@pytest.mark.parametrize("name", ["prep_sub_3k", "prep_rep_1k", "prep_exact_2k"])
def test_get_unmapper_and_sample_points_opt_in(name):
    """index="grid" on the shapes of the tests/golden/prep_* fixtures: the same unmapper, the same sampled cloud"""
    from seggroup_amd import prepare, synthetic
    e = json.load(open(os.path.join(GOLDEN, "prep_index.json")))[name]
    scan = synthetic.make_raw_scan(e["w"], e["h"], e["seed"], name=name)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    pcl, unmap, missing = prepare.sample_points(scan.xyz, scan.rgb, g["map"], device=DEV, index="grid")
    assert missing == e["unsampled"]
    assert pcl.cpu().numpy().tobytes() == g["pcl"].tobytes() and np.array_equal(unmap.cpu().numpy(), g["unmap"])
    ref = prepare.sample_points(scan.xyz, scan.rgb, g["map"], device=DEV)
    assert np.array_equal(ref[1].cpu().numpy(), g["unmap"]) and ref[2] == missing
    miss = np.nonzero(np.bincount(g["map"], minlength=e["V"]) == 0)[0]
    x = scan.xyz[miss] if miss.size else scan.xyz
    default = prepare.get_unmapper(x, g["pcl"][:, :3], device=DEV)
    for cell in (None, 0.07):
        got = prepare.get_unmapper(x, g["pcl"][:, :3], device=DEV, index="grid", cell=cell)
        assert got.dtype == default.dtype and np.array_equal(got.cpu().numpy(), default.cpu().numpy())
    if miss.size:
        assert np.array_equal(default.cpu().numpy(), g["unmap"][miss])


@pytest.mark.parametrize("name", P.CASES)
def test_the_knn_grid_still_matches_the_committed_digests(name):
    """sg_pointcloud_knn_grid builds its index through the function the nearest-point search shares: its table, unchanged"""
    from seggroup_amd import prepare
    exp = P._expected()[name]
    for cell in (None, ONE_CELL):
        t = prepare.pointcloud_knn(P._cloud(name), 10, device=DEV, index="grid", cell=cell).cpu().numpy()
        assert R.array_digest(t, "<i4") == exp["knn"], f"{name}, cell = {cell}"


def test_stage_times_and_counted_scores():
    from seggroup_amd import hip, prepare
    lib = hip.lib()
    x, y = NG.case_pairs()["plain"]
    assert lib.sg_nearest_point_grid_set_timing(1) == hip.SG_OK
    try:
        got, _, st = _grid(x, y, cell=0.3)
    finally:
        lib.sg_nearest_point_grid_set_timing(0)
    us = (C.c_float * 8)()
    assert lib.sg_nearest_point_grid_stage_times(us, 8) == 7 and all(v >= 0 for v in us) and us[5] > 0
    _equal(got, _brute("plain"), "a timed call")
    assert 0 < st["scores"] < x.shape[0] * y.shape[0], "fewer pair scores than brute force"
