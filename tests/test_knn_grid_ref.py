"""The grid-indexed kNN's search rule, without a GPU: the NumPy statement (tests/knn_grid_ref.py) against the brute-force
statement pcseg_ref.knn_table -- the margin delta bounds the score's distance from -d^2 on every cloud, the search with the margin
reproduces the table whatever the cell, the same search WITHOUT the margin gets rows wrong on the shifted room (that cloud is why the
margin exists), the tie rule by original index -- and what the host decides before any device call: the index names, --index on a mesh,
the cap, the arguments."""
import ctypes as C
import os

import numpy as np
import pytest

import knn_grid_ref as G
import pcseg_ref as R

SAMPLE = 1000                                   # rows of a room that are searched (seeded); the small clouds are searched whole
_clouds = {}


def _cloud(name):
    if not _clouds:
        _clouds.update({k: v[0] for k, v in R.case_clouds().items()})
        room = _clouds["room_j5e-4"]
        for s in G.SHIFTS:
            _clouds["room_j5e-4+(%g,%g,%g)" % s] = G.shifted(room, s)
        _clouds["room_j5e-4+outliers"] = G.with_outliers(room)
    return _clouds[name]


MARGIN_CLOUD = "room_j5e-4+(%g,%g,%g)" % G.MARGIN_SHIFT
BASE = ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup", "n_k_plus_1", "n255", "n256", "n257", "line", "all_equal"]
SHIFTED = ["room_j5e-4+(%g,%g,%g)" % s for s in G.SHIFTS]
# two forced cells per cloud: one that leaves (nearly) every point alone in its cell, one of many points per cell
CELLS = {name: (0.04, 0.3) for name in BASE}
CELLS.update({"line": (0.07, 0.5), MARGIN_CLOUD: (0.05, 0.3), "room_j5e-4+outliers": (0.1, 0.5)})
# the ring limit: the library's, except on the shifted room, whose margin spans ten cells of 0.05 -- there the rule itself is what is
# being checked, so the rings run until they settle
LIMIT = {MARGIN_CLOUD: 40}


def _rows(name, n):
    if n <= SAMPLE:
        return np.arange(n)
    return np.union1d(np.random.RandomState(11).choice(n, SAMPLE, replace=False), [n - 2, n - 1])      # the outliers are the last two


@pytest.mark.parametrize("name", BASE + SHIFTED)
def test_the_margin_bounds_the_scores_distance_from_minus_d2(name):
    """(a) max |score + d2_float64| <= delta = 2^-19 max|p|^2 on every cloud; on the shifted rooms the error is a few u M2, far above any
    squared distance between neighbours"""
    x = _cloud(name)
    err, delta = G.score_error(x), float(G.delta_of(x))
    print(f"{name}: max |score + d2| = {err:.3e} = {err / (2.0 ** -24 * float(G.m2_of(x)) + 1e-300):.2f} u M2, delta = {delta:.3e}")
    assert err <= delta


@pytest.mark.parametrize("name", BASE + [MARGIN_CLOUD, "room_j5e-4+outliers"])
def test_the_search_reproduces_the_brute_force_table(name):
    """(b) the statement's table equals knn_table for two forced cells; the small cell walks more than one ring"""
    x = _cloud(name)
    rows = _rows(name, x.shape[0])
    want = G.brute_rows(x, rows)
    if rows.shape[0] == x.shape[0]:
        assert np.array_equal(want, R.knn_table(x))
    for cell in CELLS[name]:
        got, rings, grid = G.knn_table_grid(x, 10, cell, ring_limit=LIMIT.get(name, G.RING_LIMIT), rows=rows)
        bad = (got != want).any(1)
        print(f"{name} h = {cell}: cells {grid.nc.tolist()}, largest {grid.largest_cell()}, rings max {rings.max()} mean {rings.mean():.2f}, "
              f"{int((rings == 0).sum())} by the whole cloud, {int(bad.sum())} rows wrong")
        assert not bad.any(), f"{name} h = {cell}: {int(bad.sum())} of {rows.shape[0]} rows differ, first {rows[bad][:5].tolist()}"
        if name == MARGIN_CLOUD:
            assert (rings > 0).all(), "the rings settled every row: the rule was exercised, not the fallback"
        if name == "room_j5e-4+outliers":
            assert (rings[-2:] == 0).all() and (rings[:-2] > 0).all(), "the two outliers, and only they, are finished against the whole cloud"


@pytest.mark.parametrize("cell", [0.02, 0.05])
def test_without_the_margin_the_shifted_room_goes_wrong(cell):
    """(c) delta = 0 -- the textbook rule Lb > -s_kth -- stops too early: the scores of this cloud carry an error of ~0.03, the squared
    spacing is 0.0025.  With the margin the same rows are right."""
    x = _cloud(MARGIN_CLOUD)
    rows = np.sort(np.random.RandomState(13).choice(x.shape[0], 300, replace=False))
    want = G.brute_rows(x, rows)
    naive, r0, _ = G.knn_table_grid(x, 10, cell, ring_limit=40, rows=rows, delta=0.0)
    safe, r1, _ = G.knn_table_grid(x, 10, cell, ring_limit=40, rows=rows)
    wrong = int((naive != want).any(1).sum())
    print(f"h = {cell}: {wrong} of {rows.shape[0]} rows wrong without delta (rings mean {r0.mean():.1f}), "
          f"{int((safe != want).any(1).sum())} with it (rings mean {r1.mean():.1f})")
    assert wrong >= 1 and (r0 > 0).all()
    assert np.array_equal(safe, want) and (r1 > 0).all()


def test_ties_go_by_original_index():
    """(d) one point 32 times: every list is 0..10; room_dup: of two coincident points the lower index comes first in both rows, although
    the grid meets them in cell order"""
    x = _cloud("all_equal")
    for cell in (0.04, 7.0):
        got, _, _ = G.knn_table_grid(x, 10, cell)
        assert np.array_equal(got, np.tile(np.arange(11, dtype=np.int32), (32, 1)))
    x = _cloud("room_dup")
    _, inv, cnt = np.unique(x, axis=0, return_inverse=True, return_counts=True)
    twins = np.flatnonzero(cnt[inv.reshape(-1)] > 1)
    assert twins.shape[0] == 400
    want = G.brute_rows(x, twins)
    for cell in (0.04, 0.3):
        got, rings, _ = G.knn_table_grid(x, 10, cell, rows=twins)
        assert np.array_equal(got, want) and (rings > 0).all()
    by_point = {}
    for i in twins:
        by_point.setdefault(int(inv.reshape(-1)[i]), []).append(int(i))
    for n, i in enumerate(twins):
        a, b = sorted(by_point[int(inv.reshape(-1)[i])])
        row = got[n].tolist()
        assert a in row and b in row and row.index(a) + 1 == row.index(b), "equal scores: the lower index directly before the higher"


def test_a_cell_outside_the_envelope_is_refused_by_the_statement_too():
    with pytest.raises(G.CellRange):
        G.Grid(_cloud("line"), 1e-9)                            # an axis of 2^21 cells or more
    with pytest.raises(G.CellRange):
        G.Grid(_cloud("line"), 0.04)                            # 198 x 394 x 99 cells: more than the table of 64 points holds


def test_unknown_index_names_are_value_errors():
    """(e) decided before any device is touched"""
    from seggroup_amd import hip, oversegment, prepare
    x = _cloud("n255")
    for bad in ("kd", "GRID", None, 1):
        for call in (lambda: prepare.pointcloud_knn(x, 10, index=bad), lambda: oversegment.pointcloud_edges(x, index=bad),
                     lambda: oversegment.segment_pointcloud(x, index=bad), lambda: oversegment.oversegment_scan("/nowhere/scene0000_00", index=bad),
                     lambda: oversegment.oversegment_scans("/nowhere", scenes=[], index=bad)):
            with pytest.raises(ValueError, match="index must be"):
                call()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell must be"):
            prepare.pointcloud_knn(x, 10, index="grid", cell=bad)
    assert hip.knn_index("brute") == hip.KNN_BRUTE == 0 and hip.knn_index("grid") == hip.KNN_GRID == 1


def test_index_grid_on_a_mesh_is_an_argparse_error(tmp_path, capsys):
    """(e) --index grid without --pointcloud on a scan that has faces: refused by the parser before any work, like --voxel"""
    from seggroup_amd import oversegment, prepare
    name = "scene0045_00"
    os.makedirs(tmp_path / name)
    x = _cloud("n255")
    faces = np.arange(9, dtype=np.int32).reshape(3, 3)
    prepare.write_ply(str(tmp_path / name / (name + "_vh_clean_2.ply")), x, np.zeros(x.shape, np.uint8), faces)
    with pytest.raises(SystemExit) as ei:
        oversegment.main(["--scans", str(tmp_path), "--index", "grid"])
    err = capsys.readouterr().err
    assert ei.value.code == 2 and "--pointcloud" in err and "--index grid" in err
    with pytest.raises(SystemExit) as ei:
        oversegment.main(["--scans", str(tmp_path), "--index", "octree"])
    assert ei.value.code == 2
    assert not os.path.exists(tmp_path / name / oversegment.segs_json_name(name))
    with pytest.raises(ValueError, match="point-cloud path"):
        oversegment.oversegment_scan(str(tmp_path / name), index="grid")


def test_the_envelope_is_decided_on_the_host(sg_lib):
    """(f) the cap, k, N <= k, null pointers, the cell and the workspace size need no GPU to be refused"""
    from seggroup_amd import hip
    cap = 1 << 24
    assert hip.MAX_GRID_POINTS == cap
    assert sg_lib.sg_pointcloud_knn_grid_ws_bytes(cap + 1, 10) == 0 and sg_lib.sg_pointcloud_knn_grid_ws_bytes(0, 10) == 0
    assert sg_lib.sg_pointcloud_knn_grid_ws_bytes(5000, 7) == 0
    assert sg_lib.sg_pcseg_ws_bytes_indexed(cap + 1, 10, hip.KNN_GRID) == 0 and sg_lib.sg_pcseg_ws_bytes_indexed(5000, 10, 2) == 0
    # the arithmetic at the cap stays in range: the sizes grow with N and the indexed size holds the brute-force one and the grid's
    sizes = [sg_lib.sg_pointcloud_knn_grid_ws_bytes(n, 20) for n in (1 << 20, 1 << 22, cap)]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < 1 << 40
    for n, k in ((5000, 10), (cap, 20)):
        assert sg_lib.sg_pcseg_ws_bytes_indexed(n, k, hip.KNN_BRUTE) == sg_lib.sg_pcseg_ws_bytes(n, k)
        both = sg_lib.sg_pcseg_ws_bytes(n, k) + sg_lib.sg_pointcloud_knn_grid_ws_bytes(n, k)
        assert both <= sg_lib.sg_pcseg_ws_bytes_indexed(n, k, hip.KNN_GRID) < both + 4096
    assert cap * 20 < 2 ** 31, "N * k of the segmenter's edge stages is an int"
    buf = (C.c_int * 64)()
    p = C.addressof(buf)
    call = lambda pts=p, stride=3, n=300, k=10, cell=0.0, out=p, ws=p, nb=1 << 30: sg_lib.sg_pointcloud_knn_grid(   # noqa: E731
        pts, stride, n, k, cell, out, ws, nb, None)
    assert call(n=cap + 1, pts=None, out=None, ws=None, nb=0) == hip.SG_EUNSUP and b"at most" in sg_lib.sg_last_error()
    assert call(k=7) == hip.SG_EUNSUP
    assert call(n=10) == hip.SG_EINVAL and b"points for k =" in sg_lib.sg_last_error()
    assert call(pts=None) == hip.SG_EINVAL and call(out=None) == hip.SG_EINVAL and call(ws=None) == hip.SG_EINVAL and call(stride=2) == hip.SG_EINVAL
    for cell in (-0.5, float("nan"), float("inf")):
        assert call(cell=cell) == hip.SG_EINVAL and b"cell edge" in sg_lib.sg_last_error()
    need = sg_lib.sg_pointcloud_knn_grid_ws_bytes(300, 10)
    assert call(nb=need - 1) == hip.SG_ENOMEM and b"workspace too small" in sg_lib.sg_last_error()
    stats = (C.c_int64 * 16)()
    assert sg_lib.sg_pointcloud_knn_grid_stats(stats, 16) == 9 and not any(stats), "a refused call leaves no statistics"
    assert sg_lib.sg_pointcloud_knn_grid_stats(stats, 4) == hip.SG_EINVAL
    names = [sg_lib.sg_pointcloud_knn_grid_stage_name(i) for i in range(8)]
    assert names == [b"box", b"probe", b"cells", b"sort", b"table", b"search", b"fallback", None]
    assert sg_lib.sg_pointcloud_knn_grid_set_tuning(0, 65) == hip.SG_EINVAL and sg_lib.sg_pointcloud_knn_grid_set_tuning(0, 0) == hip.SG_OK
