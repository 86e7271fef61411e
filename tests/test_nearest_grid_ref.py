"""The grid-indexed nearest point between two clouds, without a GPU: the NumPy statement of the rule
(tests/nearest_grid_ref.py) against the plain statement `brute` -- the first argmax of every row of pcseg_ref.pair_scores -- on the
pairs that each catch one mistake, the margin delta over the union of the two clouds, what the rule does WITHOUT the margin on the
three shifted rooms, and what the host decides before any device call."""
import ctypes as C

import numpy as np
import pytest

import knn_grid_ref as G
import nearest_grid_ref as NG
import pcseg_ref as R

SAMPLE = 1000                                   # queries of a pair that are searched (seeded, plus the last two: the outliers)
PAIRS = ["plain", "lattice", "dup", "all_equal", "half_room", "outliers", "shifted"]
# the ring limit: the library's, except on the shifted pair at the small cell, whose margin spans ten cells of 0.05 -- there the rule
# itself is what is being checked, so the rings run until they settle
LIMIT = {("shifted", 0.05): 40}
_want = {}


def _rows(n):
    if n <= SAMPLE:
        return np.arange(n)
    return np.union1d(np.random.RandomState(11).choice(n, SAMPLE, replace=False), [n - 2, n - 1])


def _brute(name):
    if name not in _want:
        x, y = NG.case_pairs()[name]
        _want[name] = NG.brute(x[_rows(x.shape[0])], y)
    return _want[name]


@pytest.mark.parametrize("name", PAIRS)
def test_the_statement_equals_brute_force(name):
    x, y = NG.case_pairs()[name]
    rows, want = _rows(x.shape[0]), _brute(name)
    for cell in NG.CELLS[name]:
        got, rings, grid = NG.nearest_grid(x, y, cell, ring_limit=LIMIT.get((name, cell), NG.RING_LIMIT), rows=rows)
        st = NG.stats_of(grid, rings)
        print(f"{name} h = {cell}: {st}, rings mean {rings.mean():.2f}, {int((got != want).sum())} rows wrong")
        assert np.array_equal(got, want), f"{name} h = {cell}: {int((got != want).sum())} of {rows.shape[0]} rows differ"
        assert np.array_equal(grid.whole, want)
        if name == "shifted":
            assert (rings > 0).all(), "the rings settled every query: the rule was exercised, not the queue"
        if name == "outliers":
            assert (rings[-2:] == 0).all() and (rings[:-2] > 0).all(), "the two outlying queries, and only they, end in the queue"
        if name == "half_room":
            assert rings.max() > 1, "queries outside the candidates' box walk more than one ring"
    if name == "all_equal":
        assert (want == 0).all()
    if name == "dup":
        assert (want <= rows).all(), "never a higher row than the query's own"
    if name == "lattice":
        s = R.pair_scores(x[rows[:256]], y)
        assert ((s == s.max(1, keepdims=True)).sum(1) > 1).any(), "a dropped lattice point has several equally good candidates"


def test_a_duplicate_maps_to_its_lowest_index():
    """room_dup against itself: 200 points are there twice; the higher twin's answer is the lower one, not its own row"""
    x, y = NG.case_pairs()["dup"]
    want = NG.brute(x, y)
    _, first = np.unique(x, axis=0, return_index=True)
    twins = np.setdiff1d(np.arange(x.shape[0]), first)
    assert twins.shape[0] == 200 and (want[twins] < twins).all() and np.array_equal(x[want], x)
    for cell in NG.CELLS["dup"]:
        got, rings, _ = NG.nearest_grid(x, y, cell, rows=twins)
        assert np.array_equal(got, want[twins]) and (rings > 0).all()


# rows wrong of 300 with delta = 0 at cells of (0.02, 0.05), counted here: the two-cloud, k = 1 numbers of DESIGN.md 8i
WITHOUT_DELTA = {G.SHIFTS[0]: (6, 0), G.SHIFTS[1]: (179, 65), G.SHIFTS[2]: (289, 271)}


@pytest.mark.parametrize("shift", G.SHIFTS)
def test_without_the_margin_the_shifted_rooms_go_wrong(shift):
    """delta = 0 -- the textbook rule Lb > -s_best -- stops too early on every one of the three shifts at a cell of 0.02, and on two of
    them at 0.05; with the margin the same rows are right.  Where a row cannot settle within 40 rings (the margin of the last shift
    spans more) the queue answers it."""
    room = R.case_clouds()["room_j5e-4"][0]
    x = G.shifted(room, shift)
    y = np.ascontiguousarray(x[::2])
    rows = np.sort(np.random.RandomState(13).choice(x.shape[0], 300, replace=False))
    want = NG.brute(x[rows], y)
    for cell, expected in zip((0.02, 0.05), WITHOUT_DELTA[shift]):
        naive, r0, _ = NG.nearest_grid(x, y, cell, ring_limit=40, rows=rows, delta=0.0)
        safe, r1, _ = NG.nearest_grid(x, y, cell, ring_limit=40, rows=rows)
        wrong = int((naive != want).sum())
        print(f"shift {shift} h = {cell}: {wrong} of 300 rows wrong without delta (rings mean {r0.mean():.1f}), "
              f"{int((safe != want).sum())} with it (rings mean {r1.mean():.1f})")
        assert (r0 > 0).all() and np.array_equal(safe, want)
        if expected:
            assert wrong >= 1, "wrong without"
        assert wrong == expected, "the count DESIGN.md 8i quotes"


@pytest.mark.parametrize("name", PAIRS)
def test_the_margin_bounds_the_scores_distance_from_minus_d2(name):
    """max |score + d2_float64| <= delta = 2^-19 max|p|^2 over the union, on every pair"""
    x, y = NG.case_pairs()[name]
    rows = _rows(x.shape[0])
    err, delta = NG.score_error(x[rows], y), float(NG.delta_of(x, y))
    m2 = max(float(G.m2_of(x)), float(G.m2_of(y)))
    print(f"{name}: max |score + d2| = {err:.3e} = {err / (2.0 ** -24 * m2 + 1e-300):.2f} u M2, delta = {delta:.3e}")
    assert err <= delta


def test_the_vector_test_is_8h_s_test():
    for r, h, slack, delta, s in ((1, 0.05, 1e-6, 0.25, -0.001), (11, 0.05, 1e-6, 0.25, -0.001), (2, 0.3, 0.0, 0.0, -0.2), (1, 1e-7, 1e-3, 0.0, -1.0)):
        assert bool(NG.settled(r, h, slack, delta, np.float32(s))) == G.settled(r, h, slack, delta, s)


def test_a_cell_outside_the_envelope_is_refused_by_the_statement_too():
    x, y = NG.case_pairs()["outliers"]
    with pytest.raises(G.CellRange):
        NG.Grid(x, y, 1e-9)
    with pytest.raises(G.CellRange):
        NG.Grid(x, y, 0.04)                                     # 401 x 226 x 226 cells over the union: beyond the table of 5,281 candidates


def test_unknown_index_names_are_value_errors():
    """decided before any device is touched"""
    from seggroup_amd import prepare, transfer
    x = R.case_clouds()["n255"][0]
    rgb = np.zeros(x.shape, np.uint8)
    for bad in ("kd", "GRID", None, 1):
        for call in (lambda: prepare.get_unmapper(x, x, index=bad), lambda: prepare.sample_points(x, rgb, np.arange(10), index=bad),
                     lambda: prepare.prepare_scene("/nowhere/scene0000_00", 0, index=bad), lambda: transfer.nearest_vertex(x, x, index=bad),
                     lambda: transfer.transfer_results("/nowhere", "/nowhere", "e", "s", "/nowhere", index=bad)):
            with pytest.raises(ValueError, match="index must be"):
                call()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell must be"):
            prepare.get_unmapper(x, x, index="grid", cell=bad)


def test_brute_is_refused_above_its_cap_and_names_the_grid():
    from seggroup_amd import hip, transfer
    src = np.zeros(((1 << 20) + 1, 3), np.float32)
    assert hip.MAX_POINTS == 1 << 20
    with pytest.raises(ValueError, match="--index grid"):
        transfer.nearest_vertex(src, src[:4], index="brute")


def test_the_envelope_is_decided_on_the_host(sg_lib):
    """the caps, the pointers, the strides, the cell and the workspace size need no GPU to be refused"""
    from seggroup_amd import hip
    cap_n, cap_u = 1 << 24, 1 << 27
    assert hip.MAX_GRID_POINTS == cap_n and hip.MAX_CLOUD_POINTS == cap_u
    ws = sg_lib.sg_nearest_point_grid_ws_bytes
    assert ws(5, cap_n + 1) == 0 and ws(5, 0) == 0 and ws(-1, 5) == 0 and ws(cap_u + 1, 5) == 0
    sizes = [ws(u, n) for u, n in ((0, 1), (1000, 1000), (1 << 20, 1 << 20), (cap_u, cap_n))]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] < 1 << 40
    assert ws(1000, 1000) >= sg_lib.sg_pointcloud_knn_grid_ws_bytes(1000, 10)
    buf = (C.c_int * 64)()
    p = C.addressof(buf)
    call = lambda x=p, xs=3, u=300, y=p, ys=3, n=300, cell=0.0, idx=p, d2=None, w=p, nb=1 << 30: sg_lib.sg_nearest_point_grid(   # noqa: E731
        x, xs, u, y, ys, n, cell, idx, d2, w, nb, None)
    assert call(n=cap_n + 1, x=None, y=None, idx=None, w=None, nb=0) == hip.SG_EUNSUP and b"at most" in sg_lib.sg_last_error()
    assert call(u=cap_u + 1) == hip.SG_EUNSUP and b"at most" in sg_lib.sg_last_error()
    assert call(n=0) == hip.SG_EINVAL and call(n=-3) == hip.SG_EINVAL and call(u=-1) == hip.SG_EINVAL
    assert call(x=None) == hip.SG_EINVAL and call(y=None) == hip.SG_EINVAL and call(idx=None) == hip.SG_EINVAL and call(w=None) == hip.SG_EINVAL
    assert call(xs=2) == hip.SG_EINVAL and call(ys=2) == hip.SG_EINVAL
    for cell in (-0.5, float("nan"), float("inf")):
        assert call(cell=cell) == hip.SG_EINVAL and b"cell edge" in sg_lib.sg_last_error()
    assert call(nb=ws(300, 300) - 1) == hip.SG_EINVAL and b"workspace too small" in sg_lib.sg_last_error()
    assert call(u=0, x=None, idx=None, w=None, nb=0) == hip.SG_OK, "no queries: nothing to do, nothing touched"
    stats = (C.c_int64 * 16)()
    assert sg_lib.sg_nearest_point_grid_stats(stats, 16) == 9 and not any(stats), "a refused call leaves no statistics"
    assert sg_lib.sg_nearest_point_grid_stats(stats, 4) == hip.SG_EINVAL
    names = [sg_lib.sg_nearest_point_grid_stage_name(i) for i in range(8)]
    assert names == [sg_lib.sg_pointcloud_knn_grid_stage_name(i) for i in range(8)] and names[5:] == [b"search", b"fallback", None]
    assert sg_lib.sg_nearest_point_grid_set_tuning(0, 65) == hip.SG_EINVAL and sg_lib.sg_nearest_point_grid_set_tuning(0, 0) == hip.SG_OK
    assert sg_lib.sg_nearest_point_grid_set_timing(0) == hip.SG_OK
