"""The exact k nearest candidates between two clouds and the vote over them on the GPU: sg_cloud_knn_cross_grid's rows
EQUAL to the plain statement (tests/knn_cross_ref.brute: the first k columns of a stable descending sort of the score row) on the pairs
that each catch one mistake, at two forced cells and at the library's; column 0 and its d2 equal to sg_nearest_point_grid's; the wave
and tile edges, N = k, a cell larger than a staged tile, strides, d2 = NULL; two streams and two cells; every refusal; the two query
policies of the one search kernel against each other (knn_cross_grid(x, x) and the self-kNN); every query of all three entry points
through the queue at its block edges; sg_knn_vote against the NumPy rule; and `transfer --vote` on a two-scene tree."""
import json
import os

import numpy as np
import pytest

import knn_cross_ref as KC
import knn_grid_ref as G
import nearest_grid_ref as NG
import pcseg_ref as R
import test_knn_cross_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = T.PAIRS
_rooms = {}


def _cross(x, y, k, cell=None, **kw):
    from seggroup_amd import prepare
    knn, d2 = prepare.knn_cross_grid(x, y, k, cell=cell, device=DEV, **kw)
    return knn.cpu().numpy(), (d2.cpu().numpy() if d2 is not None else None), prepare.knn_cross_stats()


def _equal(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    bad = (got != want).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first {np.flatnonzero(bad)[:3].tolist()}: " \
                          f"{got[bad][:3].tolist()} != {want[bad][:3].tolist()}"


def _big():
    if "big" not in _rooms:
        _rooms["big"] = R.case_clouds(include_large=True)["room_20k"][0]
    return _rooms["big"]


@pytest.mark.parametrize("k", KC.KS)
@pytest.mark.parametrize("name", PAIRS)
def test_rows_equal_brute_force_at_every_cell(name, k):
    """all queries searched, the sampled rows held to the statement; the library's cell also against sg_nearest_point_grid on ALL rows"""
    from seggroup_amd import prepare
    x, y = NG.case_pairs()[name]
    rows, want = T._rows(x.shape[0]), T._brute(name)[:, :k]
    got, d2, st = _cross(x, y, k, want_d2=True)
    print(f"{name} k = {k} default: {st}")
    _equal(got[rows], want, f"{name}, k = {k}, the library's cell")
    assert d2.dtype == np.float32 and d2.shape == got.shape and d2.tobytes() == KC.d2_of(x, y, got).tobytes(), "d2 bit for bit"
    idx, nd2 = prepare.nearest_point_grid(x, y, device=DEV)
    assert np.array_equal(got[:, 0].astype(np.int64), idx.cpu().numpy()), "column 0 is sg_nearest_point_grid's index"
    assert np.ascontiguousarray(d2[:, 0]).tobytes() == nd2.cpu().numpy().tobytes(), "and its d2"
    assert st["cell"] > 0 and st["occupied"] >= 1
    for n, cell in enumerate(NG.CELLS[name]):
        forced, _, st = _cross(x, y, k, cell=cell)
        print(f"{name} k = {k} h = {cell}: {st}")
        _equal(forced[rows], want, f"{name}, k = {k}, cell = {cell}")
        assert forced.tobytes() == got.tobytes(), "every row, whatever the cell"
        assert st["cell"] == np.float32(cell)
        if n == 0 and name in ("outliers", "half_room"):
            assert 0 < st["fallback"] < x.shape[0], "queries the rings cannot settle: the fallback kernel wrote their rows"


U_EDGES = [1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("u", U_EDGES)
def test_the_wave_and_tile_edges_of_the_queries(u):
    """the LAST u points of room_20k against its first 300, at k = 20 (and k = 5 at the wave edge), three cells each"""
    big = _big()
    x, y = np.ascontiguousarray(big[-u:]), np.ascontiguousarray(big[:300])
    for k in ((20, 5) if u == 65 else (20,)):
        want = KC.brute(x, y, k)
        for cell in (None, 0.2, 1000.0):
            got, d2, st = _cross(x, y, k, cell=cell, want_d2=True)
            _equal(got, want, f"U = {u}, k = {k}, cell = {cell}")
            assert d2.tobytes() == KC.d2_of(x, y, want).tobytes()
        assert st["cells"] == (1, 1, 1) and st["largest_cell"] == 300 and st["fallback"] == 0


def test_as_many_candidates_as_neighbours():
    """N = k: every row is the whole candidate cloud in score order"""
    big = _big()
    x = np.ascontiguousarray(big[-257:])
    for k in (20, 5):
        y = np.ascontiguousarray(big[:k])
        want = KC.brute(x, y, k)
        assert (np.sort(want, 1) == np.arange(k)[None, :]).all()
        for cell in (None, 0.05):
            got, _, st = _cross(x, y, k, cell=cell)
            _equal(got, want, f"N = k = {k}, cell = {cell}")


def test_a_cell_larger_than_a_tile():
    big = _big()
    x, y = np.ascontiguousarray(big[1::2][:600]), np.ascontiguousarray(big[::2])
    want = KC.brute(x, y, 20)
    got, d2, st = _cross(x, y, 20, cell=0.5, want_d2=True)
    print(st)
    _equal(got, want, "room_20k halves, cell = 0.5")
    assert st["largest_cell"] > 256 and st["largest_cell"] == NG.Grid(x, y, 0.5).largest_cell()
    assert d2.tobytes() == KC.d2_of(x, y, want).tobytes()


def test_strides_and_no_d2():
    """candidate rows of 6 floats, query rows of 4; d2 = NULL is accepted"""
    x, y = NG.case_pairs()["plain"]
    rng = np.random.RandomState(3)
    x4 = np.ascontiguousarray(np.concatenate([x, rng.standard_normal((x.shape[0], 1)).astype(np.float32)], 1))
    y6 = np.ascontiguousarray(np.concatenate([y, rng.standard_normal((y.shape[0], 3)).astype(np.float32)], 1))
    rows, want = T._rows(x.shape[0]), T._brute("plain")
    for cell in (None, 0.04):
        got, d2, _ = _cross(x4, y6, 20, cell=cell, want_d2=True)
        _equal(got[rows], want, f"strides 4 / 6, cell = {cell}")
        assert d2.tobytes() == KC.d2_of(x, y, got).tobytes()
        bare, none, _ = _cross(x4, y6, 20, cell=cell)
        assert none is None and bare.tobytes() == got.tobytes(), "d2 = NULL"


@pytest.mark.parametrize("name", ["dup", "half_room"])
def test_two_streams_and_two_cells_give_identical_bytes(name):
    import torch
    x, y = NG.case_pairs()[name]
    for k in (20, 5):
        a = _cross(x, y, k, want_d2=True)
        b = _cross(x, y, k, want_d2=True, stream=torch.cuda.Stream(device=DEV))
        c = _cross(x, y, k, want_d2=True, cell=0.11, stream=torch.cuda.Stream(device=DEV))
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
                prepare.knn_cross_grid(xx, yy, 10, device=DEV)
            assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    yy = y.copy()
    yy[3] = (1e19, -1e19, 1e19)
    with pytest.raises(hip.SgError) as ei:
        prepare.knn_cross_grid(x, yy, 10, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "brute-force path" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        prepare.knn_cross_grid(x, y, 10, cell=1e-9, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "cell too small" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        prepare.knn_cross_grid(x, y, 10, cell=0.005, device=DEV)
    assert ei.value.code == hip.SG_EUNSUP and "table" in str(ei.value)
    for k, n, code in ((10, 9, hip.SG_EINVAL), (20, 19, hip.SG_EINVAL), (5, 0, hip.SG_EINVAL), (7, 100, hip.SG_EUNSUP), (1, 100, hip.SG_EUNSUP)):
        with pytest.raises(hip.SgError) as ei:
            prepare.knn_cross_grid(x, y[:n], k, device=DEV)
        assert ei.value.code == code, (k, n)
    knn, d2 = prepare.knn_cross_grid(x[:0], y, 10, device=DEV, want_d2=True)
    assert tuple(knn.shape) == (0, 10) and tuple(d2.shape) == (0, 10) and knn.dtype == torch.int32
    lib = hip.lib()
    u, n, k = x.shape[0], y.shape[0], 10
    cap_n, cap_u = hip.MAX_GRID_POINTS, hip.MAX_CLOUD_POINTS
    ws_bytes = lib.sg_cloud_knn_cross_grid_ws_bytes
    assert ws_bytes(u, cap_n + 1, k) == 0 and ws_bytes(cap_u + 1, n, k) == 0 and ws_bytes(-1, n, k) == 0 and ws_bytes(u, k - 1, k) == 0
    assert ws_bytes(u, n, 7) == 0 and ws_bytes(cap_u, n, 20) == 0
    d_x, d_y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = torch.full((u, k), -7, dtype=torch.int32, device=DEV)
    need = ws_bytes(u, n, k)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    call = lambda uu=u, nn=n, kk=k, nb=need, xs=3, ys=3, cell=0.0, px=d_x.data_ptr(), py=d_y.data_ptr(), po=out.data_ptr(), pw=ws.data_ptr(): \
        lib.sg_cloud_knn_cross_grid(px, xs, uu, py, ys, nn, kk, cell, po, None, pw, nb, None)                    # noqa: E731
    assert call(nb=need - 1) == hip.SG_EINVAL and b"workspace too small" in lib.sg_last_error()
    assert call(kk=6) == hip.SG_EUNSUP and call(kk=0) == hip.SG_EUNSUP and call(kk=21) == hip.SG_EUNSUP
    assert call(nn=k - 1) == hip.SG_EINVAL and call(nn=0) == hip.SG_EINVAL and call(uu=-1) == hip.SG_EINVAL
    assert call(nn=cap_n + 1) == hip.SG_EUNSUP and call(uu=cap_u + 1) == hip.SG_EUNSUP
    assert call(uu=(2 ** 31 - 1) // 20 + 1, kk=20) == hip.SG_EUNSUP and b"entries" in lib.sg_last_error()
    assert call(xs=2) == hip.SG_EINVAL and call(ys=2) == hip.SG_EINVAL
    assert call(px=None) == hip.SG_EINVAL and call(py=None) == hip.SG_EINVAL and call(po=None) == hip.SG_EINVAL and call(pw=None) == hip.SG_EINVAL
    for cell in (-0.5, float("nan"), float("inf")):
        assert call(cell=cell) == hip.SG_EINVAL and b"cell edge" in lib.sg_last_error()
    assert call(uu=0) == hip.SG_OK
    torch.cuda.synchronize()
    assert (out == -7).all(), "nothing was touched"
    assert call() == hip.SG_OK
    torch.cuda.synchronize()
    rows = T._rows(u)
    assert np.array_equal(out.cpu().numpy()[rows], T._brute("plain")[:, :k])


def test_stage_times_and_counted_scores():
    from seggroup_amd import hip
    x, y = NG.case_pairs()["plain"]
    with hip.stage_timer("cloud_knn_cross_grid") as t:
        got, _, st = _cross(x, y, 10, cell=0.3)
        us = t.read()
    assert t.names == ["box", "probe", "cells", "sort", "table", "search", "fallback"] and all(v >= 0 for v in us) and us[5] > 0
    _equal(got[T._rows(x.shape[0])], T._brute("plain")[:, :10], "a timed call")
    assert 0 < st["scores"] < x.shape[0] * y.shape[0], "fewer pair scores than brute force"


# ---- one search kernel under two query policies, one queue kernel ----------------------------------------------------------------
def _tiny_cloud(n, k, dup=False):
    rng = np.random.default_rng(1000 * k + n)
    if dup:                                                     # every point twice: equal scores, the lower index first
        half = rng.random((n // 2, 3)).astype(np.float32)
        return np.ascontiguousarray(np.concatenate([half, half], 0))
    return np.ascontiguousarray(rng.random((n, 3)).astype(np.float32))


@pytest.mark.parametrize("k", KC.KS)
def test_the_two_query_policies_agree(k):
    """knn_cross_grid(x, x, k) and the self-kNN's first k columns are the first columns of the same stable sort of the same score row:
    equal as integers at every size, with every point duplicated, at a cell of several rings and at one cell over the cloud"""
    from seggroup_amd import oversegment, prepare
    clouds = [(f"N = {n}", _tiny_cloud(n, k)) for n in (k + 1, 63, 64, 65, 257)] + [("dup, N = 130", _tiny_cloud(130, k, dup=True))]
    for what, x in clouds:
        want = KC.brute(x, x, k)
        for cell in (0.1, 1000.0):
            own = prepare.pointcloud_knn(x, k, device=DEV, index="grid", cell=cell).cpu().numpy()
            st_own = oversegment.knn_grid_stats()
            cross, _, st = _cross(x, x, k, cell=cell)
            assert own.dtype == np.int32 and own.shape == (x.shape[0], k + 1)
            _equal(cross, np.ascontiguousarray(own[:, :k]), f"{what}, k = {k}, cell = {cell}: the two-cloud rows against the self-kNN's")
            _equal(cross, want, f"{what}, k = {k}, cell = {cell}: against the plain statement")
            assert st["cells"] == st_own["cells"] and st["cell"] == st_own["cell"] == np.float32(cell)
            if cell == 0.1 and x.shape[0] == 257:
                assert st["max_ring"] > 1 and st_own["max_ring"] > 1, "several rings"
        assert st["cells"] == (1, 1, 1) and st["fallback"] == 0


LATTICE_CELL = 0.01


def _lattice():
    """7 x 7 x 7 candidates of spacing 0.1, and the queries half a spacing off on every axis: at a cell of 0.01 a ring-1 block (0.03 wide)
    holds one candidate at most round a candidate and none round a query"""
    if "lattice" not in _rooms:
        a = (np.arange(7) * 0.1).astype(np.float32)
        y = np.ascontiguousarray(np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3))
        _rooms["lattice"] = (np.ascontiguousarray(y + np.float32(0.05)), y)
    return _rooms["lattice"]


class _ring_limit_one:
    """set_tuning(0, 1) for the three entry points, the defaults again afterwards whatever happens"""

    FAMILIES = ("pointcloud_knn_grid", "nearest_point_grid", "cloud_knn_cross_grid")

    def _set(self, limit):
        from seggroup_amd import hip
        for f in self.FAMILIES:
            assert getattr(hip.lib(), f"sg_{f}_set_tuning")(0, limit) == hip.SG_OK

    def __enter__(self):
        self._set(1)

    def __exit__(self, *exc):
        self._set(0)


QUEUE_EDGES = [1, 255, 256, 257]


@pytest.mark.parametrize("u", QUEUE_EDGES)
def test_every_query_through_the_queue_two_clouds(u):
    """ring limit 1: no list fills and the one-entry search sees no candidate, so every row is the queue kernel's (the nearest point:
    sg_nearest_point's kernel) -- at one query, and one block of 256 less one, full, and one more"""
    from seggroup_amd import prepare
    shifted, y = _lattice()
    x = np.ascontiguousarray(shifted[:u])
    want1, rings, _ = NG.nearest_grid(x, y, LATTICE_CELL, ring_limit=1)
    assert (rings == 0).all() and np.array_equal(want1, NG.brute(x, y)), "the statement queues every query"
    with _ring_limit_one():
        idx, d2 = prepare.nearest_point_grid(x, y, cell=LATTICE_CELL, device=DEV)
        st = prepare.nearest_grid_stats()
        assert st["fallback"] == u and st["max_ring"] == 0, st
        idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
        assert idx.dtype == np.int64 and np.array_equal(idx, want1)
        assert d2.dtype == np.float32 and d2.tobytes() == NG.d2_of(x, y, want1).tobytes(), "d2 bit for bit"
        for k in KC.KS:
            want, rings, grid = KC.knn_cross_grid(x, y, k, LATTICE_CELL, ring_limit=1)
            assert (rings == 0).all() and np.array_equal(want, grid.whole) and np.array_equal(want, KC.brute(x, y, k))
            got, d2, st = _cross(x, y, k, cell=LATTICE_CELL, want_d2=True)
            assert st["fallback"] == u and st["max_ring"] == 0, (k, st)
            _equal(got, want, f"U = {u}, k = {k}: the queue's rows")
            assert d2.dtype == np.float32 and d2.tobytes() == KC.d2_of(x, y, want).tobytes(), "d2 bit for bit"
            assert np.array_equal(got[:, 0].astype(np.int64), want1)


@pytest.mark.parametrize("n", [255, 256, 257, 343])
def test_every_query_through_the_queue_self(n):
    """the self-kNN on the first n lattice points: a ring-1 block holds the point alone, a list of k + 1 never fills"""
    from seggroup_amd import oversegment, prepare
    x = np.ascontiguousarray(_lattice()[1][:n])
    with _ring_limit_one():
        for k in KC.KS:
            want, rings, _ = G.knn_table_grid(x, k, LATTICE_CELL, ring_limit=1)
            assert (rings == 0).all() and np.array_equal(want, G.brute_rows(x, np.arange(n), k)), "the statement queues every point"
            got = prepare.pointcloud_knn(x, k, device=DEV, index="grid", cell=LATTICE_CELL).cpu().numpy()
            st = oversegment.knn_grid_stats()
            assert st["fallback"] == n and st["max_ring"] == 0, (k, st)
            _equal(got, want, f"N = {n}, k = {k}: the queue's rows")


# ---- the vote ---------------------------------------------------------------------------------------------------------------------
def _vote(knn, labels, **kw):
    from seggroup_amd import transfer
    return tuple(t.cpu().numpy() for t in transfer.vote(knn, labels, device=DEV, **kw))


@pytest.mark.parametrize("name", PAIRS)
def test_the_vote_equals_the_rule(name):
    x, y = NG.case_pairs()[name]
    labels = KC.labels_of(y)
    for k in KC.KS:
        knn = _cross(x, y, k)[0]
        got, want = _vote(knn, labels), KC.vote(knn, labels)
        for g, w, what in zip(got, want, ("winner", "rep", "count", "tied")):
            assert g.dtype == np.int32 and np.array_equal(g, w), f"{name} k = {k}: {what}"
        if name != "all_equal":
            assert want[3].mean() >= 0.01 and (want[1] != knn[:, 0]).mean() >= 0.05


@pytest.mark.parametrize("k", [1, 2, 3, 5, 6, 10, 11, 19, 20, 21, 31, 32])
def test_the_vote_at_every_row_length(k):
    """rows that are not search results: repeated neighbours, few labels (many ties), the extreme int32 values as labels"""
    import torch
    rng = np.random.default_rng(k)
    labels = rng.choice(np.array([-2 ** 31, -1, 0, 1, 7, 2 ** 31 - 1], np.int64), 97).astype(np.int32)
    knn = rng.integers(0, 97, (1031, k)).astype(np.int32)
    want = KC.vote(knn, labels)
    for g, w in zip(_vote(knn, labels), want):
        assert np.array_equal(g, w)
    for g, w in zip(_vote(knn, labels, stream=torch.cuda.Stream(device=DEV)), want):
        assert np.array_equal(g, w)
    if k == 1:
        assert np.array_equal(want[1], knn[:, 0]) and (want[2] == 1).all() and not want[3].any()
    else:
        assert want[3].any() and not want[3].all()


def test_the_vote_refuses_an_index_outside_the_labels_and_takes_null_outputs():
    import torch
    from seggroup_amd import hip, transfer
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 9, 50).astype(np.int32)
    knn = rng.integers(0, 50, (300, 10)).astype(np.int32)
    want = KC.vote(knn, labels)
    for bad in (50, -1, 2 ** 31 - 1):
        wrong = knn.copy()
        wrong[257, 9] = bad
        with pytest.raises(ValueError, match="outside 0..49"):
            transfer.vote(wrong, labels, device=DEV)
    lib = hip.lib()
    d_knn, d_lab = torch.from_numpy(knn).to(DEV), torch.from_numpy(labels).to(DEV)
    out = torch.full((4, 300), -7, dtype=torch.int32, device=DEV)
    p = [out[i].data_ptr() for i in range(4)]
    assert lib.sg_knn_vote(d_knn.data_ptr(), 300, 10, d_lab.data_ptr(), 50, p[0], p[1], None, None, None) == hip.SG_OK
    got = out.cpu().numpy()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[2:] == -7).all()
    assert lib.sg_knn_vote(d_knn.data_ptr(), 300, 10, d_lab.data_ptr(), 50, p[0], p[1], p[2], None, None) == hip.SG_OK
    assert lib.sg_knn_vote(d_knn.data_ptr(), 300, 10, d_lab.data_ptr(), 50, p[0], p[1], None, p[3], None) == hip.SG_OK
    got = out.cpu().numpy()
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert lib.sg_knn_vote(d_knn.data_ptr(), 300, 10, d_lab.data_ptr(), 49, p[0], p[1], None, None, None) == hip.SG_EINVAL
    assert lib.sg_knn_vote(d_knn.data_ptr(), 300, 33, d_lab.data_ptr(), 50, p[0], p[1], None, None, None) == hip.SG_EINVAL
    assert lib.sg_knn_vote(d_knn.data_ptr(), 0, 10, d_lab.data_ptr(), 50, None, None, None, None, None) == hip.SG_OK


# ---- transfer --vote --------------------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    """two scenes; the source carries a .sgl whose segments are the label blocks of labels_of and a loose final.sem.npy, the target is the
    source's [::2] plus jitter"""
    from seggroup_amd import pseudo_labels
    rooms = R.case_clouds()
    a, b, root = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "root")
    made = {}
    rng = np.random.RandomState(8)
    for scene, room in (("scene0071_00", "room_j5e-4"), ("scene0072_00", "room_j2e-3")):
        src = rooms[room][0]
        dst = np.ascontiguousarray((src[::2] + (rng.standard_normal(src[::2].shape) * 0.004).astype(np.float32)).astype(np.float32))
        for tree, xyz in ((a, src), (b, dst)):
            os.makedirs(os.path.join(tree, scene))
            R.write_vertex_only_ply(os.path.join(tree, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))
        sov = np.unique(KC.labels_of(src), return_inverse=True)[1].astype(np.int32)
        tables = rng.randint(-1, 40, (14, int(sov.max()) + 1)).astype(np.int32)
        loose = rng.randint(0, 40, src.shape[0]).astype(np.int32)
        d = os.path.join(root, "results", "e", scene, "epoch_last")
        os.makedirs(d)
        pseudo_labels.write(d, tables, sov)
        np.save(os.path.join(d, "final.sem.npy"), loose)
        made[scene] = (src, dst, tables, sov, loose)
    return a, b, root, made


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if not n.endswith(".npz")}


def test_transfer_with_a_vote(tmp_path):
    from seggroup_amd import pseudo_labels, transfer
    a, b, root, made = _tree(tmp_path)
    base = ["--from-scans", a, "--to-scans", b, "-n", "e", "--root", root, "--workers", "2", "--device", DEV]
    plain = []
    for n in (0, 1):
        out = str(tmp_path / f"plain{n}")
        assert transfer.main(base + ["--out", out]) == 0
        plain.append(out)
    voted = str(tmp_path / "voted")
    assert transfer.main(base + ["--out", voted, "--vote", "10"]) == 0
    on_ins = str(tmp_path / "on_ins")
    assert transfer.main(base + ["--out", on_ins, "--vote", "5", "--vote-on", "final.ins"]) == 0
    report = json.load(open(os.path.join(voted, transfer.REPORT_NAME)))
    assert sorted(report["scenes"]) == sorted(made) and report["missing"] == {}
    for scene, (src, dst, tables, sov, loose) in made.items():
        sub = os.path.join("results", "e", scene, "epoch_last")
        knn = KC.brute(dst, src, 10)
        nearest = NG.brute(dst, src)
        assert np.array_equal(knn[:, 0], nearest)
        _, rep, count, tied = KC.vote(knn, sov)
        moved = int((rep != nearest).sum())
        assert moved > 0.05 * dst.shape[0] and tied.sum() > 0.01 * dst.shape[0], "the vote changes this transfer"
        # without --vote: nearest vertex as before, twice the same bytes
        f0, f1 = _files(os.path.join(plain[0], sub)), _files(os.path.join(plain[1], sub))
        assert f0 == f1 and sorted(f0) == ["final.sem.npy", "pseudo_labels.sgl"]
        assert np.array_equal(pseudo_labels.load(os.path.join(plain[0], sub)).seg_of_vertex, sov[nearest])
        assert np.array_equal(np.load(os.path.join(plain[0], sub, "final.sem.npy")), loose[nearest])
        with np.load(os.path.join(plain[0], sub, scene + transfer.MAP_SUFFIX)) as z:
            assert sorted(z.files) == ["d2", "nearest"] and np.array_equal(z["nearest"], nearest)
            assert z["d2"].tobytes() == NG.d2_of(dst, src, nearest).tobytes()
        e = json.load(open(os.path.join(plain[0], transfer.REPORT_NAME)))["scenes"][scene]
        assert sorted(e) == ["farther_than", "max_distance", "median_distance", "source_V", "target_V"]
        # with --vote 10: every file through rep
        lab = pseudo_labels.load(os.path.join(voted, sub))
        assert lab.V == dst.shape[0] and np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[rep])
        assert np.array_equal(np.load(os.path.join(voted, sub, "final.sem.npy")), loose[rep])
        with np.load(os.path.join(voted, sub, scene + transfer.MAP_SUFFIX)) as z:
            assert sorted(z.files) == ["d2", "nearest", "rep", "tied", "votes"]
            assert z["nearest"].dtype == np.int64 and np.array_equal(z["nearest"], nearest)
            assert z["d2"].dtype == np.float32 and z["d2"].tobytes() == NG.d2_of(dst, src, nearest).tobytes()
            assert np.array_equal(z["rep"], rep) and np.array_equal(z["votes"], count) and np.array_equal(z["tied"], tied)
        e = report["scenes"][scene]
        assert (e["vote"], e["vote_on"], e["moved"], e["tied"]) == (10, "seg", moved, int(tied.sum()))
        assert (e["source_V"], e["target_V"]) == (src.shape[0], dst.shape[0])
        # --vote 5 --vote-on final.ins: the vector's expansion from the .sgl votes
        ins = tables[12][sov]
        assert np.array_equal(pseudo_labels.load(os.path.join(root, sub)).vector("final.ins"), ins)
        rep5 = KC.vote(knn[:, :5], ins)[1]
        assert np.array_equal(pseudo_labels.load(os.path.join(on_ins, sub)).seg_of_vertex, sov[rep5])
        e = json.load(open(os.path.join(on_ins, transfer.REPORT_NAME)))["scenes"][scene]
        assert (e["vote"], e["vote_on"], e["moved"]) == (5, "final.ins", int((rep5 != nearest).sum()))


def test_transfer_vote_argument_errors(tmp_path, capsys):
    from seggroup_amd import transfer
    a, b, root, made = _tree(tmp_path)
    base = ["--from-scans", a, "--to-scans", b, "-n", "e", "--root", root, "--device", DEV, "--out", str(tmp_path / "o")]
    for extra, word in ((["--vote", "10", "--index", "brute"], "--index grid"), (["--vote-on", "final.sem"], "--vote")):
        with pytest.raises(SystemExit) as ei:
            transfer.main(base + extra)
        assert ei.value.code == 2 and word in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "o"))
    bare = str(tmp_path / "bare")                               # an export directory of .npy vectors only: no segment to vote on
    for scene, (src, dst, tables, sov, loose) in made.items():
        d = os.path.join(bare, "results", "e", scene, "epoch_last")
        os.makedirs(d)
        np.save(os.path.join(d, "final.sem.npy"), loose)
    args = ["--from-scans", a, "--to-scans", b, "-n", "e", "--root", bare, "--device", DEV, "--out", str(tmp_path / "o2"), "--vote", "10"]
    with pytest.raises(SystemExit) as ei:
        transfer.main(args)
    assert ei.value.code == 2 and "--vote-on" in capsys.readouterr().err
    assert transfer.main(args + ["--vote-on", "final.sem"]) == 0
    for scene, (src, dst, tables, sov, loose) in made.items():
        rep = KC.vote(KC.brute(dst, src, 10), loose)[1]
        assert np.array_equal(np.load(os.path.join(str(tmp_path / "o2"), "results", "e", scene, "epoch_last", "final.sem.npy")), loose[rep])
