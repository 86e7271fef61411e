"""The two-cloud k-nearest search and the vote over its rows, without a GPU: the NumPy statement of the ring walk with a
list of k entries (tests/knn_cross_ref.py) against the plain statement `brute` -- the first k columns of a stable descending sort of the
score row -- on nearest_grid_ref's seven pairs at their two forced cells, column 0 against nearest_grid_ref.brute, the vote rule on
labelled candidates (with enough ties and moved vertices for the checks to mean something), and what the host refuses before any
device call."""
import ctypes as C

import numpy as np
import pytest

import knn_cross_ref as KC
import nearest_grid_ref as NG
import pcseg_ref as R

SAMPLE = 1000                                   # queries of a pair that are searched (seeded, plus the last two: the outliers)
PAIRS = ["plain", "lattice", "dup", "all_equal", "half_room", "outliers", "shifted"]
# the ring limit: the library's, except on the shifted pair at the small cell, whose margin spans ten cells of 0.05 (as in
# test_nearest_grid_ref.py: there the rule itself is what is being checked)
LIMIT = {("shifted", 0.05): 40}
_want = {}


def _rows(n):
    if n <= SAMPLE:
        return np.arange(n)
    return np.union1d(np.random.RandomState(11).choice(n, SAMPLE, replace=False), [n - 2, n - 1])


def _brute(name):
    """brute's rows at k = 20, once per pair: its first 5 and 10 columns are the statement at k = 5 and 10"""
    if name not in _want:
        x, y = NG.case_pairs()[name]
        _want[name] = KC.brute(x[_rows(x.shape[0])], y, 20)
    return _want[name]


@pytest.mark.parametrize("k", KC.KS)
@pytest.mark.parametrize("name", PAIRS)
def test_the_walk_equals_brute_force(name, k):
    x, y = NG.case_pairs()[name]
    rows, want = _rows(x.shape[0]), _brute(name)[:, :k]
    for cell in NG.CELLS[name]:
        got, rings, grid = KC.knn_cross_grid(x, y, k, cell, ring_limit=LIMIT.get((name, cell), KC.RING_LIMIT), rows=rows)
        print(f"{name} k = {k} h = {cell}: rings mean {rings.mean():.2f}, queued {int((rings == 0).sum())}, "
              f"{int((got != want).any(1).sum())} rows wrong")
        assert got.dtype == np.int32 and np.array_equal(got, want), f"{name} k = {k} h = {cell}: {int((got != want).any(1).sum())} rows differ"
        assert np.array_equal(grid.whole, want)
        if name == "shifted":
            assert (rings > 0).all(), "the rings settled every query: the rule was exercised, not the queue"
        if name == "outliers":
            assert (rings[-2:] == 0).all(), "the two outlying queries end in the queue"


@pytest.mark.parametrize("name", PAIRS)
def test_column_0_is_the_nearest_point(name):
    x, y = NG.case_pairs()[name]
    rows = _rows(x.shape[0])
    want = _brute(name)
    assert np.array_equal(want[:, 0].astype(np.int64), NG.brute(x[rows], y))
    assert np.array_equal(KC.brute(x[rows[:64]], y, 5), want[:64, :5]) and np.array_equal(KC.brute(x[rows[:64]], y, 10), want[:64, :10])
    s = R.pair_scores(x[rows[:64]], y)
    top = np.take_along_axis(s, want[:64].astype(np.int64), 1)
    assert (np.diff(top, axis=1) <= 0).all(), "descending scores"
    same = np.diff(top, axis=1) == 0
    assert (np.diff(want[:64], axis=1)[same] > 0).all(), "the lower index first among equal scores"
    if name in ("lattice", "dup", "all_equal"):
        assert same.any(), "the pair has equal scores inside a row"


def test_a_list_that_is_not_full_is_unsettled():
    """five candidates in one corner cell, queries in another: ring 1 of a far query holds nothing, a ring that holds four candidates of
    five cannot settle k = 5 whatever their scores; the answer is brute's all the same"""
    y = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.01], [0.35, 0, 0]], np.float32)
    x = np.array([[0.02, 0.02, 0.02], [1.0, 1.0, 1.0], [0.3, 0.0, 0.0]], np.float32)
    got, rings, grid = KC.knn_cross_grid(x, y, 5, 0.1)
    assert np.array_equal(got, KC.brute(x, y, 5))
    assert rings[0] > 1, "four candidates in the first block: not full, so not settled there"
    with pytest.raises(ValueError):
        KC.knn_cross_grid(x, y[:4], 5, 0.1)


def test_the_vote_rule_on_written_out_rows():
    labels = np.array([7, 7, 3, 3, 3, -1, 2 ** 31 - 1, -2 ** 31], np.int32)
    knn = np.array([[0, 2, 3, 1, 5],            # 7 3 3 7 -1: two each; 7 is met first -> rep 0, tied
                    [2, 0, 3, 1, 4],            # 3 7 3 7 3: three of 3 -> rep 2, not tied
                    [5, 6, 7, 0, 1],            # -1 max min 7 7: 7 wins with 2 -> rep 0 (column 3)
                    [5, 6, 7, 0, 2],            # all different: the first wins with 1, tied
                    [4, 4, 4, 4, 4]], np.int32)
    w, rep, cnt, tied = KC.vote(knn, labels)
    assert w.tolist() == [7, 3, 7, -1, 3] and rep.tolist() == [0, 2, 0, 5, 4]
    assert cnt.tolist() == [2, 3, 2, 1, 5] and tied.tolist() == [1, 0, 0, 1, 0]
    w1, rep1, cnt1, tied1 = KC.vote(knn[:, :1], labels)
    assert np.array_equal(rep1, knn[:, 0]) and np.array_equal(w1, labels[knn[:, 0]]) and (cnt1 == 1).all() and not tied1.any()
    with pytest.raises(ValueError):
        KC.vote(np.array([[0, 8]]), labels)


@pytest.mark.parametrize("name", PAIRS)
def test_the_vote_inputs_are_not_vacuous(name):
    """on every pair but all_equal at least 1 % of the sampled rows are tied and at least 5 % have rep != nearest, for every k"""
    x, y = NG.case_pairs()[name]
    labels = KC.labels_of(y)
    assert labels.dtype == np.int32 and labels.shape[0] == y.shape[0]
    for k in KC.KS:
        knn = _brute(name)[:, :k]
        w, rep, cnt, tied = KC.vote(knn, labels)
        share_tied, share_moved = float(tied.mean()), float((rep != knn[:, 0]).mean())
        print(f"{name} k = {k}: {100 * share_tied:.1f} % tied, {100 * share_moved:.1f} % moved, mean count {cnt.mean():.2f}")
        assert np.array_equal(w, labels[rep]) and (cnt >= 1).all() and (cnt <= k).all()
        assert ((rep[:, None] == knn).any(1)).all()
        if name == "all_equal":
            assert not tied.any() and (cnt == k).all() and np.array_equal(rep, knn[:, 0])
        else:
            assert share_tied >= 0.01 and share_moved >= 0.05


def test_the_envelope_is_decided_on_the_host(sg_lib):
    """k, the caps, U * k, the pointers, the strides, the cell and the workspace size need no GPU to be refused"""
    from seggroup_amd import hip
    cap_n, cap_u = hip.MAX_GRID_POINTS, hip.MAX_CLOUD_POINTS
    ws = sg_lib.sg_cloud_knn_cross_grid_ws_bytes
    assert ws(5, cap_n + 1, 5) == 0 and ws(5, 4, 5) == 0 and ws(-1, 50, 5) == 0 and ws(cap_u + 1, 50, 5) == 0
    assert ws(100, 100, 7) == 0 and ws(100, 100, 1) == 0 and ws(100, 19, 20) == 0
    assert ws(cap_u, 50, 20) == 0, "U * k beyond an int"
    assert ws((2 ** 31 - 1) // 20, 50, 20) > 0 and ws((2 ** 31 - 1) // 20 + 1, 50, 20) == 0
    assert ws(1000, 1000, 10) == sg_lib.sg_nearest_point_grid_ws_bytes(1000, 1000) > 0
    assert 0 < ws(0, 5, 5) < ws(1000, 1000, 5) < ws(1 << 20, 1 << 20, 20)
    buf = (C.c_int * 64)()
    p = C.addressof(buf)
    call = lambda x=p, xs=3, u=300, y=p, ys=3, n=300, k=10, cell=0.0, knn=p, d2=None, w=p, nb=1 << 30: sg_lib.sg_cloud_knn_cross_grid(   # noqa: E731
        x, xs, u, y, ys, n, k, cell, knn, d2, w, nb, None)
    for k in (0, 1, 6, 19, 21, -5):
        assert call(k=k) == hip.SG_EUNSUP and b"is not built" in sg_lib.sg_last_error()
    assert call(n=cap_n + 1, x=None, y=None, knn=None, w=None, nb=0) == hip.SG_EUNSUP and b"at most" in sg_lib.sg_last_error()
    assert call(u=cap_u + 1) == hip.SG_EUNSUP and b"at most" in sg_lib.sg_last_error()
    assert call(u=(2 ** 31 - 1) // 20 + 1, k=20) == hip.SG_EUNSUP and b"entries" in sg_lib.sg_last_error()
    assert call(n=9) == hip.SG_EINVAL and b"9 candidates for k = 10" in sg_lib.sg_last_error()
    assert call(n=0) == hip.SG_EINVAL and call(n=-3) == hip.SG_EINVAL and call(u=-1) == hip.SG_EINVAL
    assert call(x=None) == hip.SG_EINVAL and call(y=None) == hip.SG_EINVAL and call(knn=None) == hip.SG_EINVAL and call(w=None) == hip.SG_EINVAL
    assert call(xs=2) == hip.SG_EINVAL and call(ys=2) == hip.SG_EINVAL
    for cell in (-0.5, float("nan"), float("inf")):
        assert call(cell=cell) == hip.SG_EINVAL and b"cell edge" in sg_lib.sg_last_error()
    assert call(nb=ws(300, 300, 10) - 1) == hip.SG_EINVAL and b"workspace too small" in sg_lib.sg_last_error()
    assert call(u=0, x=None, knn=None, w=None, nb=0) == hip.SG_OK, "no queries: nothing to do, nothing touched"
    stats = (C.c_int64 * 16)()
    assert sg_lib.sg_cloud_knn_cross_grid_stats(stats, 16) == 9 and not any(stats), "a refused call leaves no statistics"
    assert sg_lib.sg_cloud_knn_cross_grid_stats(stats, 4) == hip.SG_EINVAL
    names = [sg_lib.sg_cloud_knn_cross_grid_stage_name(i) for i in range(8)]
    assert names == [sg_lib.sg_nearest_point_grid_stage_name(i) for i in range(8)] and names[5:] == [b"search", b"fallback", None]
    us = (C.c_float * 8)()
    assert sg_lib.sg_cloud_knn_cross_grid_stage_times(us, 8) == 7 and sg_lib.sg_cloud_knn_cross_grid_stage_times(us, 6) == hip.SG_EINVAL
    assert sg_lib.sg_cloud_knn_cross_grid_set_tuning(0, 65) == hip.SG_EINVAL and sg_lib.sg_cloud_knn_cross_grid_set_tuning(0, 0) == hip.SG_OK
    assert sg_lib.sg_cloud_knn_cross_grid_set_timing(0) == hip.SG_OK
    vote = lambda knn=p, u=4, k=5, lab=p, n=8, w=p, rep=p, cnt=None, tied=None: sg_lib.sg_knn_vote(knn, u, k, lab, n, w, rep, cnt, tied, None)   # noqa: E731
    assert vote(k=0) == hip.SG_EINVAL and vote(k=33) == hip.SG_EINVAL and b"1 <= k <= 32" in sg_lib.sg_last_error()
    assert vote(u=-1) == hip.SG_EINVAL and vote(n=0) == hip.SG_EINVAL
    assert vote(knn=None) == hip.SG_EINVAL and vote(lab=None) == hip.SG_EINVAL and vote(w=None) == hip.SG_EINVAL and vote(rep=None) == hip.SG_EINVAL
    assert vote(u=0, knn=None, lab=None, w=None, rep=None) == hip.SG_OK


def test_vote_arguments_of_the_command_line_are_decided_before_any_device(tmp_path, capsys):
    from seggroup_amd import transfer
    base = ["--from-scans", str(tmp_path), "--to-scans", str(tmp_path), "-n", "e", "--out", str(tmp_path / "o")]
    for extra, word in ((["--vote", "10", "--index", "brute"], "--index grid"), (["--vote-on", "final.sem"], "--vote"), (["--vote", "7"], "--vote"),
                        (["--vote", "10", "--vote-on", "layer_9.seg"], "--vote-on")):
        with pytest.raises(SystemExit) as ei:
            transfer.main(base + extra)
        assert ei.value.code == 2 and word in capsys.readouterr().err, extra
