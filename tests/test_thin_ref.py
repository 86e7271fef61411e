"""The voxel thinning's specification, without a GPU: the NumPy statement (tests/thin_ref.py) against a second formulation
(a plain loop over the voxels) on every case cloud and voxel edge, its invariants, the committed counts and digests
(tests/golden/thin_expected.json, tools/capture_thin.py), a crafted tie, the quality condition of the thinned-and-lifted segmentation, and
the host parts of the library: the workspace formula's cap and lift / lift_sgl."""
import json
import os

import numpy as np
import pytest

import pcseg_ref
import thin_ref as T
from conftest import GOLDEN

_clouds, _thin = {}, {}
NAMES = T.CASE_NAMES


def _cloud(name):
    if not _clouds:
        _clouds.update(T.case_clouds())
    return _clouds[name]


def _ref(name, h):
    if (name, h) not in _thin:
        _thin[(name, h)] = T.thin(_cloud(name), h)
    return _thin[(name, h)]


def _expected():
    return json.load(open(os.path.join(GOLDEN, "thin_expected.json")))


def test_the_case_list_is_complete():
    _cloud("tie")
    assert sorted(NAMES) == sorted(_clouds)


@pytest.mark.parametrize("name", NAMES)
def test_statement_equals_the_loop_over_voxels(name):
    xyz = _cloud(name)
    for h in T.VOXELS:
        rep, top, lo = _ref(name, h)
        rep2, top2, lo2 = T.thin_by_loop(xyz, h)
        assert rep.dtype == np.int32 and top.dtype == np.int32
        assert np.array_equal(rep, rep2) and np.array_equal(top, top2) and lo.tobytes() == lo2.tobytes(), (name, h)
        m = rep.shape[0]
        assert (np.diff(rep) > 0).all() and np.array_equal(top[rep], np.arange(m)), "rep ascends and maps onto itself"
        _, c, _ = T.cells(xyz, h)
        assert np.array_equal(c, c[rep[top]]), "every point shares its cell with its representative"
        assert np.unique(T.voxel_key(c)).shape[0] == m, "one representative per occupied voxel"


def test_counts_and_committed_digests():
    exp = _expected()["clouds"]
    assert sorted(exp) == sorted(NAMES)
    for name in NAMES:
        for h in T.VOXELS:
            rep, top, _ = _ref(name, h)
            e = exp[name]["%g" % h]
            assert (e["N"], e["M"]) == (_cloud(name).shape[0], rep.shape[0]), (name, h)
            assert T.array_digest(rep) == e["rep"] and T.array_digest(top) == e["thin_of_point"], (name, h)
            cells, largest = T.stats(_cloud(name), h, rep, top)
            assert cells == e["cells"] and largest == e["largest_voxel"]
    for name in ("room_j0", "room_j5e-4"):
        rep, top, _ = _ref(name, 0.02)
        n = _cloud(name).shape[0]
        assert n == 5281 and np.array_equal(rep, np.arange(n)) and np.array_equal(top, np.arange(n)), "the identity"
    assert _ref("room_20k", 0.05)[0].shape[0] == 5403
    assert all(_ref("all_equal", h)[0].shape[0] == 1 for h in T.VOXELS)
    assert np.array_equal(_ref("all_equal", 0.05)[0], [0]) and not _ref("all_equal", 0.05)[1].any()


def test_crafted_tie_goes_to_the_lower_index():
    _, _, d2 = T.cells(T.TIE, 1.0)
    assert d2[1] == d2[2] < d2[0]
    rep, top, lo = T.thin(T.TIE, 1.0)
    assert np.array_equal(rep, [1]) and np.array_equal(top, [0, 0, 0]) and not lo.any()
    rep, top, _ = T.thin(T.TIE[[0, 2, 1]], 1.0)
    assert np.array_equal(rep, [1]), "the index decides, not the coordinate"


def test_cell_range_and_bad_input():
    with pytest.raises(T.CellRange):
        T.thin(_cloud("line"), 1e-6)
    assert T.thin(_cloud("room_j0"), 1e-6)[0].shape[0] == 5281, "the rooms stay just inside 2^21 cells at that edge"
    for h in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            T.thin(_cloud("n255"), h)
    x = _cloud("n255").copy()
    x[3, 1] = np.nan
    with pytest.raises(ValueError):
        T.thin(x, 0.05)


def test_signed_zero_minimum_does_not_move_the_result():
    x = _cloud("n255").copy()
    x[:, 0] = np.abs(x[:, 0])
    x[7, 0], x[9, 0] = 0.0, -0.0
    a, b = T.thin(x, 0.05), T.thin(x[::-1], 0.05)
    assert np.signbit(a[2][0]) and a[2].tobytes() == b[2].tobytes()
    y = x.copy()
    y[9, 0] = 0.0
    c = T.thin(y, 0.05)
    assert not np.signbit(c[2][0]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_quality_of_the_thinned_and_lifted_segmentation():
    """8f's own bounds hold for room_20k thinned at 0.05, segmented by the statement of 8f and lifted: purity >= 0.95, at most 40 segments.
    (The statement alone: 0.976 and 9; un-thinned 0.996 and 17.)"""
    xyz, plane = pcseg_ref.case_clouds(include_large=True)["room_20k"]
    seg, seg_thin, rep, top = T.segment_thinned(xyz, 0.05)
    purity, segments = pcseg_ref.purity(seg, plane), np.unique(seg_thin).shape[0]
    print("room_20k thinned at 0.05: purity %.4f, %d segments" % (purity, segments))
    assert purity >= 0.95 and segments <= 40
    assert np.array_equal(np.unique(seg), rep[np.unique(seg_thin)]) and np.isin(seg, rep).all(), "ids are raw indices of representatives"
    exp = _expected()["room_20k_quality"]
    assert T.array_digest(seg) == exp["sha256"] and segments == exp["segments"]


def test_identity_thinning_reproduces_the_unthinned_statement():
    xyz = _cloud("n257")
    seg, _, rep, _ = T.segment_thinned(xyz, 1e-4)
    assert rep.shape[0] == xyz.shape[0] and np.array_equal(seg, pcseg_ref.segment_pointcloud(xyz))


# ---- host parts of the library -----------------------------------------------------------------------------------------------------
def test_workspace_formula_and_the_cap(sg_lib):
    cap = 1 << 27
    assert sg_lib.sg_cloud_thin_ws_bytes(cap + 1) == 0 and sg_lib.sg_cloud_thin_ws_bytes(0) == 0 and sg_lib.sg_cloud_thin_ws_bytes(-5) == 0
    one, full = sg_lib.sg_cloud_thin_ws_bytes(1), sg_lib.sg_cloud_thin_ws_bytes(cap)
    assert 0 < one < 1 << 16
    assert 48 * cap <= full < 56 * cap, "about 50 bytes a point: %d" % full
    assert [sg_lib.sg_cloud_thin_stage_name(i) for i in range(7)] == [b"check_box", b"keys", b"sort", b"representatives", b"compact", b"map", None]


def test_arguments_are_refused_before_any_device_call(sg_lib):
    """null pointers, the stride, N, the voxel edge, the cap and the workspace size are decided on the host: no GPU is needed to be refused"""
    import ctypes as C
    from seggroup_amd import hip
    m = C.c_int(7)
    buf = (C.c_int * 64)()
    p = C.addressof(buf)
    call = lambda pts=p, stride=3, n=4, h=0.05, rep=p, top=p, mm=C.byref(m), ws=p, nb=1 << 20: sg_lib.sg_cloud_thin(   # noqa: E731
        pts, stride, n, h, rep, top, mm, None, ws, nb, None)
    assert call(pts=None) == hip.SG_EINVAL and call(rep=None) == hip.SG_EINVAL and call(top=None) == hip.SG_EINVAL
    assert call(mm=None) == hip.SG_EINVAL and call(ws=None) == hip.SG_EINVAL
    assert call(stride=2) == hip.SG_EINVAL and call(n=0) == hip.SG_EINVAL and call(n=-1) == hip.SG_EINVAL
    for h in (0.0, -1.0, float("nan"), float("inf")):
        assert call(h=h) == hip.SG_EINVAL and b"voxel" in sg_lib.sg_last_error()
    assert call(n=(1 << 27) + 1, nb=1 << 40) == hip.SG_EUNSUP
    assert call(nb=64) == hip.SG_EINVAL and b"workspace too small" in sg_lib.sg_last_error()
    assert m.value == 0


def test_lift_and_lift_sgl_round_trip(tmp_path, sg_lib):
    from seggroup_amd import pseudo_labels, thin
    rng = np.random.RandomState(5)
    m, n, s = 700, 5000, 37
    top = rng.randint(0, m, n).astype(np.int32)
    top[:m] = rng.permutation(m)
    vals = rng.randint(-1, 9, (m, 2))
    assert np.array_equal(thin.lift(vals, top), vals[top])
    import torch
    got = thin.lift(torch.from_numpy(vals), torch.from_numpy(top))
    assert isinstance(got, torch.Tensor) and np.array_equal(got.numpy(), vals[top])
    tables = rng.randint(-1, 40, (14, s)).astype(np.int32)
    sov = rng.randint(-1, s, m).astype(np.int32)
    src = pseudo_labels.write(str(tmp_path / "thin.sgl"), tables, sov)
    thin_lab = pseudo_labels.load(src)
    dst_dir = tmp_path / "raw" / "epoch_last"
    os.makedirs(dst_dir)
    dst = thin.lift_sgl(src, str(dst_dir), top)
    assert dst == str(dst_dir / pseudo_labels.SGL_NAME)
    lab = pseudo_labels.load(dst)
    assert pseudo_labels.read_header(dst)["V"] == n == lab.V and lab.S == s
    assert np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[top])
    assert np.array_equal(lab.vectors(), thin_lab.vectors()[:, top])
    with pytest.raises(ValueError):
        thin.lift_sgl(src, str(tmp_path / "bad.sgl"), np.array([0, m], np.int32))


def test_voxel_on_a_mesh_is_an_argparse_error(tmp_path, capsys):
    """--voxel without --pointcloud on a scan that has faces: refused by the parser before any work, not silently ignored"""
    from seggroup_amd import oversegment, prepare
    name = "scene0044_00"
    os.makedirs(tmp_path / name)
    xyz = _cloud("n255")
    faces = np.arange(9, dtype=np.int32).reshape(3, 3)
    prepare.write_ply(str(tmp_path / name / (name + "_vh_clean_2.ply")), xyz, np.zeros(xyz.shape, np.uint8), faces)
    with pytest.raises(SystemExit) as ei:
        oversegment.main(["--scans", str(tmp_path), "--voxel", "0.05"])
    assert ei.value.code == 2 and "--pointcloud" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / name / oversegment.segs_json_name(name))
    with pytest.raises(ValueError, match="point-cloud path"):
        oversegment.oversegment_scan(str(tmp_path / name), voxel=0.05)
