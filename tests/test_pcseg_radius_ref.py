"""The statement of the point-cloud over-segmenter over the radius graph (tests/pcseg_radius_ref.py), checked on its own,
without a GPU: against the committed digests (tools/capture_pcseg_radius.py), its lists against radius_ref, its normals against float64
eigh, the quality of its segments on rooms whose planes are known, the clumped room that is the reason for the feature, the library's host
chain on its edges, and the new argument errors, which fire before any device call.

The bounds are 8f's, fixed before that statement was written: at most 2e-3 rad to eigh's smallest eigenvector over the points whose
relative gap (l1 - l0) / l2 is at least 0.05, at least 0.99 of the points with that gap, at most 40 segments for the 8 planes of a room
and a purity of at least 0.95."""
import json
import os

import numpy as np
import pytest

import pcseg_radius_ref as Q
import pcseg_ref as P
import radius_ref as RR
from conftest import GOLDEN

ROOMS = ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup"]
MEASURED = {"room_j0": (17, 0.9964), "room_j5e-4": (16, 0.9947), "room_j2e-3": (13, 0.9930), "room_dup": (16, 0.9964)}


def _expected():
    return json.load(open(os.path.join(GOLDEN, "pcseg_radius_expected.json")))["cases"]


def _planes(name):
    return P.case_clouds()[name][1]


@pytest.mark.parametrize("name", sorted(Q.fixture_cases()))
def test_golden_digests(name):
    xyz, _, r, seg = Q.case(name)
    exp = _expected()[name]
    assert xyz.shape[0] == exp["N"]
    for key, val in Q.stage_digests(r, seg).items():
        assert val == exp[key], key
    assert np.array_equal(np.lexsort((r["edges"][:, 1], r["edges"][:, 0], r["w"])), np.arange(r["w"].shape[0])), "ascending (w, a, b)"


@pytest.mark.parametrize("name", ["line_65_path", "line_257_all", "two_clumps", "room_dup", "all_equal", "ball_300"])
def test_lists_are_radius_ref_in_csr_form(name):
    xyz, radius, r, _ = Q.case(name)
    off, idx = r["off"], r["idx"]
    n = xyz.shape[0]
    cnt = RR.count(xyz, radius)
    assert off.dtype == np.int64 and idx.dtype == np.int32 and off[0] == 0
    assert np.array_equal(np.diff(off), cnt.astype(np.int64)) and off[n] == idx.shape[0]
    rows = np.repeat(np.arange(n), np.diff(off))
    assert (idx != rows).all(), "no self pairs"
    inner = np.ones(idx.shape[0], bool)
    inner[off[:-1][np.diff(off) > 0]] = False                                  # the first entry of every row has no predecessor
    assert (np.diff(idx.astype(np.int64))[inner[1:]] > 0).all(), "rows ascend"
    a, b = RR.pairs(xyz, radius)
    order = np.lexsort((b, a))
    assert np.array_equal(r["lex_edges"].astype(np.int64), np.stack([a[order], b[order]], 1))
    assert r["lex_edges"].shape[0] * 2 == off[n]


@pytest.mark.parametrize("name", ROOMS + ["room_20k", "clumped_room"])
def test_normals_agree_with_float64_eigh(name):
    xyz, _, r, _ = Q.case(name)
    ang, share = Q.eigh_check(xyz, r["off"], r["idx"], r["normals"])
    print(f"{name}: max angle {ang:.3e} rad, gap share {share:.4f}")
    assert share >= 0.99
    assert ang <= 2e-3


def test_five_sweeps_leave_no_off_diagonal():
    for name in Q.fixture_cases():
        xyz, _, r, _ = Q.case(name)
        _, offd = Q.normals(xyz, r["off"], r["idx"], want_offdiag=True)
        assert all(not o.any() for o in offd), name


def test_degenerate_neighbourhoods_follow_the_rule():
    xyz, _, r, seg = Q.case("all_equal")
    assert np.array_equal(r["normals"], np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (32, 1)))           # nothing rotates: column 0
    assert (np.diff(r["off"]) == 31).all() and np.unique(seg).shape[0] == 1
    xyz, _, r, _ = Q.case("line_63_none")                                                                     # no neighbour at all
    assert r["off"][-1] == 0 and r["lex_edges"].shape == (0, 2)
    assert np.array_equal(np.abs(r["normals"]), np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (63, 1)))
    xyz, _, r, _ = Q.case("ball_300")
    assert (np.diff(r["off"]) == 299).all()


@pytest.mark.parametrize("name", ROOMS)
def test_rooms_come_apart_into_their_planes(name):
    _, _, _, seg = Q.case(name)
    nseg, pur = int(np.unique(seg).shape[0]), P.purity(seg, _planes(name))
    print(f"{name}: {nseg} segments, purity {pur:.4f}")
    assert nseg <= 40
    assert pur >= 0.95
    assert (nseg, round(pur, 4)) == MEASURED[name]


def test_the_clumped_room_is_why_the_radius_graph_exists():
    xyz, plane = Q.clumped_room()
    assert xyz.shape == (15792, 3)
    seg = P.segment_pointcloud(xyz, 10)                                        # the committed kNN statement: every clump its own segment
    sizes = np.unique(seg, return_counts=True)[1]
    print(f"kNN-10: {sizes.shape[0]} segments, largest {sizes.max()}")
    assert sizes.shape[0] >= 1000 and sizes.max() <= 12
    _, _, _, seg = Q.case("clumped_room")
    nseg, pur = int(np.unique(seg).shape[0]), P.purity(seg, plane)
    print(f"radius {Q.CLUMPED_RADIUS}: {nseg} segments, purity {pur:.4f}")
    assert nseg == 16 and pur == 1.0
    length = np.diff(Q.case("clumped_room")[2]["off"])
    assert 35 <= length.min() and length.max() <= 71


def test_host_chain_equals_the_statement(sg_lib):
    from seggroup_amd import oversegment
    for name in ("line_513_path", "two_clumps", "room_j5e-4", "room_dup", "all_equal", "ball_300", "clumped_room"):
        xyz, _, r, seg = Q.case(name)
        assert np.array_equal(oversegment.merge_edges(r["edges"], r["w"], xyz.shape[0]), seg), name


def test_the_pair_cap_is_declared_on_both_sides(sg_lib):
    from seggroup_amd import hip
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "seggroup_hip.h")).read()
    assert "#define SG_MAX_RADIUS_PAIRS (1ll << 30)" in src and hip.MAX_RADIUS_PAIRS == 1 << 30 <= 2 ** 31 - 1
    assert sg_lib.sg_radius_neighbours_ws_bytes(100, hip.MAX_RADIUS_PAIRS + 1) == 0 and sg_lib.sg_pcseg_ws_bytes_radius(100, -1) == 0
    assert sg_lib.sg_radius_neighbours_ws_bytes(100, 50) > sg_lib.sg_radius_neighbours_ws_bytes(100, 0) > 0
    names = [sg_lib.sg_pcseg_radius_stage_name(i).decode() for i in range(13)]
    assert names == "box cells sort table count scan fill rows normals edges weights weight_sort gather".split()
    assert sg_lib.sg_pcseg_radius_stage_name(13) is None


def test_refusals_come_before_the_first_device_call(sg_lib):
    """no GPU here (or none touched): every one of these returns before a HIP call, with a message"""
    import ctypes as C
    from seggroup_amd import hip
    t, e = C.c_int64(-1), C.c_int(-1)
    one = 0x1000                                                               # never dereferenced
    call = sg_lib.sg_radius_neighbours_grid
    assert call(one, 3, 10, 0.1, 0.0, 0, one, None, None, one, 1 << 30, None) == hip.SG_EINVAL                 # h_T
    assert call(None, 3, 10, 0.1, 0.0, 0, one, None, C.byref(t), one, 1 << 30, None) == hip.SG_EINVAL and t.value == 0
    assert call(one, 2, 10, 0.1, 0.0, 0, one, None, C.byref(t), one, 1 << 30, None) == hip.SG_EINVAL
    assert call(one, 3, 10, float("nan"), 0.0, 0, one, None, C.byref(t), one, 1 << 30, None) == hip.SG_EINVAL
    assert call(one, 3, 10, 0.1, 0.0, -1, one, None, C.byref(t), one, 1 << 30, None) == hip.SG_EINVAL
    assert call(one, 3, 10, 0.1, 0.0, 5, one, None, C.byref(t), one, 1 << 30, None) == hip.SG_EINVAL           # room at a null d_idx
    assert call(one, 3, (1 << 24) + 1, 0.1, 0.0, 0, one, None, C.byref(t), one, 1 << 30, None) == hip.SG_EUNSUP
    assert call(one, 3, 10, 0.1, 0.0, hip.MAX_RADIUS_PAIRS + 1, one, one, C.byref(t), one, 1 << 30, None) == hip.SG_EUNSUP
    msg = sg_lib.sg_last_error().decode()
    assert "smaller radius" in msg and "thin" in msg
    assert call(one, 3, 10, 0.1, 0.0, 0, one, None, C.byref(t), one, 16, None) == hip.SG_ENOMEM
    assert "workspace too small" in sg_lib.sg_last_error().decode()
    assert sg_lib.sg_pointcloud_normals_csr(one, 0, one, one, None, one, one, 1 << 20, None) == hip.SG_EINVAL
    bad_view = (C.c_float * 3)(0.0, float("inf"), 0.0)
    assert sg_lib.sg_pointcloud_normals_csr(one, 10, one, one, bad_view, one, one, 1 << 20, None) == hip.SG_EINVAL
    assert "viewpoint" in sg_lib.sg_last_error().decode()
    assert sg_lib.sg_pcseg_edges_radius(one, 10, 0.1, 0.0, 8, None, None, None, one, one, one, C.byref(e), C.byref(t), one, 16, None) == hip.SG_ENOMEM
    assert sg_lib.sg_pcseg_edges_radius(one, 10, -1.0, 0.0, 8, None, None, None, one, one, one, C.byref(e), C.byref(t), one, 1 << 30,
                                        None) == hip.SG_EINVAL
    assert "radius" in sg_lib.sg_last_error().decode()
    ids = (C.c_int32 * 10)()
    assert sg_lib.sg_pcseg_scan_radius(one, 10, 0.1, 0.0, hip.MAX_RADIUS_PAIRS + 2, None, 0.01, 20, ids, C.byref(t), one, 1 << 30,
                                       None) == hip.SG_EUNSUP
    assert sg_lib.sg_pcseg_scan_radius(one, 0, 0.1, 0.0, 8, None, 0.01, 20, ids, C.byref(t), one, 1 << 30, None) == hip.SG_EINVAL


def test_python_argument_errors_fire_before_a_device_call(monkeypatch):
    """radius goes with neither k, nor index, nor a kNN table; the old messages are what they were"""
    from seggroup_amd import hip, oversegment, prepare
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was loaded"))
    xyz = np.zeros((30, 3), np.float32)
    for fn in (oversegment.pointcloud_edges, oversegment.segment_pointcloud):
        with pytest.raises(ValueError, match="radius and k = 20 are two different graphs"):
            fn(xyz, 20, radius=0.1)
        with pytest.raises(ValueError, match="radius and index = 'grid' are two different graphs"):
            fn(xyz, radius=0.1, index="grid")
        with pytest.raises(ValueError, match="radius must be a finite length > 0"):
            fn(xyz, radius=float("inf"))
    with pytest.raises(ValueError, match="radius and a kNN table are two different graphs"):
        oversegment.pointcloud_normals(xyz, knn=np.zeros((30, 11), np.int32), radius=0.1)
    with pytest.raises(ValueError, match="radius and k = 5"):
        oversegment.pointcloud_normals(xyz, 5, radius=0.1)
    with pytest.raises(ValueError, match="lists belong to the radius form"):
        oversegment.pointcloud_normals(xyz, lists=(np.zeros(31, np.int64), np.zeros(0, np.int32)))
    with pytest.raises(ValueError, match="radius and k = 5"):
        oversegment.oversegment_scans("/nowhere", [], knn=5, radius=0.1)
    with pytest.raises(ValueError, match="radius and knn = 5"):
        prepare.prepare_scene("/nowhere/scene0000_00", 0, knn=5, radius=0.1)
    with pytest.raises(ValueError, match="radius and knn = 20"):
        prepare.generate_mesh_adjcency_pth("scene0000_00", root="/nowhere", knn=20, radius=0.1)
    with pytest.raises(ValueError, match='index must be "brute" or "grid"|index'):                              # the old message, unchanged
        oversegment.segment_pointcloud(xyz, index="tree")


def test_a_mesh_refuses_the_radius_graph(tmp_path, monkeypatch):
    from seggroup_amd import oversegment, prepare
    monkeypatch.setattr(oversegment, "segment_mesh", lambda *a, **k: pytest.fail("the mesh path ran"))
    monkeypatch.setattr(oversegment, "segment_pointcloud", lambda *a, **k: pytest.fail("the point-cloud path ran"))
    scene = tmp_path / "scans" / "scene0000_00"
    scene.mkdir(parents=True)
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    prepare.write_ply(str(scene / "scene0000_00_vh_clean_2.ply"), xyz, np.zeros((4, 3), np.uint8), np.array([[0, 1, 2], [2, 1, 3]], np.int32))
    with pytest.raises(ValueError, match="the radius graph belongs to the point-cloud path; this scan is a mesh"):
        oversegment.oversegment_scan(str(scene), radius=0.5)
    with pytest.raises(ValueError, match="the radius graph belongs to a scan without faces"):
        prepare.prepare_scene(str(scene), 0, radius=0.5)
    for extra, text in ((["--knn", "10"], "--radius and --knn are two different graphs"),
                        (["--index", "brute"], "--radius and --index are two different graphs"),
                        ([], "--radius is the graph of point clouds, and scene0000_00 has faces")):
        with pytest.raises(SystemExit) as ex:
            oversegment.main(["--scans", str(tmp_path / "scans"), "--radius", "0.5"] + extra)
        assert ex.value.code == 2
    with pytest.raises(SystemExit):
        oversegment.main(["--scans", str(tmp_path / "scans"), "--radius", "-1", "--pointcloud"])


def test_parser_errors_name_the_conflict(tmp_path, capsys):
    from seggroup_amd import oversegment
    (tmp_path / "scans").mkdir()
    with pytest.raises(SystemExit):
        oversegment.main(["--scans", str(tmp_path / "scans"), "--radius", "0.5", "--knn", "20"])
    assert "--radius and --knn are two different graphs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        oversegment.main(["--scans", str(tmp_path / "scans"), "--radius", "0.5", "--index", "grid"])
    assert "--radius and --index are two different graphs" in capsys.readouterr().err
