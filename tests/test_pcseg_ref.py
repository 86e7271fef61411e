"""The point-cloud over-segmenter's NumPy statement (tests/pcseg_ref.py), checked on its own, without a GPU: its normals
against float64 eigh, the quality of its segments on rooms whose planes are known, its degenerate cases, the committed digests
(tools/capture_pcseg.py), the library's host chain on its edges, and a PLY without faces through read_ply / mesh_arrays.

The bounds were fixed before the statement was written: the largest angle to eigh's smallest eigenvector at most 2e-3 rad over the points whose relative gap
(l1 - l0) / l2 is at least 0.05 (three times what a float32 prototype of the contract showed, 6.6e-4), at least 0.99 of the points of
every non-degenerate case with that gap, at most 40 segments for the 8 planes of a room and a purity of at least 0.95."""
import json
import os

import numpy as np
import pytest

import pcseg_ref as R
from conftest import GOLDEN

_cache = {}


def _case(name):
    """(xyz, plane, stages, seg) of one generated cloud, computed once per session"""
    if "clouds" not in _cache:
        _cache["clouds"] = R.case_clouds(include_large=False)
    if name not in _cache:
        xyz, plane = _cache["clouds"][name]
        r = R.sorted_edges(xyz, 10)
        _cache[name] = (xyz, plane, r, R.merge(r["edges"], r["w"], xyz.shape[0]))
    return _cache[name]


def _expected():
    return json.load(open(os.path.join(GOLDEN, "pcseg_expected.json")))


SMALL = ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup", "n_k_plus_1", "n255", "n256", "n257", "line", "all_equal"]


@pytest.mark.parametrize("name", [n for n in SMALL if n not in R.DEGENERATE])
def test_normals_agree_with_float64_eigh(name):
    xyz, _, r, _ = _case(name)
    ang, share = R.eigh_check(xyz, r["knn"], r["normals"])
    print(f"{name}: max angle {ang:.3e} rad, gap share {share:.4f}")
    assert share >= 0.99
    assert ang <= 2e-3
    exp = _expected()[name]
    assert ang == pytest.approx(exp["max_angle_rad"], rel=1e-3, abs=1e-9) and share == pytest.approx(exp["gap_share"], abs=1e-9)


@pytest.mark.parametrize("name", ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup"])
def test_rooms_come_apart_into_their_planes(name):
    _, plane, _, seg = _case(name)
    nseg, pur = int(np.unique(seg).shape[0]), R.purity(seg, plane)
    print(f"{name}: {nseg} segments, purity {pur:.4f}")
    assert nseg <= 40
    assert pur >= 0.95
    exp = _expected()[name]
    assert nseg == exp["segments"] and pur == pytest.approx(exp["purity"], abs=1e-12)


def test_five_sweeps_leave_no_off_diagonal():
    for name in SMALL:
        xyz, _, r, _ = _case(name)
        _, a = R.covariance(xyz, r["knn"])
        _, off, _ = R.jacobi(a)
        assert all(not o.any() for o in off), name


def test_degenerate_neighbourhoods_follow_the_rule():
    xyz, _, r, seg = _case("all_equal")
    assert np.array_equal(r["normals"], np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (xyz.shape[0], 1)))        # column 0 of the identity
    assert np.array_equal(r["knn"], np.tile(np.arange(11, dtype=np.int32), (xyz.shape[0], 1)))                       # equal scores: lowest indices
    assert (r["edges"][:, 0] < r["edges"][:, 1]).all() and np.unique(seg).shape[0] == 1
    xyz, _, r, _ = _case("line")
    d = (xyz[1] - xyz[0]).astype(np.float64)
    n = r["normals"].astype(np.float64)
    assert np.abs(n @ d).max() <= 1e-6 * np.linalg.norm(d) and np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-6  # a unit vector across the line
    # duplicated points: a twin outranks the point itself when its index is lower, and a point's own index further down the list is a
    # self pair, which is no edge
    xyz, _, r, _ = _case("room_dup")
    own = np.arange(xyz.shape[0])
    assert 0 < int((r["knn"][:, 0] != own).sum()) <= 200
    assert int((r["knn"][:, 1:] == own[:, None]).sum()) == _expected()["room_dup"]["self_pairs"] > 0
    assert (r["edges"][:, 0] < r["edges"][:, 1]).all()
    adj = R.pairs_of(r["knn"], keep_self=True)
    assert int((adj[:, 0] == adj[:, 1]).sum()) > 0 and adj.shape[0] - int((adj[:, 0] == adj[:, 1]).sum()) == r["edges"].shape[0]


@pytest.mark.parametrize("name", SMALL)
def test_golden_digests(name):
    xyz, _, r, seg = _case(name)
    exp = _expected()[name]
    assert (xyz.shape[0], r["w"].shape[0], int((r["w"] < 0).sum())) == (exp["N"], exp["edges"], exp["negative_weights"])
    for key, val in R.stage_digests(r, seg).items():
        assert val == exp[key], key
    assert np.array_equal(np.lexsort((r["edges"][:, 1], r["edges"][:, 0], r["w"])), np.arange(r["w"].shape[0])), "ascending (w, a, b)"


def test_negative_weights_occur():
    assert sum(_expected()[n]["negative_weights"] for n in ("room_j0", "room_j5e-4", "room_j2e-3")) > 0


def test_host_chain_equals_the_statement(sg_lib):
    from seggroup_amd import oversegment
    for name in ("room_j5e-4", "room_dup", "n257", "line", "all_equal"):
        xyz, _, r, seg = _case(name)
        assert np.array_equal(oversegment.merge_edges(r["edges"], r["w"], xyz.shape[0]), seg), name
    xyz, _, r, _ = _case("room_j5e-4")
    exp = _expected()["room_j5e-4"]["sweep"]
    for k, m in R.PARAM_SWEEP:
        got = oversegment.merge_edges(r["edges"], r["w"], xyz.shape[0], k, m)
        assert R.digest(got) == exp[f"{k:g}/{m}"], (k, m)


@pytest.mark.parametrize("empty_face_element", [False, True])
def test_a_ply_without_faces_reads_as_a_cloud(tmp_path, empty_face_element):
    from seggroup_amd import prepare
    xyz, _, _, _ = _case("n257")
    rgb = (np.arange(xyz.shape[0] * 3) % 251).astype(np.uint8).reshape(-1, 3)
    p = str(tmp_path / "cloud.ply")
    R.write_vertex_only_ply(p, xyz, rgb, empty_face_element)
    ply = prepare.read_ply(p)
    assert ply["vertex"].count == xyz.shape[0]
    if not empty_face_element:
        with pytest.raises(KeyError):
            ply["face"]
    x, c, f = prepare.mesh_arrays(ply)
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and f.shape == (0, 3) and f.dtype == np.int32
    # a mesh reads as before
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    prepare.write_ply(p, xyz, rgb, faces)
    x, c, f = prepare.mesh_arrays(prepare.read_ply(p))
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and np.array_equal(f, faces)
