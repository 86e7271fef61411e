"""Connected components without a GPU: the NumPy statement (tests/components_ref.py) against scipy's connected_components on
every case, the face form against the edge form, the kNN form without a cut against the over-segmenter's edge list, the counts measured
for 8j and the committed digests (tests/golden/components_expected.json, tools/capture_components.py), the refusals the library and the
module make before any device call, and the index arithmetic of `clean` through a PLY round trip."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import components_ref as R
import overseg_ref
import pcseg_ref
from conftest import GOLDEN

_cases, _solved, _specks = {}, {}, {}


def _case(name):
    if not _cases:
        _cases.update(R.case_graphs())
    return _cases[name]


def _ref(name):
    if name not in _solved:
        _solved[name] = R.solve(_case(name))
    return _solved[name]


def _speck_refs():
    """the speck cloud, its kNN table by the statement of 8f, and the components at every cut: computed once"""
    if not _specks:
        xyz, tag = R.speck_cloud()
        table = pcseg_ref.knn_table(xyz, 10)
        _specks.update(xyz=xyz, tag=tag, table=table, cuts={cut: R.from_knn(xyz, table, cut) for cut in R.CUTS})
    return _specks


NAMES = sorted(R.case_graphs())


def _expected():
    return json.load(open(os.path.join(GOLDEN, "components_expected.json")))


def _scipy_comp(num_vertices, a, b):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    g = sp.coo_matrix((np.ones(a.shape[0], np.int8), (a, b)), shape=(num_vertices, num_vertices))
    count, lab = connected_components(g, directed=False)
    low = np.full(count, num_vertices, np.int64)
    np.minimum.at(low, lab, np.arange(num_vertices))
    return low[lab].astype(np.int32), count


def _pairs(case):
    a, b = R.pairs_from_faces(case["faces"], case["V"]) if "faces" in case else R.pairs_from_edges(case["edges"], case["V"])
    if case.get("labels") is not None:
        same = case["labels"][a] == case["labels"][b]
        a, b = a[same], b[same]
    return a, b


@pytest.mark.parametrize("name", NAMES)
def test_statement_equals_scipy(name):
    case = _case(name)
    comp, size, count = _ref(name)
    want, want_count = _scipy_comp(case["V"], *_pairs(case))
    assert comp.dtype == np.int32 and size.dtype == np.int32
    assert np.array_equal(comp, want) and count == want_count
    assert np.array_equal(size, np.bincount(comp, minlength=case["V"])[comp]) and count == int((comp == np.arange(case["V"])).sum())
    assert (comp <= np.arange(case["V"])).all() and np.array_equal(comp[comp], comp)


def test_statement_equals_scipy_on_the_knn_graphs():
    s = _speck_refs()
    for cut in R.CUTS:
        comp, _, count = s["cuts"][cut]
        want, want_count = _scipy_comp(s["xyz"].shape[0], *R.pairs_from_knn(s["xyz"], s["table"], cut))
        assert np.array_equal(comp, want) and count == want_count, cut


@pytest.mark.parametrize("name", [n for n in NAMES if "same_as" in R.case_graphs()[n]])
def test_equivalent_forms_give_the_same_bytes(name):
    """faces == the unique edge list of the faces; a noisy list == the clean one; all labels equal == no filter"""
    other = _case(name)["same_as"]
    for x, y in zip(_ref(name), _ref(other)):
        assert np.array_equal(x, y), (name, other)


def test_knn_form_without_a_cut_equals_the_cloud_edges():
    s = _speck_refs()
    n = s["xyz"].shape[0]
    want = R.from_edges(n, pcseg_ref.cloud_edges(s["table"]))
    for x, y in zip(s["cuts"][np.inf], want):
        assert np.array_equal(x, y)
    rows6 = np.concatenate([s["xyz"], np.full_like(s["xyz"], 7.0)], 1)
    assert np.array_equal(R.from_knn(rows6, s["table"], 0.1)[0], s["cuts"][0.1][0]), "columns past xyz are not read"
    shifted = s["table"].copy()
    shifted[:, 0] = 0                                           # entry 0 is skipped whatever it holds
    assert np.array_equal(R.from_knn(s["xyz"], shifted, 0.1)[0], s["cuts"][0.1][0])


def test_counts_of_8j():
    for name, (count, sizes) in R.MESH_COUNTS.items():
        comp, _, c = _ref(name)
        assert c == count, name
        if sizes is not None:
            assert R.sizes_desc(comp) == sizes, name
    s = _speck_refs()
    assert s["xyz"].shape[0] == 5307
    table = {np.inf: [5292, 15], 0.1: [5281, 15, 8, 3], 0.06: [2081, 1600, 1600, 15, 8, 3]}
    for cut, sizes in table.items():
        comp, _, count = s["cuts"][cut]
        assert R.sizes_desc(comp) == sizes and count == len(sizes), cut
    comp = s["cuts"][0.1][0]
    for n in (8, 15, 3):                                        # at 0.1 every speck is a component of its own
        assert np.unique(comp[s["tag"] == n]).shape[0] == 1 and (comp == comp[s["tag"] == n][0]).sum() == n
    assert _ref("filter_all_distinct")[2] == _case("filter_all_distinct")["V"]
    assert _ref("star_hub_highest")[2] == 1 and _ref("two_cliques_bridge_last")[2] == 1
    assert _ref("chain_permuted")[2] == 1 and not _ref("chain_permuted")[0].any()
    sizes = R.sizes_desc(_ref("random")[0])
    assert len(set(sizes)) > 10 and sizes[0] > 1000 and sizes[-1] == 1, "many components of many sizes"


def test_committed_digests():
    exp = _expected()
    assert sorted(exp["graphs"]) == NAMES
    for name in NAMES:
        comp, _, count = _ref(name)
        e = exp["graphs"][name]
        assert (e["V"], e["C"], e["sizes"], e["sha256"]) == (_case(name)["V"], count, R.sizes_desc(comp)[:10], R.digest(comp)), name
    s = _speck_refs()
    for cut in R.CUTS:
        comp, _, count = s["cuts"][cut]
        e = exp["specks"]["%g" % cut]
        assert (e["C"], e["sizes"], e["sha256"]) == (count, R.sizes_desc(comp)[:10], R.digest(comp)), cut


def test_statement_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        R.from_edges(4, [[0, 4]])
    with pytest.raises(ValueError):
        R.from_faces(4, [[0, 1, -1]])
    xyz, table = np.zeros((3, 3), np.float32), np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1]])
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            R.from_knn(xyz, table, bad)
    with pytest.raises(ValueError):
        R.from_knn(xyz, np.array([[0, 1, 3]] * 3))
    nan = xyz.copy()
    nan[1, 2] = np.nan
    with pytest.raises(ValueError):
        R.from_knn(nan, table)


# ---- the library's and the module's refusals before any device call -------------------------------------------------------------------
def test_library_refuses_before_the_first_device_call(sg_lib):
    from seggroup_amd import hip
    cap = hip.MAX_CLOUD_POINTS
    ws = sg_lib.sg_components_ws_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(cap + 1) == 0
    assert ws(1) >= 8 and ws(cap) >= 2 * 4 * cap and ws(257) > ws(1)
    buf = (C.c_char * 64)()                                     # never read: every call below is refused on its arguments
    p, c = C.addressof(buf), C.c_int(-1)
    big = 1 << 40
    edges, faces, knn = sg_lib.sg_components_edges, sg_lib.sg_components_faces, sg_lib.sg_components_knn
    inf = float("inf")
    calls = {
        "null comp": (edges(p, 1, 4, None, None, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "null count": (edges(p, 1, 4, None, p, None, None, p, big, None), hip.SG_EINVAL),
        "null workspace": (edges(p, 1, 4, None, p, None, C.byref(c), None, big, None), hip.SG_EINVAL),
        "null edges": (edges(None, 1, 4, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "no vertex": (edges(p, 1, 0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "negative E": (edges(p, -1, 4, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "E at the cap": (edges(p, 1 << 30, 4, None, p, None, C.byref(c), p, big, None), hip.SG_EUNSUP),
        "V above the cap": (edges(p, 1, cap + 1, None, p, None, C.byref(c), p, big, None), hip.SG_EUNSUP),
        "short workspace": (edges(p, 1, 1000, None, p, None, C.byref(c), p, ws(1000) - 1, None), hip.SG_EINVAL),
        "negative F": (faces(p, -1, 4, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "null faces": (faces(None, 2, 4, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "faces, V above the cap": (faces(p, 1, cap + 1, None, p, None, C.byref(c), p, big, None), hip.SG_EUNSUP),
        "faces, short workspace": (faces(p, 1, 1000, None, p, None, C.byref(c), p, 16, None), hip.SG_EINVAL),
        "null points": (knn(None, 3, p, 4, 11, inf, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "null table": (knn(p, 3, None, 4, 11, inf, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "stride 2": (knn(p, 2, p, 4, 11, inf, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "row 1": (knn(p, 3, p, 4, 1, inf, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "max_edge 0": (knn(p, 3, p, 4, 11, 0.0, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "max_edge negative": (knn(p, 3, p, 4, 11, -0.5, None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "max_edge NaN": (knn(p, 3, p, 4, 11, float("nan"), None, p, None, C.byref(c), p, big, None), hip.SG_EINVAL),
        "knn, N above the cap": (knn(p, 3, p, cap + 1, 11, inf, None, p, None, C.byref(c), p, big, None), hip.SG_EUNSUP),
        "knn, short workspace": (knn(p, 3, p, 1000, 11, 0.1, None, p, None, C.byref(c), p, ws(1000) - 1, None), hip.SG_EINVAL),
    }
    for what, (rc, want) in calls.items():
        assert rc == want, what
    assert hip.SG_EINTERNAL == -6
    assert [sg_lib.sg_components_stage_name(i) for i in range(5)] == [b"init", b"hook", b"flatten", b"sizes", None]
    assert sg_lib.sg_components_stage_times(None, 4) == hip.SG_EINVAL


def test_module_refuses_before_a_device_call():
    from seggroup_amd import components as M
    e, f = np.zeros((2, 2), np.int32), np.zeros((2, 3), np.int32)
    t, x = np.zeros((4, 11), np.int32), np.zeros((4, 3), np.float32)
    bad = [dict(), dict(edges=e, faces=f), dict(edges=e, knn=t, xyz=x), dict(knn=t), dict(edges=e, xyz=x), dict(edges=e, max_edge=0.1),
           dict(edges=f), dict(faces=e), dict(knn=t[:, :1], xyz=x), dict(knn=t, xyz=x[:, :2]), dict(knn=t, xyz=x[:3]), dict(knn=t[:3], xyz=x),
           dict(knn=t, xyz=x, max_edge=0.0), dict(knn=t, xyz=x, max_edge=-1.0), dict(knn=t, xyz=x, max_edge=float("nan")),
           dict(edges=e, labels=np.zeros(3, np.int32)), dict(edges=e.reshape(-1))]
    for kw in bad:
        with pytest.raises(ValueError):
            M.components(4, **kw)
    with pytest.raises(ValueError):
        M.components(0, edges=e)
    comp, size = np.array([0, 0, 2, 0], np.int32), np.array([3, 3, 1, 3], np.int32)
    for kw in (dict(), dict(min_verts=2, largest=True), dict(min_verts=0)):
        with pytest.raises(ValueError):
            M.keep_mask(comp, size, **kw)
    with pytest.raises(ValueError):
        M.clean_scan("nowhere/scene0000_00", "out")
    with pytest.raises(ValueError):
        M.clean_scan("nowhere/scene0000_00", "out", min_verts=3, largest=True)


def test_command_line_refuses_instead_of_guessing(tmp_path, capsys):
    from seggroup_amd import components as M
    from seggroup_amd.prepare import write_ply
    isl = R.island_mesh()
    scans = tmp_path / "scans"
    for scene, faces in (("mesh0000_00", isl["faces"]), ("cloud0000_00", np.zeros((0, 3), np.int32))):
        os.makedirs(scans / scene)
        write_ply(str(scans / scene / (scene + "_vh_clean_2.ply")), isl["xyz"], isl["rgb"], faces)
    only_mesh = tmp_path / "mesh.txt"
    only_mesh.write_text("mesh0000_00\n")
    base = ["--scans", str(scans), "--out", str(tmp_path / "out")]
    wrong = [base, base + ["--min-verts", "20", "--largest"], base + ["--min-verts", "0"], base + ["--min-verts", "20"],
             base + ["--min-verts", "20", "--scenes", str(only_mesh), "--pointcloud"],
             base + ["--min-verts", "20", "--scenes", str(only_mesh), "--max-edge", "0.1"],
             base + ["--min-verts", "20", "--max-edge", "0"], base + ["--min-verts", "20", "--max-edge", "inf"],
             base + ["--min-verts", "20", "--max-edge", "0.1", "--knn", "7"], base + ["--largest", "--workers", "17"],
             ["--scans", str(scans), "--largest"], ["--fragments", "--scans", str(scans)],
             ["--fragments", "--scans", str(scans), "-n", "exp", "--largest"]]
    for argv in wrong:
        with pytest.raises(SystemExit) as ei:
            M.main(argv)
        assert ei.value.code == 2, argv
    assert "--max-edge" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


# ---- the index arithmetic of `clean` --------------------------------------------------------------------------------------------------
def test_keep_mask():
    torch = pytest.importorskip("torch")
    from seggroup_amd import components as M
    comp, size, _ = _ref("island")
    for kw in (dict(min_verts=1), dict(min_verts=4), dict(min_verts=13), dict(min_verts=61), dict(min_verts=5000), dict(largest=True)):
        want = R.keep_mask(comp, size, **kw)
        assert np.array_equal(M.keep_mask(comp, size, **kw), want)
        assert np.array_equal(M.keep_mask(torch.from_numpy(comp), torch.from_numpy(size), **kw).numpy(), want), kw
    assert R.keep_mask(comp, size, min_verts=13).sum() == 1260 and R.keep_mask(comp, size, largest=True).sum() == 1200
    comp, size = np.array([0, 1, 1, 0, 4], np.int32), np.array([2, 2, 2, 2, 1], np.int32)       # two largest: the lowest comp
    assert M.keep_mask(comp, size, largest=True).tolist() == [True, False, False, True, False]


def test_clean_arrays_and_the_ply_round_trip(tmp_path):
    torch = pytest.importorskip("torch")
    from seggroup_amd import components as M
    from seggroup_amd.prepare import mesh_arrays, read_ply, write_ply
    isl = R.island_mesh()
    comp, size, _ = _ref("island")
    v = comp.shape[0]
    for min_verts, m in ((1, v), (4, v - 3), (20, v - 15), (61, 1200)):
        keep = R.keep_mask(comp, size, min_verts=min_verts)
        kept, new_of_old, faces = R.clean_arrays(keep, isl["faces"])
        got = [t.numpy() for t in M.clean_arrays(torch.from_numpy(keep), torch.from_numpy(isl["faces"]))]
        assert all(g.dtype == np.int32 for g in got)
        assert np.array_equal(got[0], kept) and np.array_equal(got[1], new_of_old) and np.array_equal(got[2], faces)
        assert kept.shape[0] == m and (np.diff(kept) > 0).all() and np.array_equal(new_of_old[kept], np.arange(m))
        assert (new_of_old[~keep] == -1).all() and faces.min() >= 0 and faces.max() < m
        assert np.array_equal(kept[faces], isl["faces"][keep[isl["faces"]].all(1)]), "the kept faces, in their original order"
        assert np.array_equal(keep[isl["faces"]].all(1), keep[isl["faces"]].any(1)), "a face is kept or dropped whole"
        path = str(tmp_path / ("m%d.ply" % min_verts))
        write_ply(path, isl["xyz"][kept], isl["rgb"][kept], faces)
        xyz, rgb, back = mesh_arrays(read_ply(path))
        assert xyz.tobytes() == isl["xyz"][kept].tobytes() and np.array_equal(rgb, isl["rgb"][kept]) and np.array_equal(back, faces)
        if min_verts == 1:                                      # nothing dropped: the source's vertices and faces
            assert xyz.tobytes() == isl["xyz"].tobytes() and np.array_equal(back, isl["faces"]) and np.array_equal(kept, np.arange(v))
    kept, new_of_old, faces = R.clean_arrays(np.zeros(5, bool), np.array([[0, 1, 2]]))
    assert kept.shape == (0,) and (new_of_old == -1).all() and faces.shape == (0, 3)
    got = M.clean_arrays(torch.zeros(5, dtype=torch.bool), torch.zeros((0, 3), dtype=torch.int32))
    assert got[0].shape == (0,) and got[2].shape == (0, 3)
    assert overseg_ref.mesh_edges(isl["faces"], v).shape[0] > 0
