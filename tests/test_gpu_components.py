"""Connected components on the GPU: comp, size and C of sg_components_edges / _faces / _knn BIT-EQUAL to the NumPy statement
(tests/components_ref.py) and to the committed digests on every case graph -- empty graphs and paths at the tile edges, long chains in
every edge order and with the minimum mid-chain, a star whose hub is the highest index, two cliques and a bridge, noisy lists, random pairs,
the case meshes through their faces and through their edge lists, an island mesh, the speck cloud's kNN graph at three cuts from both
neighbour searches and with rows of 4 and 6 floats, the label filter --, the refusals on the device, two streams in flight, the thinned
large cloud; an island scan directory through clean_scan -> oversegment -> transfer and the command line in child processes; fragments."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import components_ref as R
import pcseg_ref
import thin_ref
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cases, _solved, _specks = {}, {}, {}
NAMES = sorted(R.case_graphs())


def _case(name):
    if not _cases:
        _cases.update(R.case_graphs())
    return _cases[name]


def _ref(name):
    if name not in _solved:
        _solved[name] = R.solve(_case(name))
    return _solved[name]


def _expected():
    return json.load(open(os.path.join(GOLDEN, "components_expected.json")))


def _run(V, **kw):
    from seggroup_amd import components as M
    comp, size, count = M.components(V, device=DEV, **kw)
    assert str(comp.dtype) == str(size.dtype) == "torch.int32" and comp.is_cuda and size.is_cuda and comp.shape == size.shape == (V,)
    return comp.cpu().numpy(), size.cpu().numpy(), count


def _run_case(case, **kw):
    src = dict(faces=case["faces"]) if "faces" in case else dict(edges=case["edges"])
    return _run(case["V"], labels=case.get("labels"), **src, **kw)


def _same(got, want, what):
    assert got[2] == want[2], f"{what}: C = {got[2]}, the statement has {want[2]}"
    assert np.array_equal(got[0], want[0]), f"{what}: comp"
    assert np.array_equal(got[1], want[1]), f"{what}: size"


@pytest.mark.parametrize("name", NAMES)
def test_components_are_bit_equal_to_the_statement(name):
    got = _run_case(_case(name))
    _same(got, _ref(name), name)
    e = _expected()["graphs"][name]
    assert (e["C"], e["sha256"]) == (got[2], R.digest(got[0])), name
    if "same_as" in _case(name):
        _same(got, _ref(_case(name)["same_as"]), name + " against " + _case(name)["same_as"])
    if name in R.MESH_COUNTS:
        assert got[2] == R.MESH_COUNTS[name][0]


def test_size_may_be_null_and_a_run_repeats(sg_lib):
    import torch
    from seggroup_amd import hip
    case = _case("random")
    v = case["V"]
    d_e = torch.from_numpy(case["edges"]).to(DEV)
    comp = torch.empty(v, dtype=torch.int32, device=DEV)
    ws = torch.empty(sg_lib.sg_components_ws_bytes(v), dtype=torch.uint8, device=DEV)
    c = C.c_int(0)
    hip.check(sg_lib.sg_components_edges(d_e.data_ptr(), d_e.shape[0], v, None, comp.data_ptr(), None, C.byref(c), ws.data_ptr(), ws.numel(), None))
    assert c.value == _ref("random")[2] and np.array_equal(comp.cpu().numpy(), _ref("random")[0])
    a, b = _run_case(case), _run_case(case)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---- the kNN graph with a cut ----------------------------------------------------------------------------------------------------------
def _speck_refs():
    """the speck cloud, the library's kNN table (brute force), the statement's components of it at every cut: computed once"""
    if not _specks:
        from seggroup_amd import prepare
        xyz, tag = R.speck_cloud()
        table = prepare.pointcloud_knn(xyz, 10, device=DEV).cpu().numpy()
        _specks.update(xyz=xyz, tag=tag, table=table, cuts={cut: R.from_knn(xyz, table, cut) for cut in R.CUTS})
    return _specks


@pytest.mark.parametrize("cut", R.CUTS)
def test_knn_graph_with_a_cut(cut):
    from seggroup_amd import prepare
    s = _speck_refs()
    n = s["xyz"].shape[0]
    assert n == 5307 and s["table"].shape == (n, 11)
    got = _run(n, knn=s["table"], xyz=s["xyz"], max_edge=None if cut == np.inf else cut)
    _same(got, s["cuts"][cut], "cut %g" % cut)
    e = _expected()["specks"]["%g" % cut]
    assert (e["C"], e["sizes"], e["sha256"]) == (got[2], R.sizes_desc(got[0])[:10], R.digest(got[0])), "the digest of the statement on its own table"
    if cut == np.inf:
        _same(_run(n, knn=s["table"], xyz=s["xyz"], max_edge=np.inf), s["cuts"][cut], "max_edge = inf")
        _same(_run(n, edges=pcseg_ref.cloud_edges(s["table"])), s["cuts"][cut], "the edge form of the same table")
    grid = prepare.pointcloud_knn(s["xyz"], 10, device=DEV, index="grid")
    _same(_run(n, knn=grid, xyz=s["xyz"], max_edge=cut), s["cuts"][cut], "the grid index's table")
    rng = np.random.RandomState(2)
    for extra in (1, 3):
        rows = np.concatenate([s["xyz"], rng.uniform(-9, 9, (n, extra)).astype(np.float32)], 1)
        _same(_run(n, knn=s["table"], xyz=rows, max_edge=cut), s["cuts"][cut], "rows of %d floats" % (3 + extra))
    shifted = s["table"].copy()
    shifted[:, 0] = n - 1                                       # entry 0 is skipped whatever it holds
    _same(_run(n, knn=shifted, xyz=s["xyz"], max_edge=cut), s["cuts"][cut], "entry 0 overwritten")
    lab = (s["tag"] > 0).astype(np.int32)
    _same(_run(n, knn=s["table"], xyz=s["xyz"], max_edge=cut, labels=lab), R.from_knn(s["xyz"], s["table"], cut, labels=lab), "with a filter")


def test_short_rows_of_the_table():
    s = _speck_refs()
    n = s["xyz"].shape[0]
    for row in (2, 6):
        t = np.ascontiguousarray(s["table"][:, :row])
        _same(_run(n, knn=t, xyz=s["xyz"], max_edge=0.1), R.from_knn(s["xyz"], t, 0.1), "rows of %d entries" % row)


def test_the_thinned_large_cloud():
    """thin_ref.big_cloud() thinned at 0.05 on the device (the 5,403 points of 8i's test), k = 10, cut at three voxel edges (one component) and at one (497 of many sizes)"""
    from seggroup_amd import prepare, thin
    xyz, _ = thin_ref.big_cloud()
    rep, _, _ = thin.thin_cloud(xyz, 0.05, device=DEV)
    pts = xyz[rep.cpu().numpy()]
    assert pts.shape[0] == 5403
    table = prepare.pointcloud_knn(pts, 10, device=DEV, index="grid")
    for cut, key in ((3 * 0.05, "big_thinned"), (0.05, "big_thinned_tight")):
        got = _run(5403, knn=table, xyz=pts, max_edge=cut)
        _same(got, R.from_knn(pts, table.cpu().numpy(), cut), key)
        e = _expected()[key]
        assert (e["C"], e["sizes"], e["sha256"]) == (got[2], R.sizes_desc(got[0])[:10], R.digest(got[0])), key


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_leave_the_library_usable(sg_lib):
    from seggroup_amd import hip
    s = _speck_refs()
    n = s["xyz"].shape[0]
    good = _case("island")
    for bad_index in (good["V"], -1, 1 << 30, -(1 << 31)):
        e = R.island_mesh()["faces"][:, :2].copy()
        e[e.shape[0] // 2, 1] = bad_index
        f = good["faces"].copy()
        f[7, 2] = bad_index
        t = s["table"].copy()
        t[n // 2, 10] = n if bad_index == good["V"] else bad_index
        for kw, v in ((dict(edges=e), good["V"]), (dict(faces=f), good["V"]), (dict(knn=t, xyz=s["xyz"], max_edge=0.1), n)):
            with pytest.raises(hip.SgError) as ei:
                _run(v, **kw)
            assert ei.value.code == hip.SG_EINVAL and "index outside" in str(ei.value), (bad_index, list(kw))
        _same(_run_case(good), _ref("island"), "after a refusal")
    t = s["table"].copy()
    t[5, 0] = -9                                                # entry 0 is not read: not an error
    _same(_run(n, knn=t, xyz=s["xyz"], max_edge=0.1), s["cuts"][0.1], "entry 0 out of range")
    for bad in (np.nan, np.inf, -np.inf):
        x = s["xyz"].copy()
        x[n - 1, 1] = bad
        with pytest.raises(hip.SgError) as ei:
            _run(n, knn=s["table"], xyz=x)
        assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    _same(_run(n, knn=s["table"], xyz=s["xyz"], max_edge=0.06), s["cuts"][0.06], "after a refusal")
    # before the first device call: the arguments (tests/test_components_ref.py has the full list)
    import torch
    ws = torch.empty(sg_lib.sg_components_ws_bytes(n), dtype=torch.uint8, device=DEV)
    comp = torch.empty(n, dtype=torch.int32, device=DEV)
    d_x, d_t, c = torch.from_numpy(s["xyz"]).to(DEV), torch.from_numpy(s["table"]).to(DEV), C.c_int(0)
    for bad in (0.0, -0.1, float("nan")):
        assert sg_lib.sg_components_knn(d_x.data_ptr(), 3, d_t.data_ptr(), n, 11, bad, None, comp.data_ptr(), None, C.byref(c), ws.data_ptr(),
                                        ws.numel(), None) == hip.SG_EINVAL
    assert sg_lib.sg_components_knn(d_x.data_ptr(), 3, d_t.data_ptr(), n, 11, 0.1, None, comp.data_ptr(), None, C.byref(c), ws.data_ptr(),
                                    ws.numel() - 1, None) == hip.SG_EINVAL
    assert b"workspace too small" in sg_lib.sg_last_error()
    assert sg_lib.sg_components_ws_bytes(hip.MAX_CLOUD_POINTS + 1) == 0
    with pytest.raises(hip.SgError) as ei:
        _run(hip.MAX_CLOUD_POINTS + 1, edges=np.zeros((0, 2), np.int32))
    assert ei.value.code == hip.SG_EUNSUP


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
def test_two_streams_in_flight_give_the_same_bytes_as_alone():
    import torch
    from seggroup_amd import components as M
    names = ("random_noisy", "mesh_raw_scan")
    out, errors = {}, []

    def work(name):
        try:
            stream = torch.cuda.Stream(device=DEV)
            case = _case(name)
            src = dict(faces=case["faces"]) if "faces" in case else dict(edges=case["edges"])
            runs = []
            for _ in range(6):
                comp, size, count = M.components(case["V"], device=DEV, stream=stream, **src)
                runs.append((comp.cpu().numpy(), size.cpu().numpy(), count))
            out[name] = runs
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name in names:
        for got in out[name]:
            _same(got, _ref(name), name + " beside another stream")


def test_stage_times(sg_lib):
    sg_lib.sg_components_set_timing(1)
    try:
        _run_case(_case("mesh_raw_scan"))
        us = (C.c_float * 4)()
        assert sg_lib.sg_components_stage_times(us, 4) == 4
        assert all(0.0 < t < 1e6 for t in us), list(us)
    finally:
        sg_lib.sg_components_set_timing(0)


# ---- scan directories ------------------------------------------------------------------------------------------------------------------
AGG = b'{"sceneId": "x", "segGroups": [ {"id": 0, "label": "floor", "segments": [3, 10]} ]}\n'
PLY = "_vh_clean_2.ply"


def _island_scan(scans_dir, name, faceless=False):
    from seggroup_amd import oversegment, prepare
    isl = R.island_mesh()
    sp = os.path.join(scans_dir, name)
    os.makedirs(sp)
    if faceless:
        pcseg_ref.write_vertex_only_ply(os.path.join(sp, name + PLY), isl["xyz"], isl["rgb"])
    else:
        prepare.write_ply(os.path.join(sp, name + PLY), isl["xyz"], isl["rgb"], isl["faces"])
    doc = {"params": {"kThresh": "0.010000", "segMinVerts": "20"}, "sceneId": name, "segIndices": isl["seg_indices"].tolist(), "tool": "by hand"}
    with open(os.path.join(sp, oversegment.segs_json_name(name)), "w") as f:
        json.dump(doc, f)
    with open(os.path.join(sp, name + ".aggregation.json"), "wb") as f:
        f.write(AGG)
    return isl


def _check_cleaned_scan(dst, name, isl, entry, source, faces_in, want):
    """min_verts = 20 on the island scan: exactly the patches of 3 and 12 vertices are gone.  want: the statement's (comp, size, C)"""
    from seggroup_amd import oversegment, prepare
    keep = R.keep_mask(want[0], want[1], min_verts=20)
    assert np.array_equal(keep, ~np.isin(isl["patch"], (3, 12)))
    kept, new_of_old, faces = R.clean_arrays(keep, faces_in)
    m = kept.shape[0]
    assert m == isl["xyz"].shape[0] - 15
    xyz, rgb, got_faces = prepare.mesh_arrays(prepare.read_ply(os.path.join(dst, name + PLY)))
    assert xyz.tobytes() == isl["xyz"][kept].tobytes() and np.array_equal(rgb, isl["rgb"][kept])
    assert np.array_equal(got_faces, faces) and (got_faces.size == 0 or (got_faces.min() >= 0 and got_faces.max() < m))
    with np.load(os.path.join(dst, name + ".clean.npz")) as z:
        assert np.array_equal(z["kept"], kept) and np.array_equal(z["new_of_old"], new_of_old) and z["kept"].dtype == z["new_of_old"].dtype == np.int32
        assert z["comp"].dtype == np.int32 and np.array_equal(z["comp"], want[0])
        assert int(z["min_verts"]) == 20 and not bool(z["largest"]) and str(z["source"]) == source
    doc = json.load(open(os.path.join(dst, oversegment.segs_json_name(name))))
    assert doc["segIndices"] == isl["seg_indices"][kept].tolist() and doc["tool"] == "by hand" and doc["sceneId"] == name
    assert open(os.path.join(dst, name + ".aggregation.json"), "rb").read() == AGG
    before = np.unique(isl["seg_indices"])
    assert entry["V"] == isl["xyz"].shape[0] and entry["M"] == m and entry["components"] == want[2]
    assert entry["kept_components"] == np.unique(want[0][keep]).shape[0] == want[2] - 2
    assert entry["largest_sizes"] == R.sizes_desc(want[0])[:10] and entry["source"] == source
    assert entry["source_segments"] == before.shape[0] and entry["kept_segments"] == before.shape[0] - 2
    assert entry["lost_segments"] == [100003, 100012]
    return kept, new_of_old


def test_island_scan_is_cleaned_and_read_by_the_other_commands(tmp_path):
    from seggroup_amd import components as M
    from seggroup_amd import oversegment, prepare, transfer
    name = "scene0051_00"
    raw, out = str(tmp_path / "raw"), str(tmp_path / "clean")
    isl = _island_scan(raw, name)
    entry = M.clean_scan(os.path.join(raw, name), out, min_verts=20, device=DEV)
    kept, new_of_old = _check_cleaned_scan(os.path.join(out, name), name, isl, entry, "faces", isl["faces"], _ref("island"))
    assert entry["largest_sizes"] == [1200, 60, 12, 3]
    assert (entry["F"], entry["kept_F"]) == (isl["faces"].shape[0], isl["faces"].shape[0] - 1 - 12)
    assert M.clean_scan(os.path.join(raw, name), out, min_verts=20, device=DEV) is None, "never overwritten without force"
    # the cleaned tree is a scan tree: the over-segmenter reads it
    path = oversegment.oversegment_scan(os.path.join(out, name), force=True, device=DEV)
    seg = np.asarray(prepare.load_seg_labels(path))
    assert seg.shape == (kept.shape[0],)
    # results go back through the nearest kept vertex: a kept vertex is its own, at distance 0
    clean_xyz = prepare.mesh_arrays(prepare.read_ply(os.path.join(out, name, name + PLY)))[0]
    nearest, d2 = transfer.nearest_vertex(clean_xyz, isl["xyz"], device=DEV)
    nearest, d2 = nearest.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(nearest[kept], new_of_old[kept]) and not d2[kept].any() and (d2[new_of_old < 0] > 1.0).all()
    # cleaning the cleaned scan changes nothing
    again = str(tmp_path / "again")
    e2 = M.clean_scan(os.path.join(out, name), again, min_verts=20, device=DEV)
    assert e2["M"] == e2["V"] == kept.shape[0] and e2["components"] == e2["kept_components"] == 2 and e2["lost_segments"] == []
    assert e2["largest_sizes"] == [1200, 60]
    assert open(os.path.join(again, name, name + PLY), "rb").read() == open(os.path.join(out, name, name + PLY), "rb").read()
    # largest: the room alone; report_only writes nothing
    e3 = M.clean_scan(os.path.join(raw, name), str(tmp_path / "none"), largest=True, device=DEV, report_only=True)
    assert e3["M"] == 1200 and e3["kept_components"] == 1 and not os.path.exists(str(tmp_path / "none"))


def test_command_line_in_child_processes(tmp_path):
    mesh, cloud = "scene0052_00", "scene0053_00"
    raw, raw_pc = str(tmp_path / "raw"), str(tmp_path / "raw_pc")
    isl = _island_scan(raw, mesh)
    _island_scan(raw_pc, cloud, faceless=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.components"]

    def run(*args):
        return subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)

    out = str(tmp_path / "clean")
    r = run("--scans", raw, "--out", out, "--min-verts", "20", "--workers", "2")
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    report = json.load(open(os.path.join(out, "clean_report.json")))
    assert report["min_verts"] == 20 and report["largest"] is False and list(report["scenes"]) == [mesh] and report["skipped"] == []
    _check_cleaned_scan(os.path.join(out, mesh), mesh, isl, report["scenes"][mesh], "faces", isl["faces"], _ref("island"))
    r = run("--scans", raw, "--out", out, "--min-verts", "20")
    assert r.returncode == 0 and "0 written, 1 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    # the face-less twin: the kNN graph, cut at 0.1
    out_pc = str(tmp_path / "clean_pc")
    r = run("--scans", raw_pc, "--out", out_pc, "--min-verts", "20", "--pointcloud", "--max-edge", "0.1", "--knn", "10", "--index", "grid")
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    report = json.load(open(os.path.join(out_pc, "clean_report.json")))
    assert report["max_edge"] == 0.1 and report["pointcloud"] is True
    from seggroup_amd import prepare
    want = R.from_knn(isl["xyz"], prepare.pointcloud_knn(isl["xyz"], 10, device=DEV).cpu().numpy(), 0.1)
    assert R.sizes_desc(want[0]) == [1134, 66, 60, 12, 3], "the kNN graph of the room alone is in two pieces"
    _check_cleaned_scan(os.path.join(out_pc, cloud), cloud, isl, report["scenes"][cloud], "knn", np.zeros((0, 3), np.int32), want)
    # --report-only writes the report alone
    out_r = str(tmp_path / "report")
    r = run("--scans", raw, "--out", out_r, "--largest", "--report-only")
    assert r.returncode == 0 and "1 reported" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert os.listdir(out_r) == ["clean_report.json"] and json.load(open(os.path.join(out_r, "clean_report.json")))["scenes"][mesh]["M"] == 1200
    # parser errors, not silent defaults
    for args in (("--scans", raw, "--out", out), ("--scans", raw, "--out", out, "--min-verts", "20", "--largest"),
                 ("--scans", raw_pc, "--out", out, "--min-verts", "20"), ("--scans", raw, "--out", out, "--largest", "--pointcloud")):
        r = run(*args)
        assert r.returncode == 2 and "error:" in r.stderr, args


# ---- fragments ---------------------------------------------------------------------------------------------------------------------------
def test_fragments_of_an_instance_in_two_patches(tmp_path):
    from seggroup_amd import components as M
    from seggroup_amd import pseudo_labels
    name = "scene0054_00"
    raw = str(tmp_path / "raw")
    isl = _island_scan(raw, name)
    v = isl["xyz"].shape[0]
    lab = np.where(isl["patch"] == 0, 1, np.where(isl["patch"] == 3, 3, 2)).astype(np.int32)      # instance 2: the patches of 12 and 60
    want = {"V": v, "instances": 3, "fragmented": 1, "outside_largest": 12, "outside_share": 12 / v, "pieces": {2: [60, 12]}}
    assert M.fragments(lab, v, faces=isl["faces"], device=DEV) == want
    assert M.fragments(isl["patch"], v, faces=isl["faces"], device=DEV)["pieces"] == {}
    half = lab.copy()
    half[np.flatnonzero(isl["patch"] == 60)[:1]] = 7             # a corner vertex of the patch of 60 on its own
    got = M.fragments(half, v, faces=isl["faces"], device=DEV)
    assert got["pieces"] == {2: [59, 12]} and got["instances"] == 4 and got["outside_largest"] == 12
    # through the files: final.ins of a .sgl whose segments are the room, the two patches, the triangle
    sov = np.where(isl["patch"] == 0, 0, np.where(isl["patch"] == 3, 2, 1)).astype(np.int32)
    tables = np.zeros((pseudo_labels.INS_NVEC, 3), np.int32)
    tables[12] = [1, 2, 3]
    src = os.path.join(str(tmp_path), "results", "e", name, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    got = M.fragments_scene(os.path.join(raw, name), "e", "epoch_last", root=str(tmp_path), device=DEV)
    assert got == dict(want, pieces={"2": [60, 12]}, source="faces")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    path = str(tmp_path / "fragments.json")
    r = subprocess.run([sys.executable, "-m", "seggroup_amd.components", "--fragments", "--scans", raw, "-n", "e", "--stage", "epoch_last", "--root",
                        str(tmp_path), "--json", path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 in pieces" in r.stdout, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(path))
    assert doc["layer"] == "final" and doc["scenes"][name]["pieces"] == {"2": [60, 12]} and doc["scenes"][name]["outside_largest"] == 12
