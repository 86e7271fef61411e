"""Point-cloud over-segmentation on the GPU: every device stage -- the kNN table, the covariance normals, the edge set, the
weights, the sorted order -- and the final ids BIT-EQUAL to the NumPy statement of the specification (tests/pcseg_ref.py) on every
generated cloud (rooms with and without jitter, duplicated points, N = k + 1, the tile edge, a line, one point 32 times, a 20k room);
k, the chain's parameters and the viewpoint; determinism; sg_pointcloud_adjacency against the table; the refusals; a scan directory
whose PLY has no faces through prepare_scene(oversegment=True) -> pack -> SegModel.forward; the command line in a child process; and
the mesh path's committed digests, which guard the stages the two segmenters now share."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import overseg_ref
import pcseg_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CASES = ["room_j0", "room_j5e-4", "room_j2e-3", "room_dup", "n_k_plus_1", "n255", "n256", "n257", "line", "all_equal", "room_20k"]
SWEEP_CASE = "room_j5e-4"
_clouds, _refs = {}, {}


def _cloud(name):
    if not _clouds:
        _clouds.update(R.case_clouds(include_large=True))
    return _clouds[name][0]


def _ref(name, k=10):
    """the statement's stages of one cloud, computed once and shared"""
    if (name, k) not in _refs:
        _refs[(name, k)] = R.sorted_edges(_cloud(name), k)
    return _refs[(name, k)]


def _expected():
    return json.load(open(os.path.join(GOLDEN, "pcseg_expected.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {np.argwhere(diff)[0].tolist()}: " \
                           f"{got[tuple(np.argwhere(diff)[0])]!r} != {want[tuple(np.argwhere(diff)[0])]!r}"


def _check_stages(got, ref, n, what):
    """a dict of pointcloud_edges against the statement's: table, normals, edge set, weights per edge, order"""
    knn = got["knn"].cpu().numpy()
    assert knn.dtype == np.int32 and np.array_equal(knn, ref["knn"]), f"{what}: kNN table"
    _same_bits(got["normals"].cpu().numpy(), ref["normals"], f"{what}: normals")
    got_e, got_w = got["edges"].cpu().numpy(), got["w"].cpu().numpy()
    assert got_e.dtype == np.int32 and got_e.shape == ref["edges"].shape, f"{what}: edge count"
    key = lambda e: e[:, 0].astype(np.int64) * n + e[:, 1]                      # noqa: E731
    assert np.array_equal(np.sort(key(got_e)), key(ref["lex_edges"])), f"{what}: edge set"
    _same_bits(got_w[np.argsort(key(got_e), kind="stable")], ref["lex_w"], f"{what}: weights")
    assert np.array_equal(got_e, ref["edges"]), f"{what}: sorted order"
    _same_bits(got_w, ref["w"], f"{what}: sorted weights")
    return got_e, got_w


@pytest.mark.parametrize("name", CASES)
def test_every_stage_is_bit_equal_to_the_statement(name):
    from seggroup_amd import oversegment, prepare
    xyz, ref, exp = _cloud(name), _ref(name), _expected()[name]
    n = xyz.shape[0]
    got_e, got_w = _check_stages(oversegment.pointcloud_edges(xyz, device="cuda:0"), ref, n, name)
    assert got_e.shape[0] == exp["edges"] and int((got_w < 0).sum()) == exp["negative_weights"]
    # the public functions of the single stages
    table = prepare.pointcloud_knn(xyz, 10, device="cuda:0")
    assert tuple(table.shape) == (n, 11) and np.array_equal(table.cpu().numpy(), ref["knn"])
    _same_bits(oversegment.pointcloud_normals(xyz, 10, knn=table, device="cuda:0").cpu().numpy(), ref["normals"], "pointcloud_normals(knn=)")
    _same_bits(oversegment.pointcloud_normals(xyz, 10, device="cuda:0").cpu().numpy(), ref["normals"], "pointcloud_normals()")
    # final ids: the whole call, and the host chain on the device's edges
    ref_seg = R.merge(ref["edges"], ref["w"], n)
    seg = oversegment.segment_pointcloud(xyz, device="cuda:0")
    assert seg.dtype == np.int32 and np.array_equal(seg, ref_seg)
    assert np.array_equal(oversegment.merge_edges(got_e, got_w, n), ref_seg)
    assert R.digest(seg) == exp["sha256"] and np.unique(seg).shape[0] == exp["segments"]
    for key, val in R.stage_digests(ref, ref_seg).items():
        assert val == exp[key], f"the statement moved away from the committed digest of {key}"


@pytest.mark.parametrize("k", [5, 10, 20])
def test_k(k):
    from seggroup_amd import oversegment
    xyz, ref = _cloud(SWEEP_CASE), _ref(SWEEP_CASE, k)
    got_e, got_w = _check_stages(oversegment.pointcloud_edges(xyz, k, device="cuda:0"), ref, xyz.shape[0], f"k = {k}")
    seg = oversegment.segment_pointcloud(xyz, k, device="cuda:0")
    assert np.array_equal(seg, R.merge(ref["edges"], ref["w"], xyz.shape[0]))
    exp = _expected()[SWEEP_CASE]
    assert R.digest(seg) == (exp["sha256"] if k == 10 else exp["k"][str(k)]["sha256"])


@pytest.mark.parametrize("k_thresh,seg_min_verts", R.PARAM_SWEEP)
def test_parameters_reach_the_chain(k_thresh, seg_min_verts):
    from seggroup_amd import oversegment
    xyz, ref = _cloud(SWEEP_CASE), _ref(SWEEP_CASE)
    seg = oversegment.segment_pointcloud(xyz, 10, k_thresh, seg_min_verts, device="cuda:0")
    assert np.array_equal(seg, R.merge(ref["edges"], ref["w"], xyz.shape[0], k_thresh, seg_min_verts))
    assert R.digest(seg) == _expected()[SWEEP_CASE]["sweep"][f"{k_thresh:g}/{seg_min_verts}"]


def test_a_callers_viewpoint_turns_the_normals():
    from seggroup_amd import oversegment
    xyz, ref, exp = _cloud(SWEEP_CASE), _ref(SWEEP_CASE), _expected()[SWEEP_CASE]["viewpoint"]
    at = tuple(exp["at"])
    want = R.sorted_edges(xyz, 10, viewpoint=at, table=ref["knn"])
    got = oversegment.pointcloud_edges(xyz, viewpoint=at, device="cuda:0")
    _check_stages(got, want, xyz.shape[0], "viewpoint")
    nrm = got["normals"].cpu().numpy()
    flipped = (nrm != ref["normals"]).any(1)
    assert int(flipped.sum()) == exp["flipped"] > 0 and np.array_equal(nrm[flipped], -ref["normals"][flipped])
    _same_bits(oversegment.pointcloud_normals(xyz, viewpoint=at, device="cuda:0").cpu().numpy(), want["normals"], "pointcloud_normals(viewpoint=)")
    seg = oversegment.segment_pointcloud(xyz, viewpoint=at, device="cuda:0")
    assert R.digest(seg) == exp["sha256"]
    # the default is the centre of the bounding box, and passing it changes nothing
    same = oversegment.pointcloud_edges(xyz, viewpoint=R.default_viewpoint(xyz), device="cuda:0")
    _same_bits(same["normals"].cpu().numpy(), ref["normals"], "default viewpoint passed by the caller")


@pytest.mark.parametrize("name", ["room_j0", "room_dup", "room_20k"])
def test_two_runs_give_identical_bytes(name):
    import torch
    from seggroup_amd import oversegment
    xyz = _cloud(name)
    a = oversegment.pointcloud_edges(xyz, device="cuda:0")
    b = oversegment.pointcloud_edges(xyz, device="cuda:0", stream=torch.cuda.Stream(device="cuda:0"))
    for k in ("knn", "normals", "edges", "w"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    s1 = oversegment.segment_pointcloud(xyz, device="cuda:0")
    s2 = oversegment.segment_pointcloud(xyz, device="cuda:0", stream=torch.cuda.Stream(device="cuda:0"))
    assert s1.tobytes() == s2.tobytes()


@pytest.mark.parametrize("name,k", [("room_dup", 10), ("n257", 5), ("all_equal", 20)])
def test_pointcloud_adjacency_is_the_tables_pairs(name, k):
    """sg_pointcloud_adjacency's rows = (i, table[i][t]), t = 1..k, per-row sorted and unique, self pairs kept"""
    from seggroup_amd import prepare
    xyz = _cloud(name)
    table = prepare.pointcloud_knn(xyz, k, device="cuda:0").cpu().numpy()
    assert np.array_equal(table, _ref(name, k)["knn"])
    adj = prepare.get_adj_from_pointcloud(xyz, k, device="cuda:0").numpy()
    assert np.array_equal(adj, R.pairs_of(table, keep_self=True))
    if name != "n257":
        assert (adj[:, 0] == adj[:, 1]).any(), "coincident points give (i, i) rows there"


def test_bad_clouds_are_refused():
    import torch
    from seggroup_amd import hip, oversegment, prepare
    xyz = _cloud("n257")
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[xyz.shape[0] - 1, 2] = bad
        for call in (oversegment.segment_pointcloud, oversegment.pointcloud_edges):
            with pytest.raises(hip.SgError) as ei:
                call(x, device="cuda:0")
            assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    # N <= k: the error of sg_pointcloud_adjacency
    for call in (lambda: oversegment.segment_pointcloud(xyz[:10], device="cuda:0"), lambda: prepare.pointcloud_knn(xyz[:10], 10, device="cuda:0"),
                 lambda: prepare.get_adj_from_pointcloud(xyz[:10], 10, device="cuda:0"), lambda: oversegment.pointcloud_edges(xyz[:20], 20, device="cuda:0")):
        with pytest.raises(hip.SgError) as ei:
            call()
        assert ei.value.code == hip.SG_EINVAL and "points for k =" in str(ei.value)
    for call in (lambda: oversegment.segment_pointcloud(xyz, 7, device="cuda:0"), lambda: prepare.pointcloud_knn(xyz, 7, device="cuda:0")):
        with pytest.raises(hip.SgError) as ei:
            call()
        assert ei.value.code == hip.SG_EUNSUP
    with pytest.raises(ValueError):
        oversegment.segment_pointcloud(xyz[:, :2], device="cuda:0")
    with pytest.raises(ValueError):
        oversegment.pointcloud_edges(xyz, viewpoint=(1.0, 2.0), device="cuda:0")
    with pytest.raises(hip.SgError) as ei:
        oversegment.pointcloud_edges(xyz, viewpoint=(1.0, np.nan, 2.0), device="cuda:0")
    assert ei.value.code == hip.SG_EINVAL and "viewpoint" in str(ei.value)
    # a caller's table is checked on the device: an index that is no point is refused, not read through
    table = prepare.pointcloud_knn(xyz, 10, device="cuda:0")
    for bad in (xyz.shape[0], -1, 2 ** 31 - 1):
        t = table.clone()
        t[xyz.shape[0] - 1, 3] = bad
        with pytest.raises(hip.SgError) as ei:
            oversegment.pointcloud_normals(xyz, 10, knn=t, device="cuda:0")
        assert ei.value.code == hip.SG_EINVAL and "outside 0.." in str(ei.value)
    # the workspace is the caller's: too small a one is refused, not overrun
    lib = hip.lib()
    n = xyz.shape[0]
    d_x = torch.from_numpy(xyz).cuda()
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    nrm, e, w = torch.empty_like(d_x), torch.empty((n * 10, 2), dtype=torch.int32, device="cuda:0"), torch.empty(n * 10, device="cuda:0")
    n_e = C.c_int(0)
    assert lib.sg_pcseg_edges(d_x.data_ptr(), n, 10, None, None, nrm.data_ptr(), e.data_ptr(), w.data_ptr(), C.byref(n_e), ws.data_ptr(), ws.numel(),
                              None) == hip.SG_ENOMEM
    assert b"workspace too small" in lib.sg_last_error()


def _cloud_scan(name="scene0031_00"):
    from seggroup_amd import synthetic
    scan = synthetic.make_raw_scan(64, 48, 21, name=name)
    xyz = scan.xyz.copy()
    xyz[:, 2] *= 6.0                                             # a hillier surface: more than a handful of segments
    return scan, xyz


def test_scan_without_faces_reaches_the_forward(tmp_path, weight_sets):
    """vertices only -> prepare_scene(oversegment=True, label_style=None) -> the reference's tree -> pack -> SegModel.forward: the segs.json is
    the statement's, the adjacency files hold the point graph, the labels equal the oracle's on the same prepared inputs and every label
    vector has V entries.  Without the flag the missing segs.json is an error that names the flag."""
    import torch
    from oracle import cpu_ref
    from seggroup_amd import cache, hip, oversegment, prepare, synthetic
    from seggroup_amd.model import SegModel
    from seggroup_amd.scene import seg_from_lists
    scan, xyz = _cloud_scan()
    root, n = str(tmp_path), 2500
    base = os.path.join(root, "dataset", "scannet")
    sp = os.path.join(base, "scans", scan.name)
    os.makedirs(sp)
    R.write_vertex_only_ply(os.path.join(sp, scan.name + "_vh_clean_2.ply"), xyz, scan.rgb)
    segs = os.path.join(sp, oversegment.segs_json_name(scan.name))
    with pytest.raises(ValueError, match="oversegment=True"):
        prepare.prepare_scene(sp, 0, n, root=base, perm=scan.perm, device="cuda:0")
    assert not os.path.exists(segs)
    prepare.prepare_scene(sp, 0, n, root=base, perm=scan.perm, device="cuda:0", oversegment=True, label_style=None)
    doc = json.load(open(segs))
    ref = R.sorted_edges(xyz, 10)
    want = R.merge(ref["edges"], ref["w"], xyz.shape[0])
    assert doc["sceneId"] == scan.name and doc["params"] == {"kThresh": "0.010000", "segMinVerts": "20"}
    assert np.array_equal(np.asarray(doc["segIndices"], np.int32), want) and np.unique(want).shape[0] >= 5
    # the adjacency files every reader opens: the raw point graph, and its rows through the unmapper
    unmap = torch.load(os.path.join(base, "data", "resampled", scan.name, scan.name + ".unmap.pth")).numpy()
    raw = torch.load(os.path.join(base, "adj", "mesh", "raw", scan.name, scan.name + ".adj.pth")).numpy()
    adj = torch.load(os.path.join(base, "adj", "mesh", "resampled", scan.name, scan.name + ".adj.pth")).numpy()
    want_raw = R.pairs_of(ref["knn"], keep_self=True)
    assert raw.dtype == np.int64 and np.array_equal(raw, want_raw)
    rows = want_raw[want_raw[:, 0] != want_raw[:, 1]]
    assert adj.dtype == np.int64 and np.array_equal(adj, np.unique(np.sort(unmap[rows], axis=1), axis=0))
    # annotation-derived files: a few labelled segments, ground truth per raw vertex
    lists = json.load(open(os.path.join(base, "label", "real", "resampled", scan.name, scan.name + ".seg.json")))
    seg = seg_from_lists(lists, n)
    s = int(seg.max()) + 1
    weak = np.full((n, 2), -1, np.int64)
    for k, g in enumerate(range(0, s, max(s // 9, 1))):
        weak[seg == g] = (k % 5 + 1, k)
    gt = np.stack([np.maximum(weak[unmap, 0], 0) + 1, np.maximum(weak[unmap, 1], 0) + 1], 1).astype(np.int64)
    for sub, arr in ((("label", "seg", "manual", "resampled"), weak), (("label", "real", "raw"), gt)):
        dd = os.path.join(base, *sub, scan.name)
        os.makedirs(dd, exist_ok=True)
        torch.save(torch.from_numpy(arr), os.path.join(dd, scan.name + ".label.pth"))
    ds = cache.load_pack(cache.pack_scene(root, scan.name), device="cuda:0")
    assert (ds.N, ds.S, ds.V) == (n, s, xyz.shape[0])
    sov = ds.seg_of_vertex
    assert sov.shape == (xyz.shape[0],) and (sov >= 0).all() and (sov < s).all(), "every vertex has a segment"
    net = SegModel(exp_name="t", ins_infer=True, data_root=root)
    net.load_weights(weight_sets["ins_infer"])
    net.epoch = "ins_infer"
    res = net.forward_scene(ds, write=False)
    data = torch.load(os.path.join(base, "data", "resampled", scan.name, scan.name + ".pcl.pth")).numpy()
    oracle = cpu_ref.forward_scene(synthetic.Scene(scan.name, data, weak, seg, adj, unmap, gt), weight_sets["ins_infer"], "ins_infer")
    assert res.trace == oracle["trace"]
    for i in range(14):
        assert res.labels[i].shape == (xyz.shape[0],)
        assert np.array_equal(res.labels[i], oracle["labels"][hip.LABEL_NAMES[i]].astype(np.int32)), hip.LABEL_NAMES[i]


def test_command_line_and_the_pointcloud_flag(tmp_path):
    """A scan without faces takes the point-cloud path on its own (child process); the same vertices written as a mesh give the same
    segs.json bytes with pointcloud=True and the mesh path's without; --pointcloud, --knn and --viewpoint reach the segmenter."""
    from seggroup_amd import oversegment, prepare
    scan, xyz = _cloud_scan("scene0032_00")
    clouds, meshes = str(tmp_path / "clouds"), str(tmp_path / "meshes")
    for d in (clouds, meshes):
        os.makedirs(os.path.join(d, scan.name))
    R.write_vertex_only_ply(os.path.join(clouds, scan.name, scan.name + "_vh_clean_2.ply"), xyz, scan.rgb)
    prepare.write_ply(os.path.join(meshes, scan.name, scan.name + "_vh_clean_2.ply"), xyz, scan.rgb, scan.faces)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.oversegment", "--workers", "2", "--scans"]
    r = subprocess.run(cmd + [clouds], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    name = oversegment.segs_json_name(scan.name)
    from_cloud = open(os.path.join(clouds, scan.name, name), "rb").read()
    ref = R.sorted_edges(xyz, 10)
    want = R.merge(ref["edges"], ref["w"], xyz.shape[0])
    assert np.array_equal(np.asarray(json.loads(from_cloud)["segIndices"], np.int32), want)
    # the mesh: its own path without the flag, the cloud's bytes with it
    p = oversegment.oversegment_scan(os.path.join(meshes, scan.name), device="cuda:0")
    assert np.array_equal(np.asarray(prepare.load_seg_labels(p), np.int32), overseg_ref.segment_mesh(xyz, scan.faces))
    assert oversegment.oversegment_scan(os.path.join(meshes, scan.name), device="cuda:0", pointcloud=True) is None, "never overwritten without force"
    p = oversegment.oversegment_scan(os.path.join(meshes, scan.name), device="cuda:0", pointcloud=True, force=True)
    assert open(p, "rb").read() == from_cloud
    # the flags through the command line
    at = (0.4, 0.3, 30.0)
    r = subprocess.run(cmd + [meshes, "--pointcloud", "--knn", "5", "--viewpoint"] + [str(v) for v in at] + ["--force", "--k-thresh", "0.1"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    p = os.path.join(meshes, scan.name, oversegment.segs_json_name(scan.name, 0.1))
    ref5 = R.sorted_edges(xyz, 5, viewpoint=at)
    assert np.array_equal(np.asarray(prepare.load_seg_labels(p), np.int32), R.merge(ref5["edges"], ref5["w"], xyz.shape[0], 0.1))
    assert (ref5["normals"] != R.sorted_edges(xyz, 5, table=ref5["knn"])["normals"]).any(), "the viewpoint of this test turns some normals"


def test_mesh_path_still_equals_its_committed_digests():
    """the sort and gather stages are shared with the mesh segmenter now: its outputs on overseg_ref's room_j5e-4 are what they were"""
    from seggroup_amd import oversegment
    xyz, faces = overseg_ref.case_meshes()["room_j5e-4"]
    exp = json.load(open(os.path.join(GOLDEN, "overseg_expected.json")))["room_j5e-4"]
    ref_n, ref_e, ref_w = overseg_ref.sorted_edges(xyz, faces)
    r = oversegment.device_edges(xyz, faces, device="cuda:0")
    _same_bits(r["normals"].cpu().numpy(), ref_n, "vertex normals")
    assert np.array_equal(r["edges"].cpu().numpy(), ref_e) and r["edges"].shape[0] == exp["edges"]
    _same_bits(r["w"].cpu().numpy(), ref_w, "sorted weights")
    seg = oversegment.segment_mesh(xyz, faces, device="cuda:0")
    assert overseg_ref.digest(seg) == exp["sha256"] and np.unique(seg).shape[0] == exp["segments"]
