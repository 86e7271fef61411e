"""Mesh over-segmentation on the GPU: every device stage -- face normals, ordered vertex normals, edge list, weights,
sorted order -- and the final ids BIT-EQUAL to the NumPy statement of the specification (tests/overseg_ref.py) on every generated case,
a 150k-vertex lattice included; determinism; the refusals of the device check; a scan directory without a segs.json through
prepare_scene(oversegment=True) -> pack -> SegModel.forward; the command line in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import overseg_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CASES = ["room_j0", "room_j5e-4", "room_j2e-3", "raw_scan", "isolated", "one_vertex", "no_edges", "room_150k"]
_meshes = {}


def _mesh(name):
    if not _meshes:
        _meshes.update(R.case_meshes(include_large=True))
    return _meshes[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {np.argwhere(diff)[0].tolist()}: " \
                           f"{got[tuple(np.argwhere(diff)[0])]!r} != {want[tuple(np.argwhere(diff)[0])]!r}"


@pytest.mark.parametrize("name", CASES)
def test_every_stage_is_bit_equal_to_the_reference(name):
    from seggroup_amd import oversegment
    xyz, faces = _mesh(name)
    v = xyz.shape[0]
    exp = json.load(open(os.path.join(GOLDEN, "overseg_expected.json")))[name]
    ref_fn = R.face_normals(xyz, faces)
    ref_n, ref_e, ref_w = R.sorted_edges(xyz, faces)
    r = oversegment.device_edges(xyz, faces, device="cuda:0", want_face_normals=True)
    _same_bits(r["face_normals"].cpu().numpy(), ref_fn, "face normals")
    _same_bits(r["normals"].cpu().numpy(), ref_n, "vertex normals")
    got_e, got_w = r["edges"].cpu().numpy(), r["w"].cpu().numpy()
    assert got_e.dtype == np.int32 and got_e.shape == ref_e.shape and got_e.shape[0] == exp["edges"]
    # the weights as a function of the edge, whatever the order ...
    key = lambda e: e[:, 0].astype(np.int64) * v + e[:, 1]
    assert np.array_equal(np.sort(key(got_e)), np.sort(key(ref_e))), "edge set"
    _same_bits(got_w[np.argsort(key(got_e), kind="stable")], ref_w[np.argsort(key(ref_e), kind="stable")], "weights")
    # ... and the order: ascending (w, a, b), ties and negative weights included
    assert np.array_equal(got_e, ref_e), "sorted order"
    _same_bits(got_w, ref_w, "sorted weights")
    assert int((ref_w < 0).sum()) == exp["negative_weights"]
    # the public functions
    _same_bits(oversegment.vertex_normals(xyz, faces, device="cuda:0").cpu().numpy(), ref_n, "vertex_normals()")
    e2, w2 = oversegment.edge_weights(xyz, faces, device="cuda:0")
    assert np.array_equal(e2.cpu().numpy(), ref_e) and np.array_equal(_bits(w2.cpu().numpy()), _bits(ref_w))
    # final ids: the whole call, and the host chain on the device's edges
    ref_seg = R.merge(ref_e, ref_w, v)
    seg = oversegment.segment_mesh(xyz, faces, device="cuda:0")
    assert seg.dtype == np.int32 and np.array_equal(seg, ref_seg)
    assert np.array_equal(oversegment.merge_edges(got_e, got_w, v), ref_seg)
    assert R.digest(seg) == exp["sha256"] and np.unique(seg).shape[0] == exp["segments"]


@pytest.mark.parametrize("k_thresh,seg_min_verts", R.PARAM_SWEEP)
def test_parameters_reach_the_chain(k_thresh, seg_min_verts):
    from seggroup_amd import oversegment
    xyz, faces = _mesh("room_j5e-4")
    seg = oversegment.segment_mesh(xyz, faces, k_thresh, seg_min_verts, device="cuda:0")
    assert np.array_equal(seg, R.segment_mesh(xyz, faces, k_thresh, seg_min_verts))
    assert R.digest(seg) == json.load(open(os.path.join(GOLDEN, "overseg_expected.json")))["room_j5e-4"]["sweep"][f"{k_thresh:g}/{seg_min_verts}"]


@pytest.mark.parametrize("name", ["room_j0", "raw_scan", "room_150k"])
def test_two_runs_give_identical_bytes(name):
    import torch
    from seggroup_amd import oversegment
    xyz, faces = _mesh(name)
    a = oversegment.device_edges(xyz, faces, device="cuda:0", want_face_normals=True)
    b = oversegment.device_edges(xyz, faces, device="cuda:0", stream=torch.cuda.Stream(device="cuda:0"), want_face_normals=True)
    for k in ("face_normals", "normals", "edges", "w"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    s1 = oversegment.segment_mesh(xyz, faces, device="cuda:0")
    s2 = oversegment.segment_mesh(xyz, faces, device="cuda:0", stream=torch.cuda.Stream(device="cuda:0"))
    assert s1.tobytes() == s2.tobytes()


def test_bad_meshes_are_refused_by_the_device_check():
    from seggroup_amd import hip, oversegment
    xyz, faces = _mesh("raw_scan")
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[xyz.shape[0] - 1, 2] = bad
        with pytest.raises(hip.SgError) as ei:
            oversegment.segment_mesh(x, faces, device="cuda:0")
        assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    for bad in (xyz.shape[0], -1, 2 ** 31 - 1):
        f = faces.copy()
        f[f.shape[0] - 1, 1] = bad
        with pytest.raises(hip.SgError) as ei:
            oversegment.device_edges(xyz, f, device="cuda:0")
        assert ei.value.code == hip.SG_EINVAL and "outside 0.." in str(ei.value)
    with pytest.raises(ValueError):
        oversegment.segment_mesh(xyz[:, :2], faces, device="cuda:0")
    # the workspace is the caller's: too small a one is refused, not overrun
    import ctypes as C
    import torch
    lib = hip.lib()
    d_x, d_f = torch.from_numpy(xyz).cuda(), torch.from_numpy(faces).cuda()
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    nrm, e, w = torch.empty_like(d_x), torch.empty((3 * faces.shape[0], 2), dtype=torch.int32, device="cuda:0"), torch.empty(3 * faces.shape[0], device="cuda:0")
    n_e = C.c_int(0)
    assert lib.sg_overseg_edges(d_x.data_ptr(), xyz.shape[0], d_f.data_ptr(), faces.shape[0], None, nrm.data_ptr(), e.data_ptr(), w.data_ptr(),
                                C.byref(n_e), ws.data_ptr(), ws.numel(), None) == hip.SG_ENOMEM
    assert b"workspace too small" in lib.sg_last_error()


def _write_scan(sp, scan, xyz=None):
    from seggroup_amd import prepare
    os.makedirs(sp)
    prepare.write_ply(os.path.join(sp, scan.name + "_vh_clean_2.ply"), scan.xyz if xyz is None else xyz, scan.rgb, scan.faces)


def test_scan_without_segs_file_reaches_the_forward(tmp_path, weight_sets):
    """mesh only -> prepare_scene(oversegment=True) -> the reference's tree -> pack -> SegModel.forward: the labels equal the oracle's on the
    same prepared inputs and every vertex comes back with a segment.  Without the flag the missing file is the error it always was; an
    existing file is never overwritten."""
    import torch
    from oracle import cpu_ref
    from seggroup_amd import cache, hip, oversegment, prepare, synthetic
    from seggroup_amd.model import SegModel
    from seggroup_amd.scene import seg_from_lists
    scan = synthetic.make_raw_scan(64, 48, 21, name="scene0021_00")
    xyz = scan.xyz.copy()
    xyz[:, 2] *= 6.0                                             # a hillier surface: a few dozen segments instead of three
    root, n = str(tmp_path), 2500
    base = os.path.join(root, "dataset", "scannet")
    sp = os.path.join(base, "scans", scan.name)
    _write_scan(sp, scan, xyz)
    segs = os.path.join(sp, oversegment.segs_json_name(scan.name))
    with pytest.raises(FileNotFoundError):
        prepare.prepare_scene(sp, 0, n, root=base, perm=scan.perm, device="cuda:0")
    assert not os.path.exists(segs)
    prepare.prepare_scene(sp, 0, n, root=base, perm=scan.perm, device="cuda:0", oversegment=True)
    doc = json.load(open(segs))
    want = R.segment_mesh(xyz, scan.faces)
    assert doc["sceneId"] == scan.name and doc["params"] == {"kThresh": "0.010000", "segMinVerts": "20"}
    assert np.array_equal(np.asarray(doc["segIndices"], np.int32), want) and 20 <= np.unique(want).shape[0] <= 40
    # a file that is there is used as it is
    mine = {"segIndices": scan.seg_indices.tolist()}
    other = os.path.join(base, "scans", "scene0022_00")
    scan2 = synthetic.make_raw_scan(64, 48, 21, name="scene0022_00")
    _write_scan(other, scan2)
    json.dump(mine, open(os.path.join(other, oversegment.segs_json_name(scan2.name)), "w"))
    before = open(os.path.join(other, oversegment.segs_json_name(scan2.name)), "rb").read()
    prepare.prepare_scene(other, 1, n, root=base, perm=scan2.perm, device="cuda:0", oversegment=True)
    assert open(os.path.join(other, oversegment.segs_json_name(scan2.name)), "rb").read() == before
    # annotation-derived files: a few labelled segments, ground truth per raw vertex
    lists = json.load(open(os.path.join(base, "label", "real", "resampled", scan.name, scan.name + ".seg.json")))
    seg = seg_from_lists(lists, n)
    s = int(seg.max()) + 1
    assert s == np.unique(want[scan.perm[:n]] if n < xyz.shape[0] else want).shape[0]
    weak = np.full((n, 2), -1, np.int64)
    for k, g in enumerate(range(0, s, max(s // 9, 1))):
        weak[seg == g] = (k % 5 + 1, k)
    unmap = torch.load(os.path.join(base, "data", "resampled", scan.name, scan.name + ".unmap.pth")).numpy()
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
    adj = torch.load(os.path.join(base, "adj", "mesh", "resampled", scan.name, scan.name + ".adj.pth")).numpy()
    ref = cpu_ref.forward_scene(synthetic.Scene(scan.name, data, weak, seg, adj, unmap, gt), weight_sets["ins_infer"], "ins_infer")
    assert res.trace == ref["trace"]
    for i in range(14):
        assert res.labels[i].shape == (xyz.shape[0],)
        assert np.array_equal(res.labels[i], ref["labels"][hip.LABEL_NAMES[i]].astype(np.int32)), hip.LABEL_NAMES[i]


def test_command_line_writes_then_skips(tmp_path):
    from seggroup_amd import oversegment, prepare, synthetic
    scans = str(tmp_path / "scans")
    names = []
    for i, (w, h) in enumerate(((60, 50), (72, 40), (48, 48))):
        s = synthetic.make_room_scan(w, h, 30 + i, jitter=1e-3, name=f"scene{i:04d}_00")
        _write_scan(os.path.join(scans, s.name), s)
        names.append(s.name)
    os.makedirs(os.path.join(scans, "not_a_scan"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.oversegment", "--scans", scans, "--workers", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "3 written, 0 skipped" in r.stdout
    first = {}
    for nm in names:
        p = os.path.join(scans, nm, oversegment.segs_json_name(nm))
        ply = prepare.read_ply(os.path.join(scans, nm, nm + "_vh_clean_2.ply"))
        xyz, _, faces = prepare.mesh_arrays(ply)
        assert np.array_equal(np.asarray(prepare.load_seg_labels(p), np.int32), R.segment_mesh(xyz, faces)), nm
        assert sorted(os.listdir(os.path.join(scans, nm))) == sorted([nm + "_vh_clean_2.ply", os.path.basename(p)])
        first[nm] = (os.stat(p).st_mtime_ns, open(p, "rb").read())
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "0 written, 3 skipped" in r.stdout
    for nm in names:
        p = os.path.join(scans, nm, oversegment.segs_json_name(nm))
        assert (os.stat(p).st_mtime_ns, open(p, "rb").read()) == first[nm]
    # --scenes, other parameters, --force
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write(names[1] + "\n")
    r = subprocess.run(cmd + ["--scenes", lst, "--k-thresh", "0.1", "--seg-min-verts", "5", "--force"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    p = os.path.join(scans, names[1], oversegment.segs_json_name(names[1], 0.1))
    assert p.endswith(".0.100000.segs.json") and json.load(open(p))["params"] == {"kThresh": "0.100000", "segMinVerts": "5"}
