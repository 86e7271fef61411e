"""Voxel thinning on the GPU: sg_cloud_thin BIT-EQUAL to the NumPy statement of the specification (tests/thin_ref.py) on every
case cloud and voxel edge (duplicates, one point 32 times, N = 1, a crafted tie, the scan tile and the sort tile, rows of six floats) and on
a cloud of 1,058,050 points; segment_pointcloud(voxel=) on that cloud against the statement's lifted ids and 8f's purity bound, and the
identity when every point has a voxel to itself; two streams; the refusals; a face-less scan directory through thin_scan ->
prepare_scene -> SegModel.forward -> .sgl -> --lift -> evaluate; both command lines in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pcseg_ref
import thin_ref as T
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
_clouds, _big = {}, {}


def _cloud(name):
    if not _clouds:
        _clouds.update(T.case_clouds())
    return _clouds[name]


def _big_ref():
    """the large cloud, the statement's thinning and its lifted segmentation, computed once and shared"""
    if not _big:
        xyz, plane = T.big_cloud()
        seg, seg_thin, rep, top = T.segment_thinned(xyz, 0.05)
        _big.update(xyz=xyz, plane=plane, seg=seg, rep=rep, top=top)
    return _big


def _expected():
    return json.load(open(os.path.join(GOLDEN, "thin_expected.json")))


def _thin(xyz, h, **kw):
    from seggroup_amd import thin
    rep, top, lo = thin.thin_cloud(xyz, h, device="cuda:0", **kw)
    assert rep.dtype == top.dtype and str(rep.dtype) == "torch.int32" and rep.is_cuda and top.is_cuda
    return rep.cpu().numpy(), top.cpu().numpy(), lo.cpu().numpy()


def _check(xyz, h, what, points=None):
    rep, top, lo = _thin(xyz if points is None else points, h)
    want_rep, want_top, want_lo = T.thin(xyz, h)
    assert rep.shape == want_rep.shape, f"{what}: M = {rep.shape[0]}, the statement has {want_rep.shape[0]}"
    assert np.array_equal(rep, want_rep), f"{what}: rep"
    assert np.array_equal(top, want_top), f"{what}: thin_of_point"
    assert lo.tobytes() == want_lo.tobytes(), f"{what}: lo"
    return rep, top


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_thinning_is_bit_equal_to_the_statement(name):
    xyz, exp = _cloud(name), _expected()["clouds"][name]
    for h in T.VOXELS:
        rep, top = _check(xyz, h, f"{name} at {h}")
        e = exp["%g" % h]
        assert rep.shape[0] == e["M"] and T.array_digest(rep) == e["rep"] and T.array_digest(top) == e["thin_of_point"]


def test_crafted_tie_and_duplicates_go_to_the_lower_index():
    rep, top = _check(T.TIE, 1.0, "tie")
    assert np.array_equal(rep, [1]) and np.array_equal(top, [0, 0, 0])
    rep, _ = _check(T.TIE[[0, 2, 1]], 1.0, "tie, swapped")
    assert np.array_equal(rep, [1])
    xyz = _cloud("room_dup")
    rep, top = _check(xyz, 0.02, "room_dup")
    _, first = np.unique(xyz, axis=0, return_index=True)
    assert np.array_equal(rep, np.sort(first)), "of two coincident points the first one stands for the voxel"


@pytest.mark.parametrize("name", ["room_j5e-4", "room_20k[:4097]"])
def test_rows_of_six_floats(name):
    xyz = _cloud(name)
    rows = np.concatenate([xyz, np.random.RandomState(2).uniform(-9, 9, xyz.shape).astype(np.float32)], 1)
    for h in T.VOXELS:
        _check(xyz, h, f"{name}, stride 6, at {h}", points=rows)


def test_the_large_cloud():
    b, exp = _big_ref(), _expected()["big"]
    assert b["xyz"].shape[0] == 1058050 > 1 << 20
    rep, top, _ = _thin(b["xyz"], 0.05)
    assert rep.shape[0] == 5403 == exp["M"] and int(np.bincount(top).max()) == 350 == exp["largest_voxel"]
    assert np.array_equal(rep, b["rep"]) and np.array_equal(top, b["top"])
    assert T.array_digest(rep) == exp["rep"] and T.array_digest(top) == exp["thin_of_point"]


def test_segment_pointcloud_through_the_grid():
    from seggroup_amd import hip, oversegment
    b = _big_ref()
    seg = oversegment.segment_pointcloud(b["xyz"], voxel=0.05, device="cuda:0")
    assert seg.dtype == np.int32 and seg.shape == (b["xyz"].shape[0],)
    assert np.array_equal(seg, b["seg"]), "the statement's lifted ids"
    purity = pcseg_ref.purity(seg, b["plane"])
    print("1,058,050 points at 0.05: purity %.4f, %d segments" % (purity, np.unique(seg).shape[0]))
    assert purity >= 0.95
    assert T.array_digest(seg) == _expected()["big"]["quality"]["sha256"]
    with pytest.raises(hip.SgError) as ei:
        oversegment.segment_pointcloud(b["xyz"], device="cuda:0")
    assert ei.value.code == hip.SG_EUNSUP


def test_identity_thinning_changes_nothing():
    from seggroup_amd import oversegment
    xyz = _cloud("room_j5e-4")
    rep, top = _check(xyz, 0.02, "room_j5e-4")
    assert np.array_equal(rep, np.arange(xyz.shape[0])) and np.array_equal(top, rep)
    plain = oversegment.segment_pointcloud(xyz, device="cuda:0")
    assert np.array_equal(oversegment.segment_pointcloud(xyz, voxel=0.02, device="cuda:0"), plain)
    assert pcseg_ref.digest(plain) == json.load(open(os.path.join(GOLDEN, "pcseg_expected.json")))["room_j5e-4"]["sha256"]


@pytest.mark.parametrize("name,h", [("room_dup", 0.05), ("room_20k", 0.075)])
def test_two_streams_give_identical_bytes(name, h):
    import torch
    xyz = _cloud(name)
    a = _thin(xyz, h, stream=torch.cuda.Stream(device="cuda:0"))
    b = _thin(xyz, h, stream=torch.cuda.Stream(device="cuda:0"))
    c = _thin(xyz, h)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_refusals():
    from seggroup_amd import hip, thin
    xyz = _cloud("n257")
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[xyz.shape[0] - 1, 2] = bad
        with pytest.raises(hip.SgError) as ei:
            thin.thin_cloud(x, 0.05, device="cuda:0")
        assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    for h in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(hip.SgError) as ei:
            thin.thin_cloud(xyz, h, device="cuda:0")
        assert ei.value.code == hip.SG_EINVAL and "voxel" in str(ei.value)
    with pytest.raises(hip.SgError) as ei:
        thin.thin_cloud(_cloud("line"), 1e-6, device="cuda:0")
    assert ei.value.code == hip.SG_EUNSUP and "voxel too small for the cloud's extent" in str(ei.value)
    _check(_cloud("room_j0"), 1e-6, "a room at 1e-6 stays inside 2^21 cells")
    with pytest.raises(ValueError):
        thin.thin_cloud(xyz[:, :2], 0.05, device="cuda:0")
    # M <= k is the segmenter's own error
    from seggroup_amd import oversegment
    with pytest.raises(hip.SgError) as ei:
        oversegment.segment_pointcloud(_cloud("all_equal"), voxel=0.05, device="cuda:0")
    assert ei.value.code == hip.SG_EINVAL and "points for k =" in str(ei.value)


# ---- scan directories ---------------------------------------------------------------------------------------------------------------
VOXEL = 0.1
AGG = b'{"sceneId": "x", "segGroups": [ {"id": 0, "label": "floor", "segments": [3, 10]} ]}\n'


def _source_scan(scans_dir, name):
    """a face-less scan directory with a segs.json (an extra field in it) and an aggregation file -> (scan, xyz)"""
    from seggroup_amd import oversegment, synthetic
    scan = synthetic.make_raw_scan(96, 64, 21, name=name)
    xyz = scan.xyz.copy()
    xyz[:, 2] *= 6.0
    sp = os.path.join(scans_dir, name)
    os.makedirs(sp)
    pcseg_ref.write_vertex_only_ply(os.path.join(sp, name + "_vh_clean_2.ply"), xyz, scan.rgb)
    doc = {"params": {"kThresh": "0.010000", "segMinVerts": "20"}, "sceneId": name, "segIndices": scan.seg_indices.tolist(), "tool": "by hand"}
    with open(os.path.join(sp, oversegment.segs_json_name(name)), "w") as f:
        json.dump(doc, f)
    with open(os.path.join(sp, name + ".aggregation.json"), "wb") as f:
        f.write(AGG)
    return scan, xyz


def _check_thinned_scan(dst, scan, xyz, entry):
    from seggroup_amd import oversegment, prepare
    name = scan.name
    rep, top, lo = T.thin(xyz, VOXEL)
    m = rep.shape[0]
    assert 200 < m < xyz.shape[0] // 2
    want_ply = os.path.join(dst, "want.ply")
    prepare.write_ply(want_ply, xyz[rep], scan.rgb[rep], np.zeros((0, 3), np.int32))
    assert open(os.path.join(dst, name + "_vh_clean_2.ply"), "rb").read() == open(want_ply, "rb").read()
    os.remove(want_ply)
    got_xyz, got_rgb, got_faces = prepare.mesh_arrays(prepare.read_ply(os.path.join(dst, name + "_vh_clean_2.ply")))
    assert got_xyz.tobytes() == xyz[rep].tobytes() and np.array_equal(got_rgb, scan.rgb[rep]) and got_faces.shape == (0, 3)
    with np.load(os.path.join(dst, name + ".thin.npz")) as z:
        assert np.array_equal(z["rep"], rep) and np.array_equal(z["thin_of_point"], top) and z["rep"].dtype == np.int32
        assert z["voxel"] == np.float32(VOXEL) and z["lo"].tobytes() == lo.tobytes()
    doc = json.load(open(os.path.join(dst, oversegment.segs_json_name(name))))
    assert doc["segIndices"] == scan.seg_indices[rep].tolist() and doc["tool"] == "by hand" and doc["sceneId"] == name
    assert doc["params"] == {"kThresh": "0.010000", "segMinVerts": "20"}
    assert open(os.path.join(dst, name + ".aggregation.json"), "rb").read() == AGG
    cells, largest = T.stats(xyz, VOXEL, rep, top)
    before, after = np.unique(scan.seg_indices), np.unique(scan.seg_indices[rep])
    assert entry == {"V": xyz.shape[0], "M": m, "voxel": float(np.float32(VOXEL)), "cells": cells, "largest_voxel": largest,
                     "source_segments": before.shape[0], "kept_segments": after.shape[0], "lost_segments": np.setdiff1d(before, after).tolist()}
    return rep, top


def test_thinned_scan_reaches_the_forward_and_lifts_back(tmp_path, weight_sets):
    """thin_scan -> prepare_scene(oversegment=True) on the thinned tree -> pack -> SegModel.forward -> .sgl and .npy -> --lift: every lifted
    vector is the thinned vector gathered by thin_of_point, and evaluate reads the lifted files against the raw scan's ground truth"""
    import argparse

    import torch
    from seggroup_amd import cache, evaluate, hip, model, oversegment, prepare, pseudo_labels, thin
    from seggroup_amd.scene import seg_from_lists
    name = "scene0041_00"
    scan, xyz = _source_scan(str(tmp_path / "raw_scans"), name)
    root = str(tmp_path / "thinned")
    base = os.path.join(root, "dataset", "scannet")
    scans = os.path.join(base, "scans")
    entry = thin.thin_scan(os.path.join(str(tmp_path / "raw_scans"), name), scans, VOXEL, device="cuda:0")
    sp = os.path.join(scans, name)
    rep, top = _check_thinned_scan(sp, scan, xyz, entry)
    assert thin.thin_scan(os.path.join(str(tmp_path / "raw_scans"), name), scans, VOXEL, device="cuda:0") is None, "never overwritten without force"
    m, n = rep.shape[0], 1500
    segs_before = open(os.path.join(sp, oversegment.segs_json_name(name)), "rb").read()
    prepare.prepare_scene(sp, 0, n, root=base, perm=np.random.RandomState(4).permutation(m), device="cuda:0", oversegment=True, label_style=None)
    assert open(os.path.join(sp, oversegment.segs_json_name(name)), "rb").read() == segs_before, "the thinned segs.json is the scan's own"
    unmap = torch.load(os.path.join(base, "data", "resampled", name, name + ".unmap.pth")).numpy()
    lists = json.load(open(os.path.join(base, "label", "real", "resampled", name, name + ".seg.json")))
    seg = seg_from_lists(lists, n)
    s = int(seg.max()) + 1
    weak = np.full((n, 2), -1, np.int64)
    for k, g in enumerate(range(0, s, max(s // 9, 1))):
        weak[seg == g] = (k % 5 + 1, k)
    gt = np.stack([np.maximum(weak[unmap, 0], 0) + 1, np.maximum(weak[unmap, 1], 0) + 1], 1).astype(np.int64)
    assert gt.shape[0] == m
    for sub, arr in ((("label", "seg", "manual", "resampled"), weak), (("label", "real", "raw"), gt)):
        dd = os.path.join(base, *sub, name)
        os.makedirs(dd, exist_ok=True)
        torch.save(torch.from_numpy(arr), os.path.join(dd, name + ".label.pth"))
    ds = cache.load_pack(cache.pack_scene(root, name), device="cuda:0")
    assert (ds.N, ds.V) == (n, m)
    net = model.SegModel(exp_name="t", ins_infer=True, data_root=root, out_formats=("sgl", "npy"))
    net.load_weights(weight_sets["ins_infer"])
    net.epoch = "ins_infer"
    net.async_write = False
    res = net.forward_scene(ds, write=True)
    # lift into a second root that holds the RAW scan's ground truth
    root2 = str(tmp_path / "raw_root")
    assert thin.main(["--lift", "-n", "t", "--stage", "ins_infer", "--maps", scans, "--out", root2, "--root", root]) == 0
    out = os.path.join(root2, "results", "t", name, "ins_infer")
    lab = pseudo_labels.load(out)
    assert lab.V == xyz.shape[0] and pseudo_labels.read_header(out)["V"] == xyz.shape[0]
    vec = lab.vectors()
    for i, lname in enumerate(hip.LABEL_NAMES):
        assert res.labels[i].shape == (m,)
        assert np.array_equal(vec[i], res.labels[i][top]), lname
        assert np.array_equal(np.load(os.path.join(out, lname + ".npy")), res.labels[i][top]), lname + ".npy"
    dd = os.path.join(root2, "dataset", "scannet", "label", "real", "raw", name)
    os.makedirs(dd)
    torch.save(torch.from_numpy(gt[top]), os.path.join(dd, name + ".label.pth"))
    with open(os.path.join(root2, "scenes.txt"), "w") as f:
        f.write(name + "\n")
    accs = {}
    for fmt in ("sgl", "npy"):
        a = argparse.Namespace(exp_name="t", layer="all", stage="ins_infer", root=root2, scenes=os.path.join(root2, "scenes.txt"), format=fmt,
                               json=None, label_style="manual", batch=64, workers=1, ap=False)
        accs[fmt] = evaluate.run(a)
    assert sorted(accs["sgl"]) == sorted(accs["npy"]) and "final" in accs["sgl"]
    for l in accs["sgl"]:
        assert int(accs["sgl"][l].v[164]) == 1 and np.array_equal(accs["sgl"][l].v, accs["npy"][l].v), l


def test_both_command_lines(tmp_path):
    from seggroup_amd import pseudo_labels
    name = "scene0042_00"
    raw = str(tmp_path / "raw_scans")
    scan, xyz = _source_scan(raw, name)
    out = str(tmp_path / "thinned_scans")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.thin"]
    r = subprocess.run(cmd + ["--scans", raw, "--out", out, "--voxel", str(VOXEL), "--workers", "2"], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    report = json.load(open(os.path.join(out, "thin_report.json")))
    assert report["voxel"] == float(np.float32(VOXEL)) and list(report["scenes"]) == [name] and report["skipped"] == []
    rep, top = _check_thinned_scan(os.path.join(out, name), scan, xyz, report["scenes"][name])
    # results made on the thinned scan: a compact file and one loose vector
    rng = np.random.RandomState(8)
    m, s = rep.shape[0], 23
    tables, sov = rng.randint(-1, 40, (14, s)).astype(np.int32), rng.randint(-1, s, m).astype(np.int32)
    src = os.path.join(str(tmp_path), "results", "e", name, "epoch_last")
    os.makedirs(src)
    pseudo_labels.write(src, tables, sov)
    loose = rng.randint(0, 40, m).astype(np.int32)
    np.save(os.path.join(src, "final.sem.npy"), loose)
    root2 = str(tmp_path / "raw_root")
    r = subprocess.run(cmd + ["--lift", "-n", "e", "--stage", "epoch_last", "--maps", out, "--out", root2, "--root", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 scenes lifted" in r.stdout, (r.stdout + r.stderr)[-3000:]
    dst = os.path.join(root2, "results", "e", name, "epoch_last")
    lab = pseudo_labels.load(dst)
    assert lab.V == xyz.shape[0] and np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[top])
    assert np.array_equal(np.load(os.path.join(dst, "final.sem.npy")), loose[top])


def test_oversegment_command_line_takes_the_grid(tmp_path):
    """--voxel reaches the segmenter: the segs.json of a face-less scan holds the statement's lifted ids"""
    from seggroup_amd import oversegment, prepare
    name = "scene0043_00"
    xyz = _cloud("room_20k")
    sp = tmp_path / name
    os.makedirs(sp)
    pcseg_ref.write_vertex_only_ply(str(sp / (name + "_vh_clean_2.ply")), xyz, np.zeros(xyz.shape, np.uint8))
    assert oversegment.main(["--scans", str(tmp_path), "--voxel", "0.05", "--workers", "1", "--device", "cuda:0"]) == 0
    got = np.asarray(prepare.load_seg_labels(str(sp / oversegment.segs_json_name(name))), np.int32)
    assert T.array_digest(got) == _expected()["room_20k_quality"]["sha256"]
