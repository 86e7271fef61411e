"""Labels onto another geometry of the same scene (seggroup_amd/transfer.py): results made on a thinned scan carried to
the raw scan by nearest vertex -- every transferred vector is the source vector gathered by the plain statement's nearest map
(tests/nearest_grid_ref.brute), whatever the index; the files are what `thin --lift` writes, and evaluate reads them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nearest_grid_ref as NG
import pcseg_ref as R
import test_gpu_thin as TT
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_thinned_results_reach_the_raw_scan(tmp_path, weight_sets):
    """thin_scan -> prepare_scene(oversegment=True) -> pack -> SegModel.forward -> .sgl and .npy on the thinned tree; transfer to the raw
    tree WITHOUT the .thin.npz: every vector equals the thinned vector gathered by brute's nearest map, the report holds the distances,
    and evaluate gives equal accumulators from .sgl and .npy"""
    import argparse

    import torch
    from seggroup_amd import cache, evaluate, hip, model, prepare, pseudo_labels, thin, transfer
    from seggroup_amd.scene import seg_from_lists
    name = "scene0051_00"
    raw_scans = str(tmp_path / "raw_scans")
    scan, xyz = TT._source_scan(raw_scans, name)
    root = str(tmp_path / "thinned")
    base = os.path.join(root, "dataset", "scannet")
    scans = os.path.join(base, "scans")
    thin.thin_scan(os.path.join(raw_scans, name), scans, TT.VOXEL, device=DEV)
    sp = os.path.join(scans, name)
    os.remove(os.path.join(sp, name + thin.MAP_SUFFIX))                     # the map was not kept
    thin_xyz = prepare.mesh_arrays(prepare.read_ply(os.path.join(sp, name + "_vh_clean_2.ply")))[0]
    m, n = thin_xyz.shape[0], 1500
    prepare.prepare_scene(sp, 0, n, root=base, perm=np.random.RandomState(4).permutation(m), device=DEV, oversegment=True, label_style=None,
                          index="grid")
    unmap = torch.load(os.path.join(base, "data", "resampled", name, name + ".unmap.pth")).numpy()
    seg = seg_from_lists(json.load(open(os.path.join(base, "label", "real", "resampled", name, name + ".seg.json"))), n)
    s = int(seg.max()) + 1
    weak = np.full((n, 2), -1, np.int64)
    for k, g in enumerate(range(0, s, max(s // 9, 1))):
        weak[seg == g] = (k % 5 + 1, k)
    gt = np.stack([np.maximum(weak[unmap, 0], 0) + 1, np.maximum(weak[unmap, 1], 0) + 1], 1).astype(np.int64)
    for sub, arr in ((("label", "seg", "manual", "resampled"), weak), (("label", "real", "raw"), gt)):
        dd = os.path.join(base, *sub, name)
        os.makedirs(dd, exist_ok=True)
        torch.save(torch.from_numpy(arr), os.path.join(dd, name + ".label.pth"))
    ds = cache.load_pack(cache.pack_scene(root, name), device=DEV)
    assert (ds.N, ds.V) == (n, m)
    net = model.SegModel(exp_name="t", ins_infer=True, data_root=root, out_formats=("sgl", "npy"))
    net.load_weights(weight_sets["ins_infer"])
    net.epoch = "ins_infer"
    net.async_write = False
    res = net.forward_scene(ds, write=True)

    want = NG.brute(xyz, thin_xyz)
    root2 = str(tmp_path / "raw_root")
    out = os.path.join(root2, "results", "t", name, "ins_infer")
    for index in ("brute", "grid"):
        report, missing = transfer.transfer_results(scans, raw_scans, "t", "ins_infer", root2, root=root, index=index, device=DEV)
        assert missing == {} and list(report) == [name]
        with np.load(os.path.join(out, name + transfer.MAP_SUFFIX)) as z:
            assert z["nearest"].dtype == np.int64 and np.array_equal(z["nearest"], want), index
            assert z["d2"].dtype == np.float32 and z["d2"].tobytes() == NG.d2_of(xyz, thin_xyz, want).tobytes(), index
            dist = np.sqrt(z["d2"].astype(np.float64))
        lab = pseudo_labels.load(out)
        assert lab.V == xyz.shape[0] and pseudo_labels.read_header(out)["V"] == xyz.shape[0]
        vec = lab.vectors()
        for i, lname in enumerate(hip.LABEL_NAMES):
            assert np.array_equal(vec[i], res.labels[i][want]), lname
            assert np.array_equal(np.load(os.path.join(out, lname + ".npy")), res.labels[i][want]), lname + ".npy"
        e = report[name]
        assert e == json.load(open(os.path.join(root2, transfer.REPORT_NAME)))["scenes"][name]
        assert (e["source_V"], e["target_V"]) == (m, xyz.shape[0]) and e["max_distance"] == float(dist.max())
        assert e["median_distance"] == float(np.median(dist))
        assert e["farther_than"] == {"0.05": int((dist > 0.05).sum()), "0.1": int((dist > 0.1).sum()), "0.5": int((dist > 0.5).sum())}
        assert 0 < e["max_distance"] < 2 * TT.VOXEL and e["farther_than"]["0.5"] == 0
    dd = os.path.join(root2, "dataset", "scannet", "label", "real", "raw", name)
    os.makedirs(dd)
    torch.save(torch.from_numpy(gt[want]), os.path.join(dd, name + ".label.pth"))
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


def test_source_equal_to_target():
    import torch
    from seggroup_amd import transfer
    clouds = R.case_clouds()
    x = clouds["room_j5e-4"][0]
    for index in ("grid", "brute"):
        nearest, d2 = transfer.nearest_vertex(x, x, index=index, device=DEV)
        assert nearest.dtype == torch.int64 and d2.dtype == torch.float32 and nearest.is_cuda
        assert np.array_equal(nearest.cpu().numpy(), np.arange(x.shape[0])) and not d2.cpu().numpy().any()
    x = clouds["room_dup"][0]
    want = NG.brute(x, x)
    _, first = np.unique(x, axis=0, return_index=True)
    twins = np.setdiff1d(np.arange(x.shape[0]), first)
    assert twins.shape[0] == 200 and (want[twins] < twins).all()
    for index, cell in (("grid", None), ("grid", 0.04), ("brute", None)):
        nearest, d2 = transfer.nearest_vertex(x, x, index=index, cell=cell, device=DEV)
        assert np.array_equal(nearest.cpu().numpy(), want) and not d2.cpu().numpy().any()
    vals = np.arange(x.shape[0] * 2).reshape(-1, 2)
    assert np.array_equal(transfer.transfer(vals, nearest), vals[want])
    assert torch.equal(transfer.transfer(torch.from_numpy(vals).to(DEV), nearest).cpu(), torch.from_numpy(vals[want]))


def test_brute_is_refused_above_its_cap():
    from seggroup_amd import transfer
    src = np.zeros(((1 << 20) + 1, 3), np.float32)
    with pytest.raises(ValueError, match="--index grid"):
        transfer.nearest_vertex(src, src[:8], index="brute", device=DEV)
    nearest, d2 = transfer.nearest_vertex(src, src[:8], index="grid", device=DEV)       # a million coincident points: one cell, index 0
    assert not nearest.cpu().numpy().any() and not d2.cpu().numpy().any()


def test_the_command_line_in_a_child_process(tmp_path):
    """two trees of vertex-only scans; one scene is in both, one only in the source tree, one only in the target tree"""
    from seggroup_amd import pseudo_labels
    rooms = R.case_clouds()
    src_xyz = rooms["room_j5e-4"][0]
    dst_xyz = np.ascontiguousarray(rooms["room_j2e-3"][0][::-1])            # the same room from another sensor, in another order
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for tree, scene, xyz in ((a, "scene0061_00", src_xyz), (b, "scene0061_00", dst_xyz), (a, "scene0062_00", src_xyz[:300]),
                             (b, "scene0063_00", dst_xyz[:300])):
        os.makedirs(os.path.join(tree, scene))
        R.write_vertex_only_ply(os.path.join(tree, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))
    rng = np.random.RandomState(8)
    m, s = src_xyz.shape[0], 23
    tables, sov = rng.randint(-1, 40, (14, s)).astype(np.int32), rng.randint(-1, s, m).astype(np.int32)
    loose = rng.randint(0, 40, m).astype(np.int32)
    for scene in ("scene0061_00", "scene0062_00"):
        src = os.path.join(str(tmp_path), "results", "e", scene, "epoch_last")
        os.makedirs(src)
        pseudo_labels.write(src, tables, sov)
        np.save(os.path.join(src, "final.sem.npy"), loose)
    root2 = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.transfer", "--from-scans", a, "--to-scans", b, "-n", "e", "--stage", "epoch_last", "--out", root2,
           "--root", str(tmp_path), "--workers", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 scenes transferred, 2 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "skipped scene0062_00 (no scan under --to-scans)" in r.stdout and "skipped scene0063_00 (no scan under --from-scans)" in r.stdout
    report = json.load(open(os.path.join(root2, "transfer_report.json")))
    assert list(report["scenes"]) == ["scene0061_00"] and sorted(report["missing"]) == ["scene0062_00", "scene0063_00"] and report["index"] == "grid"
    want = NG.brute(dst_xyz, src_xyz)
    dst = os.path.join(root2, "results", "e", "scene0061_00", "epoch_last")
    lab = pseudo_labels.load(dst)
    assert lab.V == dst_xyz.shape[0] and np.array_equal(lab.tables, tables) and np.array_equal(lab.seg_of_vertex, sov[want])
    assert np.array_equal(np.load(os.path.join(dst, "final.sem.npy")), loose[want])
    with np.load(os.path.join(dst, "scene0061_00.transfer.npz")) as z:
        assert np.array_equal(z["nearest"], want) and z["d2"].tobytes() == NG.d2_of(dst_xyz, src_xyz, want).tobytes()
    assert not os.path.exists(os.path.join(root2, "results", "e", "scene0062_00"))
    r = subprocess.run(cmd + ["--index", "octree"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 2
