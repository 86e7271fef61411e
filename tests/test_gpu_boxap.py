"""Box IoU and detection AP on the GPU (seggroup_amd/boxap.py) against tests/boxap_ref.py: sg_box_iou EQUAL to the
restatement bit for bit, sg_box_best its index and the matrix entry's bits, the refusals, and the command on both of its routes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boxap_ref as R
import boxes_ref as BR
import pcseg_ref as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# k_bi_pairs runs 256 pairs a workgroup and k_bb_best 4 boxes of A a workgroup and 64 boxes of B a turn: the sizes either side of each
SIZES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 130)
TILE_SHAPES = ((1, 255), (1, 256), (1, 257), (3, 85), (4, 64), (5, 103), (16, 16), (255, 1), (257, 1), (3, 171), (4, 128), (127, 129))
BEST_KB = (0, 1, 63, 64, 65, 129, 1000)


def _set(seed, k):
    """k boxes in a 2 m cube, sizes 0.05 .. 1.55, a quarter of the yaws at multiples of 45 degrees, float32-valued centres; some boxes
    repeat an earlier one and some have a zero size"""
    rng = np.random.RandomState(seed)
    c = (rng.rand(k, 3) * 2.0).astype(np.float32).astype(np.float64)
    s = 0.05 + 1.5 * rng.rand(k, 3)
    s[rng.rand(k) < 0.05, rng.randint(0, 3)] = 0.0
    yaw = np.where(rng.rand(k) < 0.25, rng.randint(0, 8, k) * (np.pi / 4), rng.rand(k) * 2.0 * np.pi)
    rows = np.concatenate([c, s, np.cos(yaw)[:, None], np.sin(yaw)[:, None]], 1)
    for i in np.flatnonzero(rng.rand(k) < 0.1):
        if i:
            rows[i] = rows[rng.randint(0, i)]
    return np.ascontiguousarray(rows)


@pytest.fixture(scope="module")
def sets():
    a, b = _set(1, 130), _set(2, 257)
    b[:40] = a[:40]                                                        # identical pairs on the diagonal
    return a, b, R.box_iou(a, b)[0]                                        # the reference once: every smaller shape is a corner of it


def _equal(got, want):
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), "worst difference %.3e" % (np.abs(got - want).max() if got.size else 0.0)


@pytest.mark.parametrize("ka", SIZES)
def test_iou_equals_the_restatement(sets, ka):
    from seggroup_amd import boxap
    a, b, want = sets
    for kb in SIZES:
        _equal(boxap.box_iou(a[:ka], b[:kb], device=DEV), want[:ka, :kb])


def test_iou_either_side_of_a_workgroup(sets):
    from seggroup_amd import boxap
    a, b, want = sets
    for ka, kb in TILE_SHAPES:
        _equal(boxap.box_iou(a[:ka], b[:kb], device=DEV), want[:ka, :kb])
    v = boxap.box_iou(a, a, device=DEV)
    assert (np.abs(np.diag(v)[a[:, 3:6].min(1) > 0] - 1.0) < 1e-14).all() and (v >= 0).all() and (v <= 1 + 1e-14).all()


@pytest.mark.parametrize("scenes", (1, 2, 7))
def test_iou_in_batches(scenes):
    from seggroup_amd import boxap
    na = [5, 0, 17, 64, 0, 3, 1][:scenes]
    nb = [9, 4, 0, 65, 0, 130, 1][:scenes]                                  # scenes empty on one side, and on both
    a, b = _set(3, sum(na)), _set(4, sum(nb))
    off_a, off_b = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    got = boxap.box_iou(a, b, off_a, off_b, device=DEV)
    want = R.box_iou(a, b, off_a, off_b)
    assert len(got) == scenes
    for g, w, x, y in zip(got, want, na, nb):
        assert g.shape == (x, y)
        _equal(g, w)
    best, top = boxap.box_best(a, b, off_a=off_a, off_b=off_b, device=DEV)
    wbest, wtop = R.box_best(a, b, off_a=off_a, off_b=off_b)
    assert best.dtype == np.int32 and np.array_equal(best, wbest)
    _equal(top, wtop)


@pytest.mark.parametrize("kb", BEST_KB)
def test_best_equals_the_restatement_and_the_matrix(kb):
    from seggroup_amd import boxap
    for ka in (0, 1, 3, 4, 5, 9):
        a, b = _set(10 + ka, ka), _set(20 + kb, kb)
        if ka and kb:
            b[kb // 2] = a[0]                                               # one exact partner
        cls_a, cls_b = np.arange(ka) % 3, (np.arange(kb) * 7) % 3
        matrix = boxap.box_iou(a, b, device=DEV)
        _equal(matrix, R.box_iou(a, b)[0])
        for ca, cb in ((None, None), (cls_a, cls_b)):
            best, top = boxap.box_best(a, b, ca, cb, device=DEV)
            wbest, wtop = R.box_best(a, b, ca, cb)
            assert best.shape == (ka,) and np.array_equal(best, wbest), (ka, kb)
            _equal(top, wtop)
            hit = best >= 0
            _equal(top[hit], matrix[np.flatnonzero(hit), best[hit]])        # the bits of the matrix entry
            assert not top[~hit].any()
            if ca is not None:
                assert (cls_b[best[hit]] == cls_a[hit]).all()


def test_ties_and_rows_without_a_partner():
    from seggroup_amd import boxap
    a = np.stack([R.row(0, 0, 0, 1, 1, 1, 0.3), R.row(50, 0, 0, 1, 1, 1), R.row(0, 0, 0, 0, 0, 0)])
    b = _set(7, 200)
    b[:, 0] += 10.0                                                          # away from a's boxes
    b[150] = b[31] = b[97] = R.row(0.1, 0, 0, 1, 1, 1, 0.3)                  # three identical partners: the lowest index wins
    best, top = boxap.box_best(a, b, device=DEV)
    assert best.tolist() == [31, -1, -1] and top[1] == 0.0 and top[2] == 0.0 and 0.5 < top[0] < 1.0
    m = boxap.box_iou(a, b, device=DEV)
    assert m[0, 31] == m[0, 97] == m[0, 150] == top[0] and not m[1].any() and not m[2].any()
    cls_b = np.zeros(200, np.int32)
    cls_b[31] = 1
    best, _ = boxap.box_best(a, b, np.zeros(3, np.int32), cls_b, device=DEV)
    assert best.tolist() == [97, -1, -1]


def test_same_bytes_on_a_second_call_and_a_second_stream(sets):
    import torch
    from seggroup_amd import boxap
    a, b, want = sets
    first = boxap.box_iou(a, b, device=DEV)
    best = boxap.box_best(a, b, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    for stream in (None, side):
        again = boxap.box_iou(a, b, device=DEV, stream=stream)
        assert again.tobytes() == first.tobytes() == want.tobytes()
        b2 = boxap.box_best(a, b, device=DEV, stream=stream)
        assert b2[0].tobytes() == best[0].tobytes() and b2[1].tobytes() == best[1].tobytes()


def _raw(entry, a, b, off_a, off_b, pairs=None):
    """the library itself, past the module's own checks -> (return code, sg_last_error)"""
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    off_a, off_b = np.asarray(off_a, np.int32), np.asarray(off_b, np.int32)
    scenes = off_a.shape[0] - 1
    d_a, d_b = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ws = torch.empty(max(int(lib.sg_box_iou_ws_bytes(min(a.shape[0], 1 << 20), min(b.shape[0], 1 << 20), scenes)), 1 << 16), dtype=torch.uint8, device=DEV)
    if entry == "iou":
        n = a.shape[0] * b.shape[0] if pairs is None else pairs
        out = torch.empty(max(min(n, 1 << 16), 1), dtype=torch.float64, device=DEV)      # a refused call writes nothing
        rc = lib.sg_box_iou(d_a.data_ptr(), a.shape[0], d_b.data_ptr(), b.shape[0], off_a.ctypes.data, off_b.ctypes.data, scenes, out.data_ptr(), n,
                            ws.data_ptr(), ws.numel(), None)
    else:
        best = torch.empty(max(a.shape[0], 1), dtype=torch.int32, device=DEV)
        top = torch.empty(max(a.shape[0], 1), dtype=torch.float64, device=DEV)
        rc = lib.sg_box_best(d_a.data_ptr(), a.shape[0], d_b.data_ptr(), b.shape[0], None, None, off_a.ctypes.data, off_b.ctypes.data, scenes,
                             best.data_ptr(), top.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, lib.sg_last_error().decode()


def test_refusals_leave_the_next_call_right(sets):
    from seggroup_amd import boxap, hip
    a, b, want = sets
    a, b, want = a[:9].copy(), b[:12].copy(), want[:9, :12]
    wbest, wtop = R.box_best(a, b)

    def valid():
        _equal(boxap.box_iou(a, b, device=DEV), want)
        best, top = boxap.box_best(a, b, device=DEV)
        assert np.array_equal(best, wbest)
        _equal(top, wtop)

    valid()
    for which in ("a", "b"):
        for column, value, text in ((0, np.nan, "not finite"), (2, np.inf, "not finite"), (5, -np.inf, "not finite"), (7, np.nan, "not finite"),
                                    (3, -0.5, "negative size"), (5, -1e-300, "negative size"), (6, 1.1, "unit circle"), (7, 2e-3, "unit circle")):
            bad_a, bad_b = a.copy(), b.copy()
            (bad_a if which == "a" else bad_b)[4, column] = value
            if text == "unit circle" and column == 7:
                (bad_a if which == "a" else bad_b)[4, 6:] = (1.0, 2e-3)      # c*c + s*s - 1 = 4e-6
            for fn, entry in ((boxap.box_iou, "sg_box_iou"), (boxap.box_best, "sg_box_best")):
                with pytest.raises(ValueError, match=text) as e:
                    fn(bad_a, bad_b, device=DEV)
                assert entry in str(e.value) and ("set %s" % which.upper()) in str(e.value)
            valid()
    near = a.copy()
    near[4, 6:] = (1.0, 9e-4)                                                # c*c + s*s - 1 = 8.1e-7: inside the tolerance
    boxap.box_iou(near, b, device=DEV)
    flat = a.copy()
    flat[4, 3:6] = 0.0                                                       # a zero size is valid
    assert not boxap.box_iou(flat, b, device=DEV)[4].any()
    # offsets: the module refuses them itself (tests/test_boxap_ref.py), so the library is called directly
    for entry in ("iou", "best"):
        for off_a, off_b, text in (([0, 5, 4, 9], [0, 4, 8, 12], "ascend"), ([0, 4, 9], [0, 13, 12], "ascend"), ([0, 9], [0, 11], "end at"),
                                   ([0, 10], [0, 12], "end at"), ([1, 9], [0, 12], "start at 0"), ([0, 3, 9], [0, -1, 12], "ascend")):
            rc, msg = _raw(entry, a, b, off_a, off_b, pairs=108)
            assert rc == hip.SG_EINVAL and ("sg_box_" + entry) in msg and text in msg, msg
        valid()
    rc, msg = _raw("iou", a, b, [0, 9], [0, 12], pairs=107)
    assert rc == hip.SG_EINVAL and "pairs" in msg
    valid()


def test_more_than_2_24_pairs():
    """sg_box_iou refuses 4,097 x 4,096; sg_box_best runs the same sets"""
    from seggroup_amd import boxap, hip
    a, b = _set(31, 4097), _set(32, 4096)
    with pytest.raises(hip.SgError, match="2\\^24") as e:
        boxap.box_iou(a, b, device=DEV)
    assert e.value.code == hip.SG_EUNSUP
    rc, msg = _raw("iou", a, b, [0, 4097], [0, 4096])
    assert rc == hip.SG_EUNSUP and "sg_box_iou" in msg and "2^24" in msg
    assert hip.lib().sg_box_iou_ws_bytes((1 << 20) + 1, 1, 1) == 0 and hip.lib().sg_box_best_ws_bytes(1, 1, (1 << 16) + 1) == 0
    assert hip.lib().sg_box_best_ws_bytes(1 << 20, 1 << 20, 1 << 16) > 0
    best, top = boxap.box_best(a, b, device=DEV)
    rows = np.array([0, 1, 2047, 4095, 4096])
    wbest, wtop = R.box_best(a[rows], b)
    assert np.array_equal(best[rows], wbest)
    _equal(top[rows], wtop)
    assert (best >= 0).mean() > 0.9
    _equal(boxap.box_iou(a[:4096], b, device=DEV)[rows[:4]], R.box_iou(a[rows[:4]], b)[0])     # exactly 2^24 pairs are taken


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def _run(module, args, tail):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "seggroup_amd." + module] + args, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and tail in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_command_on_an_experiment_and_on_files(tmp_path):
    """Four lattice cuboids of 585 points (3 x 2 x 1, step 0.25, axis-aligned, so every box and IoU below is exact) with ground truth:
    G1 chair (5), G2 table (7), G3 chair, G4 sofa (6); ground-truth ids 5001, 7002, 5003, 6004, so the scene's ground-truth boxes are
    in the order G1, G3, G4, G2.  The pseudo labels are the ground truth with G1 CUT IN TWO at x = 1.5 (P1: x <= 1.5, 315 points, a box
    1.5 x 2 x 1; P5: x >= 1.75, 270 points, 1.25 x 2 x 1) and G4 given the WRONG CLASS (P4 a table).
      P1 chair: IoU with G1 = 3 / 6 = 0.5 exactly -> true at 0.25, FALSE at 0.5 (strict)
      P2 table: G2 itself, IoU 1 -> true at both
      P3 chair: G3 itself -> true at both
      P4 table: the only table is G2, IoU 0 -> no partner, false at both
      P5 chair: IoU with G1 = 2.5 / 6 -> above 0.25, but P1 took G1 first -> false at both
    chair: 3 predictions, 2 boxes; at 0.25 two true: (recall 1, precision 2/3), AP 2/3; at 0.5 one true: (1/2, 1/3), AP 1/6
    table: 2 predictions, 1 box, one true at both: (1, 1/2), AP 1/2.   sofa: a box and no prediction: AP 0, recall 0.
    mAP at 0.25 = (2/3 + 1/2 + 0) / 3, at 0.5 = (1/6 + 1/2 + 0) / 3."""
    import torch
    from seggroup_amd import boxap, boxes, pseudo_labels
    scene = "scene0011_00"
    cub = BR.lattice_cuboid()
    parts = [cub[cub[:, 0] <= 1.5], cub + np.float32([6, 0, 0]), cub + np.float32([0, 6, 0]), cub + np.float32([6, 6, 0]), cub[cub[:, 0] > 1.5]]
    assert [p.shape[0] for p in parts] == [315, 585, 585, 585, 270]
    xyz = np.concatenate(parts).astype(np.float32)
    sov = np.concatenate([np.full(p.shape[0], k) for k, p in enumerate(parts)]).astype(np.int32)
    perm = np.random.RandomState(4).permutation(xyz.shape[0])
    xyz, sov = np.ascontiguousarray(xyz[perm]), sov[perm]
    root = str(tmp_path)
    scans_dir = os.path.join(root, "scans")
    os.makedirs(os.path.join(scans_dir, scene))
    P.write_vertex_only_ply(os.path.join(scans_dir, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))

    def experiment(name, ins, sem):
        tables = np.zeros((pseudo_labels.INS_NVEC, 5), np.int32)
        tables[12], tables[13] = ins, sem
        d = os.path.join(root, "results", name, scene, "epoch_last")
        os.makedirs(d)
        pseudo_labels.write(d, tables, sov)

    experiment("pseudo", [1, 2, 3, 4, 5], [5, 7, 5, 7, 5])
    experiment("truth", [1, 2, 3, 4, 1], [5, 7, 5, 6, 5])                   # the ground truth as an experiment: `boxes` writes its files
    gt = np.stack([np.array([5, 7, 5, 6, 5])[sov], np.array([1, 2, 3, 4, 1])[sov]], 1).astype(np.int64)
    raw = os.path.join(root, "dataset", "scannet", "label", "real", "raw", scene)
    os.makedirs(raw)
    torch.save(torch.from_numpy(gt), os.path.join(raw, scene + ".label.pth"))

    out = os.path.join(root, "out")
    text = _run("boxap", ["--scans", scans_dir, "--out", out, "-n", "pseudo", "--stage", "epoch_last", "--root", root, "--workers", "1"], "1 matched, 0 skipped")
    assert "chair" in text and "sofa" in text and "average" in text
    best, iou, cls = [0, 3, 1, -1, 0], [0.5, 1.0, 1.0, 0.0, 2.5 / 6.0], [5, 7, 5, 7, 5]
    with np.load(os.path.join(out, scene + boxap.MATCH_SUFFIX)) as z:
        assert z["best"].tolist() == best and z["iou"].tolist() == iou and z["cls"].tolist() == cls and z["gt_cls"].tolist() == [5, 5, 6, 7]
    want = R.evaluate(best, iou, cls, [0] * 5, {5: 2, 6: 1, 7: 1})
    assert want[0.25]["classes"][5] == dict(ap=2.0 / 3.0, recall=1.0, pred=3, gt=2, tp=2)
    assert want[0.5]["classes"][5] == dict(ap=0.5 * (1.0 / 3.0), recall=0.5, pred=3, gt=2, tp=1)
    assert want[0.25]["classes"][7] == want[0.5]["classes"][7] == dict(ap=0.5, recall=1.0, pred=2, gt=1, tp=1)
    assert want[0.25]["classes"][6] == dict(ap=0.0, recall=0.0, pred=0, gt=1, tp=0)
    assert want[0.25]["map"] == (2.0 / 3.0 + 0.0 + 0.5) / 3 and want[0.5]["map"] == (0.5 * (1.0 / 3.0) + 0.0 + 0.5) / 3

    def check(doc):
        assert sorted(doc["thresholds"]) == ["0.25", "0.5"]
        for t in (0.25, 0.5):
            got = doc["thresholds"][repr(t)]
            assert got["map"] == want[t]["map"]
            assert got["classes"] == {str(c): v for c, v in want[t]["classes"].items()}

    doc = json.load(open(os.path.join(out, boxap.REPORT_NAME)))
    check(doc)
    assert doc["parameters"]["kind"] == "yaw" and doc["parameters"]["min_points"] == 100 and doc["parameters"]["classes"] == "scannet18"
    assert doc["scenes"][scene] == {"V": int(xyz.shape[0]), "pred": 5, "gt": 4}
    # the file route over what `boxes` wrote for the same scene: the same table
    pred_dir, gt_dir = os.path.join(root, "pred"), os.path.join(root, "gt")
    for name, d in (("pseudo", pred_dir), ("truth", gt_dir)):                # in this process: one child process is what the test is about
        rep, _ = boxes.boxes_scans(scans_dir, d, workers=1, device=DEV, exp=name, stage="epoch_last", root=root, min_points=1)
        assert rep[scene]["kept"] == (5 if name == "pseudo" else 4)
    out2 = os.path.join(root, "out2")
    boxap.boxap_scans(scans_dir, out2, workers=1, device=DEV, pred=pred_dir, gt=gt_dir)
    doc2 = json.load(open(os.path.join(out2, boxap.REPORT_NAME)))
    check(doc2)
    assert doc2["thresholds"] == doc["thresholds"]
    with np.load(os.path.join(out2, scene + boxap.MATCH_SUFFIX)) as z:
        assert z["iou"].tolist() == iou and z["cls"].tolist() == cls
        assert z["best"].tolist() == [0, 1, 2, -1, 0]                        # the file's boxes are in instance order: G1, G2, G3, G4
