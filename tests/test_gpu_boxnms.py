"""Non-maximum suppression on the GPU (seggroup_amd/boxnms.py) against tests/boxnms_ref.py: keep, rep and rank EQUAL to the
restatement -- they are integers --, the refusals, the long way round through sg_box_iou, and the command behind `boxes` and before
`boxap`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boxap_ref as A
import boxes_ref as BR
import boxnms_ref as R
import pcseg_ref as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# k_nm_mask works in tiles of 64 x 64 and k_nm_scan in blocks of 64 ranks, k_nm_rank in workgroups and score tiles of 256: either side of each
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1000)
THRESHOLDS = (0.0, 0.25, 0.5)
BATCH = (5, 0, 17, 64, 0, 130, 1)


def _same(got, want, what=""):
    for name, g, w in zip(("keep", "rep", "rank"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.flatnonzero(g != w)[:8].tolist())


@pytest.mark.parametrize("k", SIZES)
def test_one_scene_equals_the_restatement(k):
    from seggroup_amd import boxnms
    rows, score = R.proposals(k, k)
    cls = (np.arange(k) * 7 % 3).astype(np.int32)
    for t in THRESHOLDS:
        for c in (None, cls):
            want = R.box_nms(rows, score, t, c)
            _same(boxnms.box_nms(rows, score, t, c, device=DEV), want, (k, t, c is not None))
            if k >= 63 and t == 0.25 and c is None:
                cen = R.census(rows, score, t, *want)
                assert cen["kept_through"] > 0 and cen["not_first"] > 0 and cen["tied"] > 0, cen      # what the comparison is about


@pytest.fixture(scope="module")
def long_scene():
    rows, score, layer = R.layered(7, [64] * 64 + [65])
    return rows, score, layer, R.box_nms(rows, score, 0.25)


def test_a_long_scene(long_scene):
    """ONE scene of 4,161 boxes: its bit rows are 66 words, so a lane of the scan holds more than one word of `removed`"""
    from seggroup_amd import boxnms
    rows, score, layer, want = long_scene
    assert rows.shape[0] == 4161 and (rows.shape[0] + 63) // 64 == 66
    rng = np.random.RandomState(1)
    i, j = rng.randint(0, 4161, 4000), rng.randint(0, 4161, 4000)
    cross = layer[i] != layer[j]
    assert cross.sum() > 3000 and not A.pair_iou(rows[i[cross]], rows[j[cross]])[0].any()          # exactly 0 across layers
    got = boxnms.box_nms(rows, score, 0.25, device=DEV)
    _same(got, want)
    assert 1000 < got.keep.sum() < 1400 and (layer[got.rep] == layer).all()
    sizes = boxnms.cluster_sizes(got)
    assert sizes.tolist() == R.cluster_sizes(want[0], want[1]).tolist() and sizes.sum() == 4161 and sizes.max() >= 8


@pytest.mark.parametrize("scenes", (1, 2, 7, 300))
def test_batches(scenes):
    from seggroup_amd import boxnms
    n = list(BATCH[:scenes]) if scenes <= 7 else np.random.RandomState(5).randint(8, 41, scenes).tolist()
    parts = [R.proposals(50 + s, m) for s, m in enumerate(n)]
    rows, score = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    off = np.concatenate([[0], np.cumsum(n)])
    cls = (np.arange(rows.shape[0]) % 3).astype(np.int32)
    for c in (None, cls):
        got = boxnms.box_nms(rows, score, 0.25, c, off, device=DEV)
        _same(got, R.box_nms(rows, score, 0.25, c, off), (scenes, c is not None))
        assert boxnms.cluster_sizes(got, off).tolist() == R.cluster_sizes(got.keep, got.rep, off).tolist()
    assert 0 < got.keep.sum() < rows.shape[0] or scenes == 1


def test_same_bytes_on_a_second_call_and_a_second_stream(long_scene):
    import torch
    from seggroup_amd import boxnms
    rows, score, _, want = long_scene
    rows, score = rows[:1500], score[:1500]
    first = boxnms.box_nms(rows, score, 0.25, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    for stream in (None, side):
        again = boxnms.box_nms(rows, score, 0.25, device=DEV, stream=stream)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first))
    _same(first, R.box_nms(rows, score, 0.25))


def test_permuting_the_input_permutes_the_result():
    from seggroup_amd import boxnms
    k = 300
    rows, _ = R.proposals(k, k)
    rng = np.random.RandomState(k)
    score = rng.permutation(k) / float(k)                                    # DISTINCT scores
    perm = rng.permutation(k)
    a = boxnms.box_nms(rows, score, 0.25, device=DEV)
    b = boxnms.box_nms(rows[perm], score[perm], 0.25, device=DEV)
    assert np.array_equal(b.keep, a.keep[perm]) and np.array_equal(b.rank, a.rank[perm]) and np.array_equal(perm[b.rep], a.rep[perm])
    assert 0 < a.keep.sum() < k


def test_the_long_way_round():
    """sg_box_iou of the scene in rank order, thresholded on the host, and the greedy pass in loops: the same keep -- the matrix entry
    and the mask bit come from the same function"""
    from seggroup_amd import boxap, boxnms
    k = 300
    rows, score = R.proposals(k, k)
    got = boxnms.box_nms(rows, score, 0.25, device=DEV)
    order = np.argsort(got.rank)
    assert order.tolist() == R.order_of(score)
    over = boxap.box_iou(rows[order], rows[order], device=DEV) > 0.25        # entry (i, j) = IoU(a = rank i, b = rank j)
    keep = np.zeros(k, np.int32)
    kept = []
    for r in range(k):
        if not any(over[q, r] for q in kept):
            kept.append(r)
            keep[order[r]] = 1
    assert np.array_equal(keep, got.keep)


def _raw(rows, score, off, thresh=0.25, words=None, k=None, null=None, ws_bytes=None):
    """the library itself, past the module's own checks -> (return code, sg_last_error)"""
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    off = np.ascontiguousarray(off, dtype=np.int32)
    scenes = off.shape[0] - 1
    k = rows.shape[0] if k is None else k
    words = R.words(off) if words is None else words
    d_box = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    d_score = torch.from_numpy(np.ascontiguousarray(score)).to(DEV)
    out = torch.zeros((3, max(rows.shape[0], 1)), dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.sg_box_nms_ws_bytes(rows.shape[0], scenes, R.words([0, rows.shape[0]]))), 1 << 16), dtype=torch.uint8, device=DEV)
    ptrs = dict(box=d_box.data_ptr(), score=d_score.data_ptr(), rank=out[0].data_ptr(), keep=out[1].data_ptr(), rep=out[2].data_ptr(), ws=ws.data_ptr())
    if null:
        ptrs[null] = None
    rc = lib.sg_box_nms(ptrs["box"], ptrs["score"], None, k, off.ctypes.data if null != "off" else None, scenes, thresh, ptrs["rank"], ptrs["keep"],
                        ptrs["rep"], words, ptrs["ws"], ws.numel() if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, lib.sg_last_error().decode()


def test_refusals_leave_the_next_call_right():
    from seggroup_amd import boxnms, hip
    rows, score = R.proposals(21, 21)
    want = R.box_nms(rows, score, 0.25)
    off3 = [0, 5, 5, 21]
    want3 = R.box_nms(rows, score, 0.25, None, off3)

    def valid():
        _same(boxnms.box_nms(rows, score, 0.25, device=DEV), want)
        _same(boxnms.box_nms(rows, score, 0.25, off=off3, device=DEV), want3)

    valid()
    # through the flag word: the module passes these on, and the library names itself
    for column, value, text in ((0, np.nan, "not finite"), (2, np.inf, "not finite"), (5, -np.inf, "not finite"), (7, np.nan, "not finite"),
                                (3, -0.5, "negative size"), (5, -1e-300, "negative size"), (6, 1.1, "unit circle"), (7, 2e-3, "unit circle")):
        bad = rows.copy()
        bad[9, column] = value
        if text == "unit circle" and column == 7:
            bad[9, 6:] = (1.0, 2e-3)                                         # c*c + s*s - 1 = 4e-6
        with pytest.raises(ValueError, match=text) as e:
            boxnms.box_nms(bad, score, 0.25, device=DEV)
        assert "sg_box_nms" in str(e.value)
        valid()
    for value in (np.nan, np.inf, -np.inf):
        bad = score.copy()
        bad[13] = value
        with pytest.raises(ValueError, match="score") as e:
            boxnms.box_nms(rows, bad, 0.25, device=DEV)
        assert "sg_box_nms" in str(e.value) and "not finite" in str(e.value)
        valid()
    near, flat = rows.copy(), rows.copy()
    near[9, 6:] = (1.0, 9e-4)                                                # c*c + s*s - 1 = 8.1e-7: inside the tolerance
    boxnms.box_nms(near, score, 0.25, device=DEV)
    flat[9, 3:6] = 0.0                                                       # a zero size is valid: it overlaps nothing
    got = boxnms.box_nms(flat, score, 0.25, device=DEV)
    assert got.keep[9] == 1 and (got.rep[np.arange(21) != 9] != 9).all()
    # what the module refuses itself goes to the library directly
    for kw, text in ((dict(off=[0, 5, 4, 21]), "ascend"), (dict(off=[0, 20]), "end at"), (dict(off=[0, 22]), "end at"), (dict(off=[1, 21]), "start at 0"),
                     (dict(off=[0, -1, 21]), "ascend"), (dict(thresh=1.0), "threshold"), (dict(thresh=-1e-9), "threshold"), (dict(thresh=float("nan")), "threshold"),
                     (dict(thresh=float("inf")), "threshold"), (dict(words=20), "words"), (dict(words=22), "words"), (dict(off=off3, words=20), "words"),
                     (dict(null="box"), "null"), (dict(null="score"), "null"), (dict(null="rank"), "null"), (dict(null="keep"), "null"),
                     (dict(null="rep"), "null"), (dict(null="ws"), "null"), (dict(null="off"), "null"), (dict(ws_bytes=256), "workspace")):
        kw.setdefault("off", [0, 21])
        rc, msg = _raw(rows, score, **kw)
        assert rc == hip.SG_EINVAL and "sg_box_nms" in msg and text in msg, (kw, msg)
        valid()
    rc, msg = _raw(rows, score, [0, 21])
    assert rc == 0, msg
    rc, msg = _raw(rows[:0], score[:0], [0, 0, 0])                           # no box at all
    assert rc == 0, msg
    empty = boxnms.box_nms(rows[:0], score[:0], 0.25, off=[0, 0, 0], device=DEV)
    assert all(v.shape == (0,) and v.dtype == np.int32 for v in empty)


def test_limits_are_refused_without_a_launch():
    """SG_EUNSUP comes from the host checks, before anything is read on the device: the buffers here are a single box long"""
    from seggroup_amd import boxnms, hip
    rows, score = R.proposals(1, 1)
    big = (1 << 14) + 1
    for kw, text in ((dict(off=[0, big], k=big, words=big * 257), "2^14"), (dict(off=[0, 1, 1 + big], k=1 + big, words=1 + big * 257), "2^14"),
                     (dict(off=[0, (1 << 20) + 1], k=(1 << 20) + 1, words=0), "2^20"), (dict(off=np.zeros((1 << 16) + 2, np.int32), k=0, words=0), "2^16"),
                     (dict(off=np.arange(6) * (1 << 14), k=5 << 14, words=5 << 22), "2^24")):
        rc, msg = _raw(rows, score, **kw)
        assert rc == hip.SG_EUNSUP and "sg_box_nms" in msg and text in msg, msg
        _same(boxnms.box_nms(rows, score, 0.5, device=DEV), R.box_nms(rows, score, 0.5))
    with pytest.raises(hip.SgError, match="2\\^14"):
        boxnms.box_nms(np.broadcast_to(rows, (big, 8)), np.zeros(big), 0.5, device=DEV)


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def _run(module, args, tail):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "seggroup_amd." + module] + args, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and tail in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_command_between_boxes_and_boxap(tmp_path):
    """Four lattice cuboids of 585 points (3 x 2 x 1, step 0.25, axis-aligned, kind aabb, so every box and IoU is exact) with ground
    truth: G1 chair (5), G2 table (7), G3 chair, G4 sofa (6).  The pseudo labels are the ground truth with G1's points SPLIT BY LATTICE
    PARITY into two pseudo instances: P1 (the even lattice sums, 293 points -- all eight corners are even) and P5 (the odd ones, 292
    points, which still reach every face).  Both halves have G1's box: two stacked boxes of IoU 1, scores (`count`) 293 and 292.
    `boxes` writes five boxes in instance order P1 P2 P3 P4 P5 with counts 293 585 585 585 292; the order by score is P2 P3 P4 P1 P5,
    so rank = 3 0 1 2 4; P5 is suppressed by P1 (IoU 1 > 0.5, the same class), nothing else overlaps: keep = 1 1 1 1 0, rep = 0 1 2 3 0,
    the largest cluster 2.  Per class: chair 3 in, 2 kept; sofa 1 and 1; table 1 and 1.
    boxap without scores (every prediction 1.0, one precision-recall point per class), at both thresholds:
      before: chair 3 predictions for 2 boxes, P1 and P3 true, P5 false (P1 took G1): (recall 1, precision 2/3), AP 2/3; table and sofa 1
              mAP = (2/3 + 1 + 1) / 3
      after:  chair 2 predictions, both true: AP 1; mAP = 1 -- the rise is the removed false positive."""
    from seggroup_amd import boxap, boxes, boxnms, pseudo_labels
    scene = "scene0011_00"
    cub = BR.lattice_cuboid()
    even = np.rint(cub / 0.25).astype(np.int64).sum(1) % 2 == 0
    parts = [cub[even], cub + np.float32([6, 0, 0]), cub + np.float32([0, 6, 0]), cub + np.float32([6, 6, 0]), cub[~even]]
    assert [p.shape[0] for p in parts] == [293, 585, 585, 585, 292]
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

    experiment("pseudo", [1, 2, 3, 4, 5], [5, 7, 5, 6, 5])
    experiment("truth", [1, 2, 3, 4, 1], [5, 7, 5, 6, 5])
    pred_dir, gt_dir, kept_dir = os.path.join(root, "pred"), os.path.join(root, "gt"), os.path.join(root, "kept")
    for name, d, n in (("pseudo", pred_dir, 5), ("truth", gt_dir, 4)):
        rep, _ = boxes.boxes_scans(scans_dir, d, workers=1, device=DEV, exp=name, stage="epoch_last", root=root, min_points=1, kind="aabb")
        assert rep[scene]["kept"] == n
    text = _run("boxnms", ["--boxes", pred_dir, "--out", kept_dir, "--iou", "0.5", "--score-key", "count", "--workers", "1"], "1 written, 0 skipped")
    assert scene in text
    with np.load(os.path.join(kept_dir, scene + boxnms.NMS_SUFFIX)) as z:
        assert z["keep"].tolist() == [1, 1, 1, 1, 0] and z["rep"].tolist() == [0, 1, 2, 3, 0] and z["rank"].tolist() == [3, 0, 1, 2, 4]
        assert z["score"].tolist() == [293, 585, 585, 585, 292]
    with np.load(os.path.join(kept_dir, scene + ".boxes.npz")) as z, np.load(os.path.join(pred_dir, scene + ".boxes.npz")) as before:
        assert z["count"].tolist() == [293, 585, 585, 585] and z["values"].tolist() == [1, 2, 3, 4] and z["sem"].tolist() == [5, 7, 5, 6]
        assert np.array_equal(z["center"], before["center"][:4]) and np.array_equal(before["center"][4], before["center"][0]) and str(z["kind"]) == "aabb"
    doc = json.load(open(os.path.join(kept_dir, boxnms.REPORT_NAME)))
    assert doc == {"parameters": {"suffix": ".boxes.npz", "iou": 0.5, "score_key": "count", "class_agnostic": False},
                   "scenes": {scene: {"boxes": 5, "dropped": 0, "kept": 4, "largest_cluster": 2}},
                   "classes": {"5": {"in": 3, "kept": 2}, "6": {"in": 1, "kept": 1}, "7": {"in": 1, "kept": 1}}, "skipped": []}
    maps = {}
    for name, d in (("before", pred_dir), ("after", kept_dir)):
        out = os.path.join(root, "ap_" + name)
        boxap.boxap_scans(scans_dir, out, workers=1, device=DEV, pred=d, gt=gt_dir)
        maps[name] = json.load(open(os.path.join(out, boxap.REPORT_NAME)))["thresholds"]
    one = dict(ap=1.0, recall=1.0, pred=1, gt=1, tp=1)
    for t in ("0.25", "0.5"):
        assert maps["before"][t]["classes"] == {"5": dict(ap=2.0 / 3.0, recall=1.0, pred=3, gt=2, tp=2), "6": one, "7": one}
        assert maps["after"][t]["classes"] == {"5": dict(ap=1.0, recall=1.0, pred=2, gt=2, tp=2), "6": one, "7": one}
        assert maps["before"][t]["map"] == (2.0 / 3.0 + 1.0 + 1.0) / 3 and maps["after"][t]["map"] == 1.0
    # a second run writes nothing without --force
    text = _run("boxnms", ["--boxes", pred_dir, "--out", kept_dir, "--iou", "0.5", "--score-key", "count"], "0 written, 1 skipped")
