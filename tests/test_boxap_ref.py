"""Box IoU and detection AP without a GPU: tests/boxap_ref.py on hand cases and against an exact clipping in fractions,
the scoring rule of seggroup_amd/boxap.py against the restatement's loops on hand-built scenes, box_rows, and everything the module and
its command refuse before a device call."""
import math

import numpy as np
import pytest

import boxap_ref as R

# The restatement against the exact IoU (fractions.Fraction over the doubles the boxes hold) over R.random_pairs(0, 3000), measured on the
# CPU: the worst absolute difference.  |IoU(a,b) - IoU(b,a)| is held to the same gate.  Both boxes moved 1,000 m away: the centres lose
# bits (a unit in the last place of 1,000 is 1.1e-13, against sides from 0.05), so that difference is measured and gated on its own.
# The gates are 16 times the measurements (the rule of 8p.6, 8s.5, 8t.5).
EXACT_MEASURED = 5.9e-15
MOVED_MEASURED = 3.7e-12
EXACT_BOUND = 16 * EXACT_MEASURED
MOVED_BOUND = 16 * MOVED_MEASURED
PAIRS = 3000
FAR = np.array([1000.0, -1000.0, 1000.0, 0, 0, 0, 0, 0])


def _iou(a, b):
    return float(R.pair_iou(a, b)[0][0])


@pytest.fixture(scope="module")
def pairs():
    a, b = R.random_pairs(0, PAIRS)
    truth = [R.exact_iou(a[i], b[i]) for i in range(PAIRS)]
    return a, b, np.array([float(t[0]) for t in truth]), np.array([t[1] for t in truth])


def test_hand_cases_are_exact():
    r = R.row
    assert _iou(r(1, 2, 3, 1, 2, 3), r(1, 2, 3, 1, 2, 3)) == 1.0                          # a box with itself
    assert _iou(r(0, 0, 0, 1, 1, 1), r(1, 0, 0, 1, 1, 1)) == 0.0                          # two boxes sharing a face
    assert _iou(r(0, 0, 0, 1, 1, 1), r(0, 1, 0, 1, 1, 1, math.pi / 2)) == 0.0             # ... one of them a quarter turn round
    assert _iou(r(0, 0, 0, 1, 1, 1), r(0.5, 0, 0, 1, 1, 1)) == 1.0 / 3.0                  # shifted by half a side
    assert _iou(r(0.25, -0.125, 0.5, 1, 1, 1), r(0, 0, 0, 2, 2, 2)) == 0.125              # side 1 inside side 2: va / vb
    assert _iou(r(0, 0, 0, 2, 2, 2), r(0.25, -0.125, 0.5, 1, 1, 1)) == 0.125
    assert _iou(r(0, 0, 0, 0, 0, 0), r(0, 0, 0, 0, 0, 0)) == 0.0                          # two single-point boxes: no union
    assert _iou(r(0, 0, 0, 1, 1, 1), r(0, 0, 2, 1, 1, 1)) == 0.0                          # disjoint in z only
    assert _iou(r(0, 0, 0, 1, 1, 1), r(0, 0, 1, 1, 1, 1)) == 0.0                          # touching in z
    assert _iou(r(0, 0, 0, 0, 1, 1), r(0, 0, 0, 1, 1, 1)) == 0.0                          # a zero size is valid: a sheet has no volume
    # two side-2 cubes, one turned 45 degrees: an octagon of area 8 sqrt(2) - 8, IoU 1 / sqrt(2)
    v, n = R.pair_iou(r(0, 0, 0, 2, 2, 2), r(0, 0, 0, 2, 2, 2, math.pi / 4))
    assert n[0] == 8 and abs(v[0] - 1.0 / math.sqrt(2.0)) <= EXACT_BOUND
    v, n = R.pair_iou(r(0, 0, 0, 2, 2, 2, math.pi / 4), r(0, 0, 0, 2, 2, 2))
    assert n[0] == 8 and abs(v[0] - 1.0 / math.sqrt(2.0)) <= EXACT_BOUND


def test_restatement_against_exact_clipping(pairs):
    a, b, truth, verts = pairs
    got, n = R.pair_iou(a, b)
    worst = float(np.abs(got - truth).max())
    print("restatement - exact: worst %.3e over %d pairs, %d overlapping, polygons of up to %d vertices" % (worst, PAIRS, (truth > 0).sum(), n.max()))
    assert (truth > 0).sum() > PAIRS // 4 and n.max() == 8 and verts.max() >= 7      # the set reaches the octagon
    assert worst <= EXACT_BOUND
    assert np.array_equal(got == 0.0, truth == 0.0) or np.abs(got - truth)[(got == 0.0) != (truth == 0.0)].max() <= EXACT_BOUND
    assert (got >= 0.0).all() and (got <= 1.0 + EXACT_BOUND).all()


def test_symmetry_and_translation(pairs):
    a, b, truth, _ = pairs
    ab, ba = R.pair_iou(a, b)[0], R.pair_iou(b, a)[0]
    sym = float(np.abs(ab - ba).max())
    moved = float(np.abs(R.pair_iou(a + FAR, b + FAR)[0] - ab).max())
    print("IoU(a,b) - IoU(b,a): worst %.3e; both moved 1,000 m: worst %.3e" % (sym, moved))
    assert sym <= EXACT_BOUND
    assert np.abs(ba - truth).max() <= EXACT_BOUND
    assert moved <= MOVED_BOUND


def test_blocks_and_best_of_the_restatement():
    a = np.stack([R.row(0, 0, 0, 1, 1, 1), R.row(5, 0, 0, 1, 1, 1), R.row(0, 0, 0, 2, 2, 2)])
    b = np.stack([R.row(0.5, 0, 0, 1, 1, 1), R.row(0, 0, 0, 1, 1, 1), R.row(0, 0, 0, 1, 1, 1), R.row(9, 9, 9, 1, 1, 1)])
    blocks = R.box_iou(a, b)
    assert len(blocks) == 1 and blocks[0].tolist() == [[1 / 3, 1.0, 1.0, 0.0], [0.0] * 4, [0.125, 0.125, 0.125, 0.0]]
    best, top = R.box_best(a, b)
    assert best.tolist() == [1, -1, 0] and top.tolist() == [1.0, 0.0, 0.125]             # the lower of two equals; nothing at IoU 0
    best, top = R.box_best(a, b, cls_a=[4, 4, 7], cls_b=[4, 5, 5, 7])
    assert best.tolist() == [0, -1, -1] and top.tolist() == [1 / 3, 0.0, 0.0]
    blocks = R.box_iou(a, b, [0, 1, 1, 3], [0, 2, 4, 4])
    assert [x.shape for x in blocks] == [(1, 2), (0, 2), (2, 0)] and blocks[0].tolist() == [[1 / 3, 1.0]]
    best, top = R.box_best(a, b, off_a=[0, 1, 1, 3], off_b=[0, 2, 4, 4])
    assert best.tolist() == [1, -1, -1]


# ---- the scoring rule ---------------------------------------------------------------------------------------------------------------------------
# Two scenes.  Ground truth: scene 0 has chairs (class 5) g0, g1 and a table (7) g2; scene 1 has a chair g0 and a desk (14) g1.
#   p0  scene 0, chair, best g0 at 0.8          -> true positive at 0.25 and at 0.5
#   p1  scene 0, chair, best g0 at 0.6          -> a duplicate on g0: false positive at both
#   p2  scene 0, chair, best g1 at exactly 0.5  -> true at 0.25, FALSE at 0.5 (the comparison is strict)
#   p3  scene 0, table, its best box overall is a chair, so among tables it has no partner (-1, 0.0) -> false at both; g2 is a miss
#   p4  scene 1, chair, best g0 at 0.3          -> true at 0.25, false at 0.5
#   p5  scene 1, sofa (6): a class without ground truth -> false, AP NaN, not in the mean
#   desk: ground truth and no prediction -> AP 0, recall 0, in the mean
# chairs at 0.25: 4 predictions, 3 ground truth, 3 true: one point (recall 1, precision 3/4), AP 3/4; at 0.5: 1 true: (1/3, 1/4), AP 1/12
# mAP over chair, table, desk: 0.25 -> (3/4 + 0 + 0) / 3 = 1/4;  0.5 -> (1/12) / 3 = 1/36
BEST = np.array([0, 0, 1, -1, 0, -1])
IOU = np.array([0.8, 0.6, 0.5, 0.0, 0.3, 0.0])
CLS = np.array([5, 5, 5, 7, 5, 6])
SCENE = np.array([0, 0, 0, 0, 1, 1])
N_GT = {(0, 5): 2, (0, 7): 1, (1, 5): 1, (1, 14): 1}
N_GT_CLASS = {5: 3, 7: 1, 14: 1}


def _same(got, want):
    """the module's report against the restatement's, float for float (NaN where NaN)"""
    assert sorted(got["thresholds"]) == sorted(repr(t) for t in want)
    for t, w in want.items():
        g = got["thresholds"][repr(t)]
        assert g["map"] == w["map"] or (math.isnan(g["map"]) and math.isnan(w["map"]))
        assert sorted(g["classes"]) == sorted(str(c) for c in w["classes"])
        for c, wc in w["classes"].items():
            gc = g["classes"][str(c)]
            for k in ("ap", "recall"):
                assert gc[k] == wc[k] or (math.isnan(gc[k]) and math.isnan(wc[k])), (t, c, k, gc[k], wc[k])
            assert (gc["pred"], gc["gt"], gc["tp"]) == (wc["pred"], wc["gt"], wc["tp"]), (t, c)


def test_scoring_by_hand_without_scores():
    from seggroup_amd import boxap
    m = boxap.match(BEST, IOU, CLS, SCENE, N_GT)
    assert m.tp.tolist() == [[True, False, True, False, True, False], [True, False, False, False, False, False]]
    assert m.tp.tolist() == R.match(BEST, IOU, CLS, SCENE)
    assert m.n_gt == N_GT_CLASS and m.missed == [{5: 0, 7: 1, 14: 1}, {5: 2, 7: 1, 14: 1}]
    got = boxap.evaluate(BEST, IOU, CLS, SCENE, N_GT)
    _same(got, R.evaluate(BEST, IOU, CLS, SCENE, N_GT_CLASS))
    q, h = got["thresholds"]["0.25"], got["thresholds"]["0.5"]
    assert q["classes"]["5"] == {"ap": 0.75, "recall": 1.0, "pred": 4, "gt": 3, "tp": 3}
    assert h["classes"]["5"] == {"ap": (1.0 / 3.0) * 0.25, "recall": 1.0 / 3.0, "pred": 4, "gt": 3, "tp": 1}
    assert q["classes"]["7"] == {"ap": 0.0, "recall": 0.0, "pred": 1, "gt": 1, "tp": 0}
    assert q["classes"]["14"] == {"ap": 0.0, "recall": 0.0, "pred": 0, "gt": 1, "tp": 0}
    assert math.isnan(q["classes"]["6"]["ap"]) and q["classes"]["6"]["pred"] == 1 and q["classes"]["6"]["gt"] == 0
    assert q["map"] == 0.75 / 3 and abs(h["map"] - 1.0 / 36.0) < 1e-17


def test_scoring_by_hand_with_scores():
    """chairs p0 .9, p1 .8, p2 .7, p4 .6 at 0.25: true, false, true, true -> points (1/3, 1), (1/3, 1/2), (2/3, 2/3), (1, 3/4); the
    envelope is 1, 3/4, 3/4, 3/4 and AP = 1/3 + 0 + 1/4 + 1/4 = 5/6.  With p1 above p0 the duplicate comes FIRST and takes g0."""
    from seggroup_amd import boxap
    score = np.array([0.9, 0.8, 0.7, 0.5, 0.6, 0.4])
    got = boxap.evaluate(BEST, IOU, CLS, SCENE, N_GT, score)
    _same(got, R.evaluate(BEST, IOU, CLS, SCENE, N_GT_CLASS, score))
    assert abs(got["thresholds"]["0.25"]["classes"]["5"]["ap"] - 5.0 / 6.0) < 1e-15
    score[1] = 0.95
    m = boxap.match(BEST, IOU, CLS, SCENE, N_GT, score)
    assert m.tp[0].tolist() == [False, True, True, False, True, False] and m.tp[1].tolist() == [False, True, False, False, False, False]
    _same(boxap.evaluate(BEST, IOU, CLS, SCENE, N_GT, score), R.evaluate(BEST, IOU, CLS, SCENE, N_GT_CLASS, score))
    # distinct scores 0.95 (true), 0.9 (false), 0.7, 0.6 (true): (1/3, 1), (1/3, 1/2), (2/3, 2/3), (1, 3/4): 5/6 again
    assert abs(boxap.evaluate(BEST, IOU, CLS, SCENE, N_GT, score)["thresholds"]["0.25"]["classes"]["5"]["ap"] - 5.0 / 6.0) < 1e-15


def test_permuted_predictions_give_the_same_ap():
    """equal scores: who comes first decides WHICH duplicate is the true positive, never how many there are"""
    from seggroup_amd import boxap
    want = boxap.evaluate(BEST, IOU, CLS, SCENE, N_GT)
    for seed in range(6):
        p = np.random.RandomState(seed).permutation(6)
        _same(boxap.evaluate(BEST[p], IOU[p], CLS[p], SCENE[p], N_GT), R.evaluate(BEST[p], IOU[p], CLS[p], SCENE[p], N_GT_CLASS))
        assert boxap.evaluate(BEST[p], IOU[p], CLS[p], SCENE[p], N_GT) == want or _nan_equal(boxap.evaluate(BEST[p], IOU[p], CLS[p], SCENE[p], N_GT), want)
    p = np.array([1, 0, 2, 3, 4, 5])
    assert boxap.match(BEST[p], IOU[p], CLS[p], SCENE[p], N_GT).tp[0].tolist() == [True, False, True, False, True, False]   # the 0.6 one now


def _nan_equal(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_nan_equal(a[k], b[k]) for k in a)
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


def test_average_precision_by_hand():
    from seggroup_amd import boxap
    # true, false, true of 2 boxes: (1/2, 1), (1/2, 1/2), (1, 2/3); envelope 1, 2/3, 2/3 -> 1/2 + 0 + 1/3
    for fn in (boxap.average_precision, R.average_precision):
        ap, rec = fn([True, False, True], [0.9, 0.8, 0.7], 2)
        assert abs(ap - 5.0 / 6.0) < 1e-15 and rec == 1.0
        assert fn([True, False, True], [1.0, 1.0, 1.0], 4) == (0.5 * (2.0 / 3.0), 0.5)      # equal scores: ONE point (1/2, 2/3)
        assert fn([False, True], [0.9, 0.1], 1) == (0.5, 1.0)                                # (0, 0), (1, 1/2)
        assert fn([True, True], [0.2, 0.7], 2) == (1.0, 1.0)
        assert fn([False, False], [0.2, 0.7], 3) == (0.0, 0.0)
        assert fn([], [], 3) == (0.0, 0.0)
        assert all(math.isnan(v) for v in fn([False], [1.0], 0))
    rng = np.random.RandomState(5)
    for _ in range(50):
        k = int(rng.randint(1, 30))
        tp, score = rng.rand(k) < 0.5, np.round(rng.rand(k), 1)                              # many equal scores
        n_gt = int(tp.sum()) + int(rng.randint(0, 4))
        assert boxap.average_precision(tp, score, n_gt) == R.average_precision(tp.tolist(), score.tolist(), n_gt) or n_gt == 0


def _boxes(kind, R3, center, size):
    from seggroup_amd import boxes
    k = center.shape[0]
    z = np.zeros((k, 3))
    return boxes.Boxes(values=np.arange(k, dtype=np.int32), count=np.full(k, 5), first=np.arange(k, dtype=np.int32), lo=z.astype(np.float32),
                       hi=z.astype(np.float32), centroid=z, cov=np.zeros((k, 6)), R=R3, center=center, size=size, yaw=np.zeros(k), kind=kind,
                       angles=0, min_points=1)


def test_box_rows_on_each_kind():
    from seggroup_amd import boxset
    c, s = math.cos(0.3), math.sin(0.3)
    center = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
    size = np.array([[2.0, 4.0, 6.0], [1.0, 0.5, 0.25]])
    rows = boxset.box_rows(_boxes("aabb", np.tile(np.eye(3), (2, 1, 1)), center, size))
    assert rows.dtype == np.float64 and rows.tolist() == [[1, 2, 3, 2, 4, 6, 1, 0], [-4, 0.5, 0, 1, 0.5, 0.25, 1, 0]]
    rows = boxset.box_rows(_boxes("yaw", np.array([np.eye(3), [[c, s, 0], [-s, c, 0], [0, 0, 1]]]), center, size))
    assert rows[1].tolist() == [-4, 0.5, 0, 1, 0.5, 0.25, c, s] and rows[0, 6:].tolist() == [1, 0]     # the bits of R, no cos taken again
    assert boxset.box_rows(_boxes("yaw", np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 3)))).shape == (0, 8)
    with pytest.raises(ValueError, match="not upright"):
        boxset.box_rows(_boxes("pca", np.tile(np.eye(3), (2, 1, 1)), center, size))
    with pytest.raises(ValueError, match="kind"):
        boxset.box_rows(_boxes("obb", np.tile(np.eye(3), (2, 1, 1)), center, size))


def _write_boxes(path, kind="yaw", sem=True, k=2, **more):
    arrays = dict(center=np.zeros((k, 3)), size=np.ones((k, 3)), R=np.tile(np.eye(3), (k, 1, 1)), kind=np.array(kind))
    if sem:
        arrays["sem"] = np.full(k, 5, np.int32)
    arrays.update(more)
    np.savez(path, **arrays)


def test_what_is_refused_before_a_device_call(tmp_path, capsys):
    """on a machine without a GPU a device call is a RuntimeError: every refusal below is a ValueError, an SgError that names the limit, or
    the parser's exit, before it"""
    from seggroup_amd import boxap, hip
    a, b = np.tile(R.row(0, 0, 0, 1, 1, 1), (3, 1)), np.tile(R.row(0, 0, 0, 1, 1, 1), (4, 1))
    for fn in (boxap.box_iou, boxap.box_best):
        for args, kw, match in (((a[:, :7], b), {}, r"\[K,8\]"), ((a, b.ravel()), {}, r"\[K,8\]"), ((a.astype(str), b), {}, r"\[K,8\]"),
                                ((a, b), dict(off_a=[0, 3]), "both or neither"), ((a, b), dict(off_b=[0, 4]), "both or neither"),
                                ((a, b), dict(off_a=[0, 2, 1, 3], off_b=[0, 1, 2, 4]), "ascend"), ((a, b), dict(off_a=[1, 3], off_b=[0, 4]), "ascend"),
                                ((a, b), dict(off_a=[0, 2], off_b=[0, 4]), "ascend"), ((a, b), dict(off_a=[0, 3], off_b=[0, 5]), "ascend"),
                                ((a, b), dict(off_a=[0, 1, 3], off_b=[0, 4]), "scenes"), ((a, b), dict(off_a=[0.0, 3.0], off_b=[0, 4]), "whole"),
                                ((a, b), dict(off_a=[[0, 3]], off_b=[0, 4]), "whole")):
            with pytest.raises(ValueError, match=match):
                fn(*args, **kw)
        with pytest.raises(ValueError, match="not upright"):
            fn(_boxes("pca", np.tile(np.eye(3), (3, 1, 1)), np.zeros((3, 3)), np.ones((3, 3))), b)
    for kw, match in ((dict(cls_a=[1, 2, 3]), "both"), (dict(cls_b=[1, 2, 3, 4]), "both"), (dict(cls_a=[1, 2], cls_b=[1, 2, 3, 4]), "cls_a"),
                      (dict(cls_a=[1, 2, 3], cls_b=[1.5, 2, 3, 4]), "cls_b")):
        with pytest.raises(ValueError, match=match):
            boxap.box_best(a, b, **kw)
    big = np.tile(R.row(0, 0, 0, 1, 1, 1), (4097, 1))
    with pytest.raises(hip.SgError, match="2\\^24") as e:
        boxap.box_iou(big, big[:4096])
    assert e.value.code == hip.SG_EUNSUP
    for kw, match in ((dict(iou=IOU[:5]), "one value per prediction"), (dict(score=np.ones(5)), "score"), (dict(score=np.full(6, np.nan)), "score"),
                      (dict(thresholds=(0.5, 0.5)), "thresholds"), (dict(thresholds=(1.0,)), "thresholds"), (dict(thresholds=()), "thresholds")):
        args = dict(best=BEST, iou=IOU, cls=CLS, scene_of_pred=SCENE, n_gt_per_scene_class=N_GT)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            boxap.match(**args)
    with pytest.raises(ValueError, match="one value per prediction"):
        boxap.average_precision([True], [1.0, 2.0], 1)
    # the command
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    base = ["--scans", str(tmp_path / "scans"), "--out", str(tmp_path / "out")]
    exp = base + ["-n", "e", "--stage", "s"]
    files = base + ["--pred", str(pred), "--gt", str(gt)]
    for argv in (base, exp + ["--pred", str(pred), "--gt", str(gt)], base + ["--pred", str(pred)], base + ["--gt", str(gt)],
                 exp + ["--kind", "pca"], files + ["--kind", "pca"], exp + ["--kind", "obb"], exp + ["--angles", "0"], exp + ["--kind", "aabb", "--angles", "9"],
                 exp + ["--min-points", "0"], exp + ["--classes", "nyu40"], exp + ["--score-key", "score"], exp + ["--workers", "0"],
                 exp + ["--thresholds", "1.5"], exp + ["--thresholds", "0.5", "0.5"], files + ["--kind", "yaw"], files + ["--angles", "90"],
                 files + ["--min-points", "5"], files + ["--stage", "s"], files + ["--layer", "final"], files + ["--label_style", "manual"]):
        with pytest.raises(SystemExit):
            boxap.main(argv)
    capsys.readouterr()
    _write_boxes(str(pred / "scene0001_00.boxes.npz"))
    _write_boxes(str(gt / "scene0001_00.boxes.npz"))
    _write_boxes(str(pred / "scene0002_00.boxes.npz"))
    with pytest.raises(SystemExit):
        boxap.main(files)
    assert "scene0002_00" in capsys.readouterr().err                                       # on one side only: named
    _write_boxes(str(gt / "scene0002_00.boxes.npz"), sem=False)
    with pytest.raises(SystemExit):
        boxap.main(files)
    err = capsys.readouterr().err
    assert "sem" in err and "scene0002_00" in err
    _write_boxes(str(gt / "scene0002_00.boxes.npz"), kind="pca")
    with pytest.raises(SystemExit):
        boxap.main(files)
    assert "not upright" in capsys.readouterr().err
    _write_boxes(str(gt / "scene0002_00.boxes.npz"))
    with pytest.raises(SystemExit):
        boxap.main(files + ["--score-key", "score"])
    assert "score" in capsys.readouterr().err
    _write_boxes(str(pred / "scene0001_00.boxes.npz"), score=np.ones(3))
    _write_boxes(str(pred / "scene0002_00.boxes.npz"), score=np.ones(2))
    with pytest.raises(SystemExit):
        boxap.main(files + ["--score-key", "score"])
    assert "score" in capsys.readouterr().err


def test_the_box_kernels_are_in_the_library_and_use_no_scratch(sg_lib):
    """the clipped polygon lives in named slots, not in an array indexed at run time: no kernel of csrc/kernels_boxiou.hip has scratch"""
    import os
    import sys
    from conftest import ROOT
    from seggroup_amd import hip
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_report
    if not os.path.exists(os.path.join(scratch_report.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    kernels = scratch_report.kernels_of_library(hip.LIB_PATH)
    for needle in ("k_bi_check", "k_bi_pairs", "k_bb_best"):
        mine = [(n, b, s) for n, b, _, s in kernels if needle in n]
        assert mine and not any(b or s for _, b, s in mine), (needle, mine)
