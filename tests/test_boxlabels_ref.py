"""Points in boxes and box labels without a GPU: tests/boxlabels_ref.py on hand cases and against exact containment in
fractions, the owner and segment rules of seggroup_amd/boxlabels.py against the restatement's loops on a hand-built scene, box_frames,
and everything the module and its command refuse before a device call."""
import math

import numpy as np
import pytest

import boxlabels_ref as R

STEP = 0.25
# the box [0,2] x [0.5,1.5] x [0,1] on the 0.25 lattice, and the same box described in a frame a quarter turn round (axis 0 along y)
BOX = R.row(1, 1, 0.5, 2, 1, 1)
BOX_TURNED = R.row(1, 1, 0.5, 1, 2, 1, R=R.QUARTER)
ON = np.array([[2, 1, 0.5], [2, 1.5, 0.5], [2, 1.5, 1], [0, 0.5, 0], [1, 1, 0.5]], np.float32)              # face, edge, corner, corner, centre
OFF = np.array([[2.25, 1, 0.5], [2.25, 1.75, 0.5], [2.25, 1.75, 1.25], [-0.25, 0.25, -0.25], [1, 1, 1.25]], np.float32)   # one step further out


def _out(xyz, boxes, margin=0.0):
    count, first, inner, held = R.points_in_boxes(xyz, np.asarray(boxes).reshape(-1, 15), margin)
    return count.tolist(), first.tolist(), inner.tolist(), held.tolist()


def test_hand_cases_are_exact():
    for box in (BOX, BOX_TURNED):
        assert _out(ON, box) == ([1] * 5, [0] * 5, [0] * 5, [5])             # a face, an edge and a corner are inside
        assert _out(OFF, box) == ([0] * 5, [-1] * 5, [-1] * 5, [0])          # one lattice step further out
        assert _out(OFF, box, margin=STEP)[0] == [1] * 5                     # ... and inside again with that step as the margin
        assert _out(OFF, box, margin=STEP / 2)[0] == [0] * 5
    # a sheet holds exactly its plane's points
    sheet = R.row(1, 1, 0.5, 2, 1, 0)
    above = np.nextafter(np.float32(0.5), np.float32(1))
    pts = np.array([[1, 1, 0.5], [2, 1.5, 0.5], [1, 1, above], [1, 1, 0.25], [2.25, 1, 0.5]], np.float32)
    assert _out(pts, sheet)[0] == [1, 1, 0, 0, 0]
    assert _out(np.array([[1, 1, 0.5], [1, 1, above]], np.float32), R.row(1, 1, 0.5, 0, 0, 0))[0] == [1, 0]      # a point box
    # two identical boxes: both hold the point, the lower index is first and inner
    assert _out(ON[:1], [BOX, BOX]) == ([2], [0], [0], [1, 1])
    # a small box inside a large one: first is the lower index, inner the small box whichever comes first
    small = R.row(1, 1, 0.5, 0.5, 0.5, 0.5)
    centre, rim = ON[4:5], ON[:1]
    assert _out(centre, [BOX, small]) == ([2], [0], [1], [1, 1])
    assert _out(centre, [small, BOX]) == ([2], [0], [0], [1, 1])
    assert _out(rim, [BOX, small]) == ([1], [0], [0], [1, 0])
    assert _out(rim, [small, BOX]) == ([1], [1], [1], [0, 1])
    # scenes: only points and boxes of one scene meet, and the indices count within the scene
    both = np.concatenate([centre, centre, rim])
    count, first, inner, held = R.points_in_boxes(both, np.stack([small, BOX, small]), 0.0, [0, 1, 3, 3], [0, 1, 3, 3])
    assert (count.tolist(), first.tolist(), inner.tolist(), held.tolist()) == ([1, 2, 1], [0, 0, 0], [0, 1, 0], [1, 2, 1])
    count, first, inner, _ = R.points_in_boxes(both, np.zeros((0, 15)))
    assert (count.tolist(), first.tolist(), inner.tolist()) == ([0] * 3, [-1] * 3, [-1] * 3)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_restatement_against_exact_containment(seed):
    """every (point, box) whose exact | |l_k| - h_k | exceeds 1e-12 on all axes: the restatement and exact arithmetic agree"""
    xyz, boxes = R.random_scene(seed)
    n, k = xyz.shape[0], boxes.shape[0]
    got, _ = R.inside_matrix(xyz, boxes)
    clear = np.zeros((n, k), bool)
    truth = np.zeros((n, k), bool)
    for j in range(k):
        for i in range(n):
            gaps = R.exact_gaps(xyz[i], boxes[j])
            clear[i, j] = all(abs(g) > 1e-12 for g in gaps)
            truth[i, j] = all(g <= 0 for g in gaps)
    left_out = int((~clear).sum())
    count, first, inner, _ = R.points_in_boxes(xyz, boxes)
    shares = [float((count == 0).mean()), float((count == 1).mean()), float((count > 1).mean())]
    differ = float((first != inner).mean())
    print("seed %d: %d of %d pairs left out, %d differ; shares none / one / several %.2f / %.2f / %.2f, first != inner %.2f"
          % (seed, left_out, n * k, int((got != truth)[clear].sum()), *shares, differ))
    assert left_out * 1000 <= n * k                                          # at most 1 pair in 1,000 is too close to a face to call
    assert np.array_equal(got[clear], truth[clear])
    assert min(shares) >= 0.1 and differ >= 0.05                             # the input is not degenerate


# ---- the owner and the segment rules ----------------------------------------------------------------------------------------------------------
# Two boxes (K = 2; codes 0 = no box, 1 = box 0, 2 = box 1, 3 = several).  Per vertex (count, first, inner):
#   segment 10   5 vertices in box 0 only                                    -> pure: box 0
#   segment 11   9 vertices in box 1 only, 1 in no box                       -> 9 of 10: no box at purity 1.0, box 1 at 0.9 (9 >= 0.9 * 10)
#   segment 12   3 vertices in no box, 1 in box 0                            -> the winner is "no box": none
#   segment 13   4 vertices in both boxes, box 1 the inner one               -> skip: the winner is "several": none;  inner: box 1, pure
#   segment 14   2 vertices in box 0 only, 2 in box 1 only                   -> a tie: none
IN0, IN1, NONE, BOTH = (1, 0, 0), (1, 1, 1), (0, -1, -1), (2, 0, 1)
SCENE = [(10, IN0)] * 5 + [(11, IN1)] * 9 + [(11, NONE)] + [(12, NONE)] * 3 + [(12, IN0)] + [(13, BOTH)] * 4 + [(14, IN0)] * 2 + [(14, IN1)] * 2
SEG = np.array([s for s, _ in SCENE], np.int32)
COUNT, FIRST, INNER = (np.array([v[i] for _, v in SCENE], np.int32) for i in range(3))


def test_owner_and_segment_rule_by_hand():
    from seggroup_amd import boxlabels
    pib = boxlabels.PointsInBoxes(COUNT, FIRST, INNER)
    want = {("skip", 1.0): [0, -1, -1, -1, -1], ("skip", 0.9): [0, 1, -1, -1, -1], ("inner", 1.0): [0, -1, -1, 1, -1], ("inner", 0.9): [0, 1, -1, 1, -1]}
    for (overlap, purity), boxes in want.items():
        owner = boxlabels.vertex_owner(pib, 2, overlap).numpy()
        assert owner.dtype == np.int32 and owner.tolist() == R.vertex_owner(COUNT, FIRST, INNER, 2, overlap)
        assert owner[19:23].tolist() ==([3] * 4 if overlap == "skip" else [2] * 4)
        ids, winner, votes, size, tied = R.vote(SEG, owner)
        assert ids == [10, 11, 12, 13, 14] and size == [5, 10, 4, 4, 4] and tied == [0, 0, 0, 0, 1]
        got = boxlabels.segment_rule(winner, votes, size, tied, 2, purity)
        table = R.segment_boxes(SEG, owner, 2, purity)
        assert got.dtype == np.int32 and got.tolist() == boxes == [table[s][0] for s in ids], (overlap, purity)
        ins, sem = R.weak_labels(SEG, owner, 2, [7, 9], [5, 6], purity)
        assert ins[:5] == [7] * 5 and sem[:5] == [5] * 5 and ins[15:19] == [-1] * 4
    for purity in (0.5, 0.0, 1.0001, -1.0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="purity"):
            boxlabels.segment_rule([1], [1], [1], [0], 2, purity)
        with pytest.raises(ValueError, match="purity"):
            boxlabels.segment_boxes(SEG, COUNT, 2, purity)
    with pytest.raises(ValueError, match="overlap"):
        boxlabels.vertex_owner(pib, 2, "outer")


def _boxes(kind, R3, center, size):
    from seggroup_amd import boxes
    k = center.shape[0]
    z = np.zeros((k, 3))
    return boxes.Boxes(values=np.arange(k, dtype=np.int32), count=np.full(k, 5), first=np.arange(k, dtype=np.int32), lo=z.astype(np.float32),
                       hi=z.astype(np.float32), centroid=z, cov=np.zeros((k, 6)), R=R3, center=center, size=size, yaw=np.zeros(k), kind=kind,
                       angles=0, min_points=1)


def test_box_frames_on_each_input():
    from seggroup_amd import boxset
    c, s = math.cos(0.3), math.sin(0.3)
    center = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
    size = np.array([[2.0, 4.0, 6.0], [1.0, 0.5, 0.25]])
    tilted, _ = np.linalg.qr(np.random.RandomState(3).normal(size=(3, 3)))
    frames = np.array([np.eye(3), tilted])
    for kind in ("aabb", "yaw", "pca"):                                      # a Boxes of any kind: center, size and R as they stand
        rows = boxset.box_frames(_boxes(kind, frames, center, size))
        assert rows.dtype == np.float64 and rows.shape == (2, 15)
        assert rows[:, :3].tolist() == center.tolist() and rows[:, 3:6].tolist() == size.tolist() and rows[:, 6:].tolist() == frames.reshape(2, 9).tolist()
    assert boxset.box_frames(rows) is not rows and boxset.box_frames(rows).tolist() == rows.tolist()     # [K,15]: as they are
    eight = np.concatenate([center, size, [[1.0, 0.0], [c, s]]], 1)
    got = boxset.box_frames(eight)
    assert got[0].tolist() == R.row(1, 2, 3, 2, 4, 6).tolist() and got[1, 6:].tolist() == [c, s, 0, -s, c, 0, 0, 0, 1]
    seven = np.concatenate([center, size, [[5.0], [14.0]]], 1)
    got, cls = boxset.box_frames(seven, classes=True)
    assert got.tolist() == [R.row(1, 2, 3, 2, 4, 6).tolist(), R.row(-4, 0.5, 0, 1, 0.5, 0.25).tolist()] and cls.tolist() == [5, 14]
    assert boxset.box_frames(seven).shape == (2, 15) and boxset.box_frames(eight, classes=True)[1] is None
    assert boxset.box_frames(np.zeros((0, 15))).shape == (0, 15) and boxset.box_frames(np.zeros((0, 7))).shape == (0, 15)
    for bad in (np.zeros((2, 9)), np.zeros(15), np.zeros((2, 15), str), np.concatenate([center, size, [[5.5], [14.0]]], 1)):
        with pytest.raises(ValueError, match="box_frames"):
            boxset.box_frames(bad)


def _write_boxes(path, sem=True, k=2, **more):
    arrays = dict(center=np.zeros((k, 3)), size=np.ones((k, 3)), R=np.tile(np.eye(3), (k, 1, 1)), kind=np.array("pca"), values=np.arange(1, k + 1))
    if sem:
        arrays["sem"] = np.full(k, 5, np.int32)
    arrays.update(more)
    np.savez(path, **arrays)


def test_what_is_refused_before_a_device_call(tmp_path, capsys):
    """on a machine without a GPU a device call is a RuntimeError: every refusal below is a ValueError, an SgError that names the limit, or
    the parser's exit, before it"""
    from seggroup_amd import boxlabels, hip
    xyz = np.zeros((6, 3), np.float32)
    b = np.tile(BOX, (4, 1))
    for args, kw, match in (((xyz[:, :2], b), {}, r"\[N, >= 3\]"), ((xyz.ravel(), b), {}, r"\[N, >= 3\]"), ((xyz, b[:, :9]), {}, "box_frames"),
                            ((xyz, b), dict(margin=-1e-9), "margin"), ((xyz, b), dict(margin=float("nan")), "margin"),
                            ((xyz, b), dict(margin=float("inf")), "margin"), ((xyz, b), dict(margin="1"), "margin"),
                            ((xyz, b), dict(off_points=[0, 6]), "both or neither"), ((xyz, b), dict(off_boxes=[0, 4]), "both or neither"),
                            ((xyz, b), dict(off_points=[0, 4, 3, 6], off_boxes=[0, 1, 2, 4]), "ascend"),
                            ((xyz, b), dict(off_points=[1, 6], off_boxes=[0, 4]), "ascend"), ((xyz, b), dict(off_points=[0, 5], off_boxes=[0, 4]), "ascend"),
                            ((xyz, b), dict(off_points=[0, 6], off_boxes=[0, 5]), "ascend"), ((xyz, b), dict(off_points=[0, 1, 6], off_boxes=[0, 4]), "scenes"),
                            ((xyz, b), dict(off_points=[0.0, 6.0], off_boxes=[0, 4]), "whole"), ((xyz, b), dict(off_points=[[0, 6]], off_boxes=[0, 4]), "whole")):
        with pytest.raises(ValueError, match=match):
            boxlabels.points_in_boxes(*args, **kw)
    many = np.broadcast_to(np.zeros((1, 3), np.float32), ((1 << 24) + 1, 3))
    with pytest.raises(hip.SgError, match="2\\^24") as e:
        boxlabels.points_in_boxes(many, b)
    assert e.value.code == hip.SG_EUNSUP
    with pytest.raises(hip.SgError, match="2\\^16") as e:
        boxlabels.points_in_boxes(xyz, b, off_points=[0] * (1 << 16) + [0, 6], off_boxes=[0] * (1 << 16) + [0, 4])
    assert e.value.code == hip.SG_EUNSUP
    assert hip.lib().sg_points_in_boxes_ws_bytes((1 << 24) + 1, 1, 1) == 0 and hip.lib().sg_points_in_boxes_ws_bytes(1, (1 << 20) + 1, 1) == 0
    assert hip.lib().sg_points_in_boxes_ws_bytes(1, 1, (1 << 16) + 1) == 0 and hip.lib().sg_points_in_boxes_ws_bytes(-1, 1, 1) == 0
    assert hip.lib().sg_points_in_boxes_ws_bytes(1 << 24, 1 << 20, 1 << 16) > 0 and hip.lib().sg_points_in_boxes_ws_bytes(0, 0, 0) > 0
    # weak_labels: ids and sem below 1 (the label files count from 1 and -1 is "no label"), and its other arguments
    seg = np.arange(6)
    for kw, match in ((dict(ids=[1, 2, 0, 4]), "ids"), (dict(sem=[1, 2, 3, -1]), "sem"), (dict(ids=[1, 2, 3]), "ids"), (dict(sem=[1.0, 2, 3, 4]), "sem"),
                      (dict(purity=0.5), "purity"), (dict(purity=1.5), "purity"), (dict(overlap="both"), "overlap"), (dict(margin=-1.0), "margin"),
                      (dict(seg=np.arange(5)), "seg"), (dict(seg=np.arange(6) * 1.0), "seg")):
        args = dict(xyz=xyz, seg=seg, boxes=b, ids=[1, 2, 3, 4], sem=[5, 5, 7, 7])
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            boxlabels.weak_labels(**args)
    # the command
    scans_dir, box_dir = tmp_path / "scans", tmp_path / "boxes"
    box_dir.mkdir()
    for s in ("scene0001_00", "scene0002_00"):
        (scans_dir / s).mkdir(parents=True)
        (scans_dir / s / (s + "_vh_clean_2.ply")).write_bytes(b"ply\n")
    base = ["--scans", str(scans_dir), "--root", str(tmp_path)]
    real = base + ["--from-real"]
    files = base + ["--boxes", str(box_dir)]
    for argv in (base, real + ["--boxes", str(box_dir)], real + ["--kind", "obb"], real + ["--angles", "0"], real + ["--kind", "aabb", "--angles", "9"],
                 real + ["--kind", "pca", "--angles", "9"], real + ["--min-points", "0"], real + ["--suffix", ".boxes.npz"], real + ["--margin", "-0.1"],
                 real + ["--margin", "nan"], real + ["--purity", "0.5"], real + ["--purity", "1.01"], real + ["--overlap", "outer"],
                 real + ["--style-name", "a/b"], real + ["--style-name", ""], real + ["--style-name", ".."], real + ["--workers", "0"],
                 files + ["--kind", "yaw"], files + ["--angles", "90"], files + ["--min-points", "5"], files + ["--suffix", ".npz"]):
        with pytest.raises(SystemExit):
            boxlabels.main(argv)
    capsys.readouterr()
    _write_boxes(str(box_dir / "scene0001_00.boxes.npz"))
    with pytest.raises(SystemExit):
        boxlabels.main(files)
    err = capsys.readouterr().err
    assert "scene0002_00" in err and "both sides" in err                                   # a scan without a box file: named
    _write_boxes(str(box_dir / "scene0002_00.boxes.npz"))
    _write_boxes(str(box_dir / "scene0003_00.boxes.npz"))
    with pytest.raises(SystemExit):
        boxlabels.main(files)
    err = capsys.readouterr().err
    assert "scene0003_00" in err and "both sides" in err                                   # a box file without a scan: named
    (box_dir / "scene0003_00.boxes.npz").unlink()
    _write_boxes(str(box_dir / "scene0002_00.boxes.npz"), sem=False)
    with pytest.raises(SystemExit):
        boxlabels.main(files)
    err = capsys.readouterr().err
    assert "sem" in err and "scene0002_00" in err                                          # a file without a class: named
    _write_boxes(str(box_dir / "scene0002_00.boxes.npz"), sem=False, values=np.array([0, 1]))
    with pytest.raises(SystemExit):
        boxlabels.main(files)
    capsys.readouterr()
    _write_boxes(str(box_dir / "scene0002_00.boxes.npz"), values=np.array([0, 1]))
    with pytest.raises(SystemExit):
        boxlabels.main(files)
    assert ">= 1" in capsys.readouterr().err
    np.save(str(box_dir / "scene0001_00_bbox.npy"), np.zeros((2, 7)) + 1.0)
    np.save(str(box_dir / "scene0002_00_bbox.npy"), np.zeros((2, 6)))
    with pytest.raises(SystemExit):
        boxlabels.main(files + ["--suffix", "_bbox.npy"])
    err = capsys.readouterr().err
    assert "class" in err and "scene0002_00" in err
    assert boxlabels.check_command(True, None, None, None, None, None, None, None, None, None) == dict(
        from_real=True, kind="aabb", angles=0, min_points=1, margin=0.0, purity=1.0, overlap="skip", style_name="box")
    rows, ids, sem = boxlabels.file_boxes(str(box_dir / "scene0001_00_bbox.npy"))
    assert rows.shape == (2, 15) and ids.tolist() == [1, 2] and sem.tolist() == [1, 1]
    rows, ids, sem = boxlabels.file_boxes(str(box_dir / "scene0001_00.boxes.npz"))                # kind pca is taken
    assert rows.shape == (2, 15) and ids.tolist() == [1, 2] and sem.tolist() == [5, 5]


def test_the_kernels_are_in_the_library_and_use_no_scratch(sg_lib):
    """nothing of csrc/kernels_inbox.hip is indexed at run time: the point stays in registers, the boxes in LDS"""
    import os
    import sys
    from conftest import ROOT
    from seggroup_amd import hip
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_report
    if not os.path.exists(os.path.join(scratch_report.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    kernels = scratch_report.kernels_of_library(hip.LIB_PATH)
    for needle in ("k_pb_prepare", "k_pb_test"):
        mine = [(n, b, s) for n, b, _, s in kernels if needle in n]
        assert mine and not any(b or s for _, b, s in mine), (needle, mine)
    assert len([n for n, _, _, _ in kernels if "k_pb_test" in n]) == 2                     # with and without the per-box counts
