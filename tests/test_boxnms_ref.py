"""Non-maximum suppression without a GPU: tests/boxnms_ref.py on hand cases that are exact, its properties on the
proposal generator, everything seggroup_amd/boxnms.py and its command refuse before a device call, the command's file cutting on
hand-written files of both kinds, and the kernels in the built library."""
import os

import numpy as np
import pytest

import boxap_ref as A
import boxnms_ref as R

SIZES = (16, 63, 64, 65, 129, 300, 1000)
THIRD = 1.0 / 3.0
CUBES = np.stack([A.row(0.0, 0, 0, 1, 1, 1), A.row(0.5, 0, 0, 1, 1, 1), A.row(1.0, 0, 0, 1, 1, 1)])       # IoU 1/3, 1/3 and 0 (a shared face)


def _nms(rows, score, thresh, cls=None, off=None):
    keep, rep, rank = R.box_nms(rows, score, thresh, cls, off)
    return keep.tolist(), rep.tolist(), rank.tolist()


def test_hand_cases_are_exact():
    iou = R.ordered_iou(CUBES)
    assert iou[0, 1] == THIRD and iou[1, 2] == THIRD and iou[0, 2] == 0.0
    # scores descending: the middle one goes to the first, and the third -- which only the SUPPRESSED middle one overlaps -- is KEPT
    assert _nms(CUBES, [0.9, 0.8, 0.7], 0.25) == ([1, 0, 1], [0, 0, 2], [0, 1, 2])
    # the middle one scoring highest takes both
    assert _nms(CUBES, [0.8, 0.9, 0.7], 0.25) == ([0, 1, 0], [1, 1, 1], [1, 0, 2])
    # the threshold exactly at the IoU: the comparison is strict
    assert _nms(CUBES, [0.9, 0.8, 0.7], THIRD) == ([1, 1, 1], [0, 1, 2], [0, 1, 2])
    assert _nms(CUBES, [0.9, 0.8, 0.7], np.nextafter(THIRD, 0.0)) == ([1, 0, 1], [0, 0, 2], [0, 1, 2])
    # equal scores: the lower index wins
    twins = np.stack([CUBES[1], CUBES[0], CUBES[0]])
    assert _nms(twins, [0.5, 0.5, 0.5], 0.5) == ([1, 1, 0], [0, 1, 1], [0, 1, 2])
    assert _nms(twins, [0.5, 0.7, 0.7], 0.5) == ([1, 1, 0], [0, 1, 1], [2, 0, 1])
    # -0.0 against 0.0 is a tie: the lower index wins whichever zero it holds
    assert _nms(twins[1:], [-0.0, 0.0], 0.5) == ([1, 0], [0, 0], [0, 1])
    assert _nms(twins[1:], [0.0, -0.0], 0.5) == ([1, 0], [0, 0], [0, 1])
    # classes: a duplicate of another class survives, and is suppressed without classes
    assert _nms(twins[1:], [0.9, 0.8], 0.5, cls=[5, 7]) == ([1, 1], [0, 1], [0, 1])
    assert _nms(twins[1:], [0.9, 0.8], 0.5, cls=[5, 5]) == ([1, 0], [0, 0], [0, 1])
    assert _nms(twins[1:], [0.9, 0.8], 0.5) == ([1, 0], [0, 0], [0, 1])
    # two scenes that would suppress each other if they met; indices count within the scene
    assert _nms(twins, [0.5, 0.9, 0.8], 0.5, off=[0, 2, 3]) == ([1, 1, 1], [0, 1, 0], [1, 0, 0])
    assert _nms(twins, [0.5, 0.9, 0.8], 0.5, off=[0, 1, 3]) == ([1, 1, 0], [0, 0, 0], [0, 0, 1])
    # a single box, an empty scene, no box at all
    assert _nms(CUBES[:1], [0.1], 0.0) == ([1], [0], [0])
    assert _nms(CUBES[:2], [0.1, 0.2], 0.0, off=[0, 1, 1, 2]) == ([1, 1], [0, 0], [0, 0])
    assert _nms(np.zeros((0, 8)), [], 0.5) == ([], [], [])
    assert R.cluster_sizes([1, 0, 1], [0, 0, 2]).tolist() == [2, 0, 1]
    assert R.words([0, 0, 1, 65, 193]) == 0 + 1 + 64 + 128 * 2


@pytest.fixture(scope="module")
def scenes():
    """the proposal scenes at thresh 0.25, once: size -> (rows, score, keep, rep, rank, census)"""
    out = {}
    for k in SIZES:
        rows, score = R.proposals(k, k)                                     # the seed is the size
        keep, rep, rank = R.box_nms(rows, score, 0.25)
        out[k] = (rows, score, keep, rep, rank, R.census(rows, score, 0.25, keep, rep, rank))
    return out


def test_the_proposals_chain(scenes):
    """what uniform random boxes hardly ever do: boxes kept through a chain, representatives that are not the first overlap, ties"""
    for k in SIZES:
        c = scenes[k][5]
        print(k, c)
        assert 0 < c["kept"] < k and c["kept_through"] > 0 and c["not_first"] > 0 and c["tied"] > 0 and c["largest"] > 1, (k, c)


def test_kept_boxes_do_not_overlap_and_representatives_are_kept_and_earlier(scenes):
    for k in SIZES:
        rows, score, keep, rep, rank, _ = scenes[k]
        for cls in (None, np.arange(k) % 3):
            if cls is not None:
                keep, rep, rank = R.box_nms(rows, score, 0.25, cls)
            order = np.argsort(rank)
            iou = R.ordered_iou(rows[order])
            kept = keep[order] == 1
            same = np.ones((k, k), bool) if cls is None else cls[order][:, None] == cls[order][None, :]
            assert not (iou[np.ix_(kept, kept)] > 0.25)[same[np.ix_(kept, kept)]].any()
            gone = np.flatnonzero(keep == 0)
            assert gone.size and (keep[rep[gone]] == 1).all() and (rank[rep[gone]] < rank[gone]).all()
            assert (iou[rank[rep[gone]], rank[gone]] > 0.25).all()
            assert (rep[keep == 1] == np.flatnonzero(keep == 1)).all() and sorted(rank.tolist()) == list(range(k))


def test_permuting_the_input_permutes_the_result(scenes):
    """with DISTINCT scores the order does not depend on the positions, so keep moves with the box and rep maps through the permutation"""
    for k in (65, 300):
        rows = scenes[k][0]
        rng = np.random.RandomState(k)
        score = rng.permutation(k) / float(k)
        keep, rep, rank = R.box_nms(rows, score, 0.25)
        perm = rng.permutation(k)                                            # new position p holds old box perm[p]
        keep2, rep2, rank2 = R.box_nms(rows[perm], score[perm], 0.25)
        assert np.array_equal(keep2, keep[perm]) and np.array_equal(rank2, rank[perm]) and np.array_equal(perm[rep2], rep[perm])
        assert 0 < keep.sum() < k


def _write_npz(path, k=3, kind="aabb", sem=True, **more):
    arrays = dict(center=np.arange(3 * k, dtype=np.float64).reshape(k, 3), size=np.ones((k, 3)), R=np.tile(np.eye(3), (k, 1, 1)), kind=np.array(kind),
                  values=np.arange(1, k + 1), count=np.arange(10, 10 + k), angles=np.int32(0), min_points=np.int64(1))
    if sem is not False:
        arrays["sem"] = np.full(k, 5, np.int32) if sem is True else sem
    arrays.update(more)
    np.savez(path, **arrays)


def test_what_is_refused_before_a_device_call(tmp_path, capsys):
    """on a machine without a GPU a device call is a RuntimeError: every refusal below is a ValueError, an SgError that names the limit,
    or the parser's exit, before it"""
    from seggroup_amd import boxnms, hip
    rows = np.tile(A.row(0, 0, 0, 1, 1, 1), (4, 1))
    sc = np.arange(4.0)
    for args, kw, match in (((rows[:, :7], sc, 0.5), {}, r"\[K,8\]"), ((rows.ravel(), sc, 0.5), {}, r"\[K,8\]"), ((rows, sc[:3], 0.5), {}, "scores"),
                            ((rows, sc.astype(str), 0.5), {}, "scores"), ((rows, sc, 1.0), {}, "threshold"), ((rows, sc, -0.1), {}, "threshold"),
                            ((rows, sc, float("nan")), {}, "threshold"), ((rows, sc, "0.5"), {}, "threshold"), ((rows, sc, True), {}, "threshold"),
                            ((rows, sc, 0.5), dict(cls=[1, 2, 3]), "cls"), ((rows, sc, 0.5), dict(cls=[1.0, 2, 3, 4]), "cls"),
                            ((rows, sc, 0.5), dict(off=[0, 3]), "ascend"), ((rows, sc, 0.5), dict(off=[1, 4]), "ascend"),
                            ((rows, sc, 0.5), dict(off=[0, 3, 2, 4]), "ascend"), ((rows, sc, 0.5), dict(off=[0.0, 4.0]), "whole"),
                            ((rows, sc, 0.5), dict(off=[[0, 4]]), "whole")):
        with pytest.raises(ValueError, match=match):
            boxnms.box_nms(*args, **kw)

    class Tilted:
        kind, R, center, size = "pca", np.eye(3)[None], np.zeros((1, 3)), np.ones((1, 3))
    with pytest.raises(ValueError, match="pca"):
        boxnms.box_nms(Tilted(), [1.0], 0.5)
    big = np.broadcast_to(rows[:1], ((1 << 14) + 1, 8))
    for args, kw, match in (((np.broadcast_to(rows[:1], ((1 << 20) + 1, 8)), np.zeros((1 << 20) + 1), 0.5), {}, "2\\^20"),
                            ((rows, sc, 0.5), dict(off=[0] * (1 << 16) + [0, 4]), "2\\^16"), ((big, np.zeros(big.shape[0]), 0.5), {}, "2\\^14"),
                            ((np.broadcast_to(rows[:1], (5 * 16384, 8)), np.zeros(5 * 16384), 0.5), dict(off=np.arange(6) * 16384), "2\\^24")):
        with pytest.raises(hip.SgError, match=match) as e:
            boxnms.box_nms(*args, **kw)
        assert e.value.code == hip.SG_EUNSUP
    ws = hip.lib().sg_box_nms_ws_bytes
    assert ws((1 << 20) + 1, 1, 1) == 0 and ws(1, (1 << 16) + 1, 1) == 0 and ws(1, 1, (1 << 24) + 1) == 0 and ws(-1, 1, 1) == 0 and ws(1, 1, -1) == 0
    assert ws(1 << 20, 1 << 16, 1 << 24) > (1 << 27) and ws(0, 0, 0) > 0
    assert boxnms.matrix_words([0, 0, 1, 65, 193]) == R.words([0, 0, 1, 65, 193])
    assert boxnms.cluster_sizes(boxnms.Nms(np.array([1, 0, 1, 1, 0]), np.array([0, 0, 2, 0, 0]), np.zeros(5)), [0, 3, 5]).tolist() == [2, 0, 1, 2, 0]
    # the command's options
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _write_npz(str(src / "scene0001_00.boxes.npz"))
    base = ["--boxes", str(src), "--out", str(out)]
    for argv in (base + ["--score-key", "count"], base + ["--iou", "0.5"], base + ["--iou", "1.0", "--score-key", "count"],
                 base + ["--iou", "-0.5", "--score-key", "count"], base + ["--iou", "nan", "--score-key", "count"],
                 base + ["--iou", "0.5", "--score-key", "count", "--suffix", ".npz"], base + ["--iou", "0.5", "--score-key", "count", "--suffix", "_bbox.npy"],
                 base + ["--iou", "0.5", "--score-key", "count", "--min-score", "inf"], base + ["--iou", "0.5", "--score-key", "count", "--workers", "0"],
                 ["--boxes", str(src), "--out", str(src), "--iou", "0.5", "--score-key", "count"]):
        with pytest.raises(SystemExit):
            boxnms.main(argv)
    capsys.readouterr()
    good = base + ["--iou", "0.5", "--score-key", "count"]
    for change, text in ((dict(kind="pca"), "pca"), (dict(kind="obb"), "obb"), (dict(sem=False), "sem"), (dict(count=np.arange(2)), "count"),
                         (dict(count=np.array(["a", "b", "c"])), "count")):
        _write_npz(str(src / "scene0001_00.boxes.npz"), **change)
        with pytest.raises(SystemExit):
            boxnms.main(good)
        err = capsys.readouterr().err
        assert text in err and "scene0001_00" in err, err
    _write_npz(str(src / "scene0001_00.boxes.npz"))
    with pytest.raises(SystemExit):
        boxnms.main(base + ["--iou", "0.5", "--score-key", "votes"])
    assert "votes" in capsys.readouterr().err
    listed = tmp_path / "scenes.txt"
    listed.write_text("scene0009_00\n")
    with pytest.raises(SystemExit):
        boxnms.main(good + ["--scenes", str(listed)])
    assert "scene0009_00" in capsys.readouterr().err
    det = tmp_path / "det"
    det.mkdir()
    np.save(str(det / "scene0001_00_bbox.npy"), np.ones((2, 7)))
    dbase = ["--boxes", str(det), "--out", str(out), "--suffix", "_bbox.npy", "--iou", "0.5"]
    for prepare, text in ((lambda: None, "_score.npy"), (lambda: np.save(str(det / "scene0001_00_score.npy"), np.ones(3)), "_score.npy"),
                          (lambda: (np.save(str(det / "scene0001_00_score.npy"), np.ones(2)), np.save(str(det / "scene0001_00_bbox.npy"), np.ones((2, 6)))), "[K,7]"),
                          (lambda: np.save(str(det / "scene0001_00_bbox.npy"), np.ones((2, 7)) * 1.5), "class")):
        prepare()
        with pytest.raises(SystemExit):
            boxnms.main(dbase)
        assert text in capsys.readouterr().err
    assert not out.exists()                                                  # nothing was written by a refused command
    assert boxnms.check_command(None, 0.25, "count", False, None) == dict(suffix=".boxes.npz", iou=0.25, score_key="count", class_agnostic=False,
                                                                          min_score=None)


def test_the_command_cuts_files_that_the_other_commands_read(tmp_path):
    """hand-written files of both kinds, a hand-written result: every array whose first dimension is K is cut to the kept boxes in
    ascending index, everything else is copied; boxap's and boxlabels' readers take what was written"""
    from seggroup_amd import boxap, boxlabels, boxnms
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    k = 5
    _write_npz(str(src / "s.boxes.npz"), k=k, kind="yaw", sem=np.array([5, 7, 5, 7, 9], np.int32), extra=np.arange(7), per_box=np.arange(2 * k).reshape(k, 2))
    p = boxnms.check_command(None, 0.5, "count", False, None)
    f = boxnms.read_scene(str(src), "s", p)
    assert f.rows.shape == (k, 8) and f.score.tolist() == [10, 11, 12, 13, 14] and f.cls.tolist() == [5, 7, 5, 7, 9]
    assert f.rows[:, 6].tolist() == [1.0] * k and f.rows[:, 7].tolist() == [0.0] * k and f.rows[1, :3].tolist() == [3.0, 4.0, 5.0]
    nms = boxnms.Nms(np.array([0, 1, 1, 0, 1], np.int32), np.array([2, 1, 2, 1, 4], np.int32), np.array([4, 3, 2, 1, 0], np.int32))
    boxnms.write_scene(str(out), "s", p, f, nms)
    with np.load(str(out / "s.boxes.npz")) as z, np.load(str(src / "s.boxes.npz")) as before:
        assert sorted(z.files) == sorted(before.files)
        for name in ("center", "size", "R", "values", "count", "sem", "per_box"):
            assert np.array_equal(z[name], before[name][[1, 2, 4]]), name
        for name in ("kind", "angles", "min_points", "extra"):
            assert np.array_equal(z[name], before[name]) and z[name].dtype == before[name].dtype, name
    with np.load(str(out / "s.nms.npz")) as z:
        assert z["keep"].tolist() == [0, 1, 1, 0, 1] and z["rep"].tolist() == [2, 1, 2, 1, 4] and z["rank"].tolist() == [4, 3, 2, 1, 0]
        assert z["score"].tolist() == [10, 11, 12, 13, 14]
    rows, sem, score = boxap._file_boxes(str(out / "s.boxes.npz"), "count")
    assert rows.tolist() == f.rows[[1, 2, 4]].tolist() and sem.tolist() == [7, 5, 9] and score.tolist() == [11, 12, 14]
    frames, ids, sem = boxlabels.file_boxes(str(out / "s.boxes.npz"))
    assert frames.shape == (3, 15) and ids.tolist() == [2, 3, 5] and sem.tolist() == [7, 5, 9]
    # the detector's files: [K,7] with the class in column 6, the scores beside them
    det = np.concatenate([np.arange(3 * k, dtype=np.float64).reshape(k, 3), np.ones((k, 3)), np.array([[5], [7], [5], [7], [9]], np.float64)], 1)
    np.save(str(src / "s_bbox.npy"), det)
    np.save(str(src / "s_score.npy"), np.array([0.5, 0.4, 0.3, 0.2, 0.1]))
    p = boxnms.check_command("_bbox.npy", 0.5, None, False, None)
    f = boxnms.read_scene(str(src), "s", p)
    assert f.rows[:, :6].tolist() == det[:, :6].tolist() and f.rows[:, 6:].tolist() == [[1.0, 0.0]] * k and f.cls.tolist() == [5, 7, 5, 7, 9]
    assert boxnms.read_scene(str(src), "s", dict(p, class_agnostic=True)).cls is None
    boxnms.write_scene(str(out), "s", p, f, nms)
    assert np.load(str(out / "s_bbox.npy")).tolist() == det[[1, 2, 4]].tolist() and np.load(str(out / "s_score.npy")).tolist() == [0.4, 0.3, 0.1]
    frames, ids, sem = boxlabels.file_boxes(str(out / "s_bbox.npy"))
    assert frames.shape == (3, 15) and sem.tolist() == [7, 5, 9]
    # nothing kept: files of no boxes that are still read
    boxnms.write_scene(str(out), "s", boxnms.check_command(None, 0.5, "count", False, None), boxnms.read_scene(str(src), "s", dict(p, suffix=".boxes.npz", score_key="count")),
                       boxnms.Nms(np.zeros(k, np.int32), np.full(k, -1, np.int32), np.full(k, -1, np.int32)))
    assert boxap._file_boxes(str(out / "s.boxes.npz"))[0].shape == (0, 8)


def test_the_kernels_are_in_the_library_and_use_no_scratch(sg_lib):
    """nothing of csrc/kernels_boxnms.hip is indexed at run time, and the moved pair function still is not (csrc/box_iou_device.h)"""
    import sys
    from conftest import ROOT
    from seggroup_amd import hip
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_report
    if not os.path.exists(os.path.join(scratch_report.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    kernels = scratch_report.kernels_of_library(hip.LIB_PATH)
    for needle in ("k_nm_check", "k_nm_rank", "k_nm_mask", "k_nm_scan", "k_bi_pairs", "k_bb_best"):
        mine = [(n, b, s) for n, b, _, s in kernels if needle in n]
        assert len(mine) == 1 and not any(b or s for _, b, s in mine), (needle, mine)
