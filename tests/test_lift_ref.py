"""The restatement of sg_lift's rule (tests/lift_ref.py) on cases worked out by hand, and the host side of seggroup_amd/lift.py: the PNG
reader, the integer resize rule, ScanNet-shaped frame trees and the command's refusals.  No GPU: nothing here makes a device call."""
import os
import re

import numpy as np
import pytest

import lift_ref as L
import render_ref as R
from seggroup_amd import lift as M
from seggroup_amd import render

CAM = R.pixel_camera()[None]             # orthographic: world x, y are pixels (X = 256 x), depth is world z
W, H = 4, 3


def _images(label=0, depth=2.0):
    return np.full((1, H, W), label, np.int32), np.full((1, H, W), depth, np.float32)


def _one(xyz, labels, depth, tol=0.0, C=2, cams=CAM):
    return L.accumulate(np.asarray(xyz, np.float32), cams, labels, depth, tol, C, ortho=True)


def _stats(**kw):
    return dict(dict.fromkeys(L.STAT_NAMES, 0), **kw)


def test_a_vertex_on_a_pixel_boundary_goes_to_the_pixel_on_its_right():
    labels, depth = _images()
    labels[0, 1] = [0, 0, 1, 1]
    xyz = [[2.0, 1.5, 2.0], [2.0 - 1.0 / 256.0, 1.5, 2.0], [0.0, 0.0, 2.0], [3.0 + 255.0 / 256.0, 2.0 + 255.0 / 256.0, 2.0]]      # X = 512, 511, 0, 1023
    counts, seen, stats, bad = _one(xyz, labels, depth)
    assert counts.tolist() == [[0, 1], [1, 0], [1, 0], [1, 0]] and seen.tolist() == [1, 1, 1, 1] and bad == 0
    assert stats == _stats(labelled=4)


def test_one_subpixel_step_left_of_the_image_is_outside():
    labels, depth = _images()
    xyz = [[-1.0 / 256.0, 1.0, 2.0], [1.0, -1.0 / 256.0, 2.0], [4.0, 1.0, 2.0], [1.0, 3.0, 2.0], [0.0, 0.0, 2.0]]                 # X = -1; Y = -1; X = 1024; Y = 768
    counts, seen, stats, _ = _one(xyz, labels, depth)
    assert seen.tolist() == [0, 0, 0, 0, 1] and stats == _stats(outside=4, labelled=1) and counts.sum() == 1


def test_a_depth_difference_equal_to_the_tolerance_is_visible():
    labels, depth = _images(depth=1.5)
    above = np.nextafter(np.float32(2.0), np.float32(3.0))
    xyz = [[1.5, 1.5, 2.0], [1.5, 1.5, above], [1.5, 1.5, 1.0], [1.5, 1.5, np.nextafter(np.float32(1.0), np.float32(0.0))]]
    counts, seen, stats, _ = _one(xyz, labels, depth, tol=0.5)
    assert seen.tolist() == [1, 0, 1, 0] and stats == _stats(labelled=2, occluded=2)
    assert _one(xyz, labels, depth, tol=0.0)[2] == _stats(occluded=4)
    assert _one([[1.5, 1.5, 1.5]], labels, depth, tol=0.0)[2] == _stats(labelled=1)      # tol 0: equal depths are visible


def test_depths_that_are_zero_nan_infinite_or_negative_are_no_depth():
    labels, depth = _images()
    depth[0, 0] = [0.0, np.nan, np.inf, -2.0]
    depth[0, 1, 0] = -np.inf
    xyz = [[0.5, 0.5, 2.0], [1.5, 0.5, 2.0], [2.5, 0.5, 2.0], [3.5, 0.5, 2.0], [0.5, 1.5, 2.0], [1.5, 1.5, 2.0]]
    counts, seen, stats, _ = _one(xyz, labels, depth, tol=10.0)
    assert seen.tolist() == [0, 0, 0, 0, 0, 1] and stats == _stats(nodepth=5, labelled=1)


def test_a_negative_label_is_seen_and_casts_no_vote():
    labels, depth = _images(label=-1)
    labels[0, 2, 3] = -7
    counts, seen, stats, bad = _one([[0.5, 0.5, 2.0], [3.5, 2.5, 2.0]], labels, depth)
    assert seen.tolist() == [1, 1] and counts.sum() == 0 and stats == _stats(visible=2) and bad == 0
    assert [a.tolist() for a in L.vote(counts)] == [[-1, -1], [0, 0], [0, 0], [0, 0]]


def test_a_label_of_C_or_more_is_refused_and_adds_nothing():
    labels, depth = _images(label=1)
    labels[0, 0, 0] = 2
    counts, seen, stats, bad = _one([[0.5, 0.5, 2.0], [1.5, 0.5, 2.0]], labels, depth)
    assert bad == 1 and seen.tolist() == [0, 1] and counts.tolist() == [[0, 0], [0, 1]] and stats == _stats(labelled=1)


def test_behind_far_and_the_seven_counts_sum_to_all_pairs():
    labels, depth = _images()
    labels[0, 0, 1], depth[0, 0, 2] = -1, 0.0
    xyz = np.array([[0.5, 0.5, 2.0], [1.5, 0.5, 2.0], [2.5, 0.5, 2.0], [3.5, 0.5, 9.0], [9.0, 0.5, 2.0], [20000.0, 0.5, 2.0], [0.5, 0.5, 0.01], [np.nan, 0.5, 2.0]],
                   np.float32)
    cams = np.concatenate([CAM, CAM])
    cams[1, 3] = 1.0                                                             # the second camera one pixel to the left: everything lands one to the right
    lab2, dep2 = np.concatenate([labels, labels]), np.concatenate([depth, depth])
    counts, seen, stats, bad = _one(xyz, lab2, dep2, cams=cams)
    assert stats == dict(behind=4, far=2, outside=3, nodepth=2, occluded=1, visible=2, labelled=2) and bad == 0
    assert sum(stats.values()) == 2 * xyz.shape[0] and seen.sum() == stats["visible"] + stats["labelled"] and counts.sum() == stats["labelled"]


def test_a_tie_goes_to_the_lower_label_and_thresholds_drop_labels():
    # four views of one pixel: labels 30, 7, 30, 7 -> 2 : 2, the lower label 7 wins and `tied` is set; a second vertex sees 30, 30, 30, 7
    cams = np.concatenate([CAM] * 4)
    labels = np.full((4, H, W), -1, np.int32)
    labels[:, 0, 0] = [30, 7, 30, 7]
    labels[:, 0, 1] = [30, 30, 30, 7]
    labels[0, 0, 2] = 30
    depth = np.full((4, H, W), 2.0, np.float32)
    xyz = np.array([[0.5, 0.5, 2.0], [1.5, 0.5, 2.0], [2.5, 0.5, 2.0], [3.5, 0.5, 2.0]], np.float32)
    got, counts, stats = L.lift(xyz, cams, labels, depth, 0.0, ortho=True)
    assert got.label.tolist() == [7, 30, 30, -1] and got.votes.tolist() == [2, 3, 1, 0] and got.total.tolist() == [4, 4, 1, 0]
    assert got.tied.tolist() == [1, 0, 0, 0] and got.seen.tolist() == [4, 4, 4, 4] and counts.tolist() == [[2, 2], [1, 3], [0, 1], [0, 0]]
    assert stats == _stats(labelled=9, visible=7)
    assert L.lift(xyz, cams, labels, depth, 0.0, ortho=True, min_votes=2)[0].label.tolist() == [7, 30, -1, -1]
    assert L.lift(xyz, cams, labels, depth, 0.0, ortho=True, min_votes=3)[0].label.tolist() == [-1, 30, -1, -1]
    assert L.lift(xyz, cams, labels, depth, 0.0, ortho=True, min_share=0.5)[0].label.tolist() == [7, 30, 30, -1]       # 2 of 4 is half
    assert L.lift(xyz, cams, labels, depth, 0.0, ortho=True, min_share=0.75)[0].label.tolist() == [-1, 30, 30, -1]
    assert L.lift(xyz, cams, labels, depth, 0.0, ortho=True, min_share=0.76)[0].label.tolist() == [-1, -1, 30, -1]
    # the module's own host half: classes, and the vote's outputs back to labels
    cols, values = M.label_classes(labels)
    assert values.tolist() == [7, 30] and np.array_equal(cols, L.classes(labels)[0]) and cols.dtype == np.int32
    winner, votes, total, tied = L.vote(counts)
    for kw in (dict(), dict(min_votes=2), dict(min_votes=3), dict(min_share=0.75), dict(min_share=0.76)):
        mine = M.finish(winner, votes, total, got.seen, tied, values, **kw)
        want = L.lift(xyz, cams, labels, depth, 0.0, ortho=True, **kw)[0]
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(mine, want)), kw


def test_view_chunks_hold_at_most_64_views_and_2_to_26_pixels():
    assert M.view_chunks(70, 16, 12) == [(0, 64), (64, 70)] and M.view_chunks(1, 4096, 4096) == [(0, 1)]
    assert M.view_chunks(5, 4096, 4096) == [(0, 4), (4, 5)] and M.view_chunks(64, 640, 480) == [(0, 64)]      # 2^24 pixels a view: four a chunk
    assert M.view_chunks(9, 4096, 2048) == [(0, 8), (8, 9)]
    rows = M.view_rows(np.tile(R.pixel_camera(), (70, 1)))
    assert rows.shape == (70, 16)
    bad = np.tile(R.pixel_camera(), (70, 1))
    bad[66, 12] = 0.0
    with pytest.raises(ValueError, match="fx or fy"):
        M.view_rows(bad)


def test_the_function_refuses_on_the_host(monkeypatch):
    from seggroup_amd import hip

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the refusal")

    monkeypatch.setattr(hip, "require_device", no_device)
    monkeypatch.setattr(hip, "lib", no_device)
    xyz = np.zeros((5, 3), np.float32)
    labels, depth = _images()
    with pytest.raises(TypeError):
        M.lift(xyz, CAM, labels, depth)                                           # tol has no default
    for kw, word in ((dict(tol=-1.0), "tol="), (dict(tol=float("nan")), "tol="), (dict(tol=None), "tol="), (dict(tol=0.1, min_votes=0), "min_votes="),
                     (dict(tol=0.1, min_share=1.5), "min_share="), (dict(tol=0.1, near=0.0), "near="), (dict(tol=0.1, point_size=4), "point_size=")):
        with pytest.raises(ValueError, match=word):
            M.lift(xyz, CAM, labels, depth, **kw)
    for lab, dep, word in ((labels[0], depth, "labels="), (labels.astype(np.float32), depth, "labels="), (np.concatenate([labels, labels]), depth, "labels="),
                           (labels, depth[:, :2], "depth="), (labels, depth.astype(np.int32), "depth=")):
        with pytest.raises(ValueError, match=word):
            M.lift(xyz, CAM, lab, dep, tol=0.1)
    with pytest.raises(ValueError, match="faces="):
        M.lift(xyz, CAM, labels, None, np.zeros((4, 2), np.int32), tol=0.1)
    many = np.arange(5000, dtype=np.int32).reshape(1, 50, 100)
    with pytest.raises(ValueError, match="5000 distinct labels"):
        M.lift(xyz, CAM, many, np.ones((1, 50, 100), np.float32), tol=0.1)


# ---- PNGs ---------------------------------------------------------------------------------------------------------------------------------------
def test_read_png_reads_what_write_png_writes(tmp_path):
    rng = np.random.RandomState(1)
    rgb = rng.randint(0, 256, (13, 31, 3)).astype(np.uint8)
    grey = rng.randint(0, 65536, (7, 5)).astype(np.uint16)
    grey[0, :2] = [0, 65535]
    for name, img in (("rgb.png", rgb), ("grey.png", grey), ("one.png", grey[:1, :1])):
        render.write_png(str(tmp_path / name), img)
        back = M.read_png(str(tmp_path / name))
        assert back.dtype == img.dtype and np.array_equal(back, img), name


@pytest.mark.parametrize("filters", ((1,), (2,), (3,), (4,), (0, 1, 2, 3, 4), (4, 3, 2, 1, 0)), ids=str)
def test_read_png_undoes_every_scanline_filter(tmp_path, filters):
    rng = np.random.RandomState(sum(filters))
    images = dict(grey8=rng.randint(0, 256, (9, 17)).astype(np.uint8), grey16=rng.randint(0, 65536, (8, 11)).astype(np.uint16),
                  rgb=rng.randint(0, 256, (6, 7, 3)).astype(np.uint8), column=rng.randint(0, 256, (5, 1)).astype(np.uint8))
    for name, img in images.items():
        path = str(tmp_path / (name + ".png"))
        L.write_filtered_png(path, img, filters)
        back = M.read_png(path)
        assert back.dtype == img.dtype and back.shape == img.shape and np.array_equal(back, img), name


def test_read_png_refuses_by_name(tmp_path):
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    path = str(tmp_path / "bad.png")
    L.write_filtered_png(path, img, (0,), lace=1)
    with pytest.raises(ValueError, match="interlaced"):
        M.read_png(path)
    L.write_filtered_png(path, img, (0,), colour=3)
    with pytest.raises(ValueError, match="palette"):
        M.read_png(path)
    L.write_filtered_png(path, np.zeros((3, 4), np.uint16), (0,), colour=4)            # grey + alpha at 16 bits
    with pytest.raises(ValueError, match="colour type 4 at 16 bits"):
        M.read_png(path)
    with open(path, "wb") as f:
        f.write(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        M.read_png(path)
    L.write_filtered_png(path, img, (0,))
    raw = bytearray(open(path, "rb").read())
    raw[40] ^= 1                                                                 # inside the tEXt chunk: its CRC fails
    with open(path, "wb") as f:
        f.write(bytes(raw))
    with pytest.raises(ValueError, match="CRC"):
        M.read_png(path)


def test_depth_from_millimetres_keeps_zero():
    d = M.depth_from_mm(np.array([[0, 1, 1234, 65535]], np.uint16))
    assert d.dtype == np.float32 and d.tolist() == [[0.0, np.float32(0.001), np.float32(1.234), np.float32(65.535)]]
    assert M.depth_from_mm(np.array([250], np.uint16), scale=4000.0).tolist() == [0.0625]
    with pytest.raises(ValueError, match="depth_from_mm"):
        M.depth_from_mm(np.zeros(3, np.float32))


def test_the_integer_nearest_rule_five_to_three():
    """sx = ((2 x + 1) * 5) // 6 for x = 0, 1, 2: 5 // 6, 15 // 6, 25 // 6 = 0, 2, 4; three to five: ((2 x + 1) * 3) // 10 = 0, 0, 1, 2, 2"""
    src = np.array([[10, 11, 12, 13, 14]], np.uint16)
    assert M.resize_nearest(src, (3, 1)).tolist() == [[10, 12, 14]]
    assert M.resize_nearest(src[:, :3], (5, 1)).tolist() == [[10, 10, 11, 12, 12]]
    grid = np.arange(25).reshape(5, 5)
    assert M.resize_nearest(grid, (3, 3)).tolist() == [[0, 2, 4], [10, 12, 14], [20, 22, 24]]
    assert M.resize_nearest(grid, (5, 5)).tolist() == grid.tolist() and M.resize_nearest(grid, (1, 1)).tolist() == [[12]]
    big = np.arange(968 * 1296, dtype=np.int64).reshape(968, 1296)               # ScanNet's colour frames onto its depth frames
    out = M.resize_nearest(big, (640, 480))
    assert out.shape == (480, 640) and out[0, 0] == big[1, 1] and out[479, 639] == big[((2 * 479 + 1) * 968) // 960, ((2 * 639 + 1) * 1296) // 1280]


# ---- a ScanNet-shaped tree -----------------------------------------------------------------------------------------------------------------------
def test_a_scannet_shaped_tree_numeric_order_every_and_lost_tracking(tmp_path):
    d, K, tree = L.scannet_tree(tmp_path)
    assert M.scannet_frame_names(d) == ["0", "1", "2", "10", "11"] and M.scannet_frame_names(d, 2) == ["0", "2", "11"]
    fr = M.load_scannet_frames(d)
    assert fr.used == ["0", "1", "10", "11"] and fr.skipped == ["2"] and fr.ortho is False
    assert fr.rows.shape == (4, 16) and fr.label.shape == (4, 6, 8) and fr.label.dtype == np.int32 and fr.depth.dtype == np.float32
    for k, f in enumerate(fr.used):
        P, depth, lab, _ = tree[f]
        assert np.array_equal(fr.rows[k], render.from_pose(P, K).row()) and fr.rows[k, 14] == 4.0 and fr.rows[k, 15] == 3.0      # centres on halves
        assert np.array_equal(fr.depth[k], (depth.astype(np.float64) / 1000.0).astype(np.float32)) and (fr.depth[k][depth == 0] == 0).all()
        assert np.array_equal(fr.label[k], lab[1::2, 1::2])                       # 16 -> 8: ((2 x + 1) * 16) // 16 = 2 x + 1
    every = M.load_scannet_frames(d, "instance-filt", 2)
    assert every.used == ["0", "11"] and every.skipped == ["2"]
    assert np.array_equal(every.label[1], tree["11"][3][1::2, 1::2])
    os.remove(os.path.join(d, "depth", "10.png"))
    with pytest.raises(ValueError, match="10.png is missing"):
        M.load_scannet_frames(d)
    lost, _, _ = L.scannet_tree(tmp_path / "lost", frames=("0", "1"), lost=("0", "1"))
    with pytest.raises(ValueError, match="no frame with a finite pose .2 skipped."):
        M.load_scannet_frames(lost)


def test_frames_files_are_checked_on_the_host(tmp_path):
    path = str(tmp_path / "s.frames.npz")
    T = np.tile(np.eye(4)[None], (3, 1, 1))
    K = np.tile([5.0, 5.0, 2.0, 1.5], (3, 1))
    label = np.zeros((3, 3, 4), np.int16)
    np.savez(path, T=T, K=K, label=label, depth=np.ones((3, 3, 4), np.float32), ortho=True)
    fr = M.load_frames(path)
    assert fr.rows.shape == (3, 16) and fr.ortho is True and fr.depth.shape == (3, 3, 4) and fr.label.dtype == np.int32 and fr.skipped == []
    np.savez(path, T=T[:, :3], K=K, label=label)
    fr = M.load_frames(path)
    assert fr.depth is None and fr.ortho is False and len(fr.used) == 3
    np.savez(path, T=T, K=K)
    with pytest.raises(ValueError, match="needs the arrays T, K and label"):
        M.load_frames(path)
    np.savez(path, T=T, K=K[:2], label=label)
    with pytest.raises(ValueError, match="--frames"):
        M.load_frames(path)
    np.savez(path, T=T, K=K, label=label[:2])
    with pytest.raises(ValueError, match="labels="):
        M.load_frames(path)


# ---- the command's refusals: all before the device is asked for ----------------------------------------------------------------------------------
BASE = ["--scans", "nowhere", "--out", "nowhere"]
REFUSALS = [
    (["--tol", "0.05"], "exactly one source of frames"),
    (["--tol", "0.05", "--frames", "a", "--scannet-frames", "b"], "exactly one source of frames"),
    (["--frames", "a"], "--tol is needed"),
    (["--frames", "a", "--tol", "-0.01"], "--tol is needed"),
    (["--frames", "a", "--tol", "nan"], "--tol is needed"),
    (["--frames", "a", "--tol", "inf"], "--tol is needed"),
    (["--frames", "a", "--tol", "0.05", "--every", "2"], "--image-kind and --every belong to --scannet-frames"),
    (["--frames", "a", "--tol", "0.05", "--image-kind", "label-filt"], "--image-kind and --every belong to --scannet-frames"),
    (["--scannet-frames", "a", "--tol", "0.05", "--every", "0"], "--every"),
    (["--scannet-frames", "a", "--tol", "0.05", "--every", "-3"], "--every"),
    (["--scannet-frames", "a", "--tol", "0.05", "--image-kind", "color"], "--image-kind is label-filt or instance-filt"),
    (["--frames", "a", "--tol", "0.05", "--min-share", "1.01"], "--min-share"),
    (["--frames", "a", "--tol", "0.05", "--min-share", "-0.1"], "--min-share"),
    (["--frames", "a", "--tol", "0.05", "--min-votes", "0"], "--min-votes"),
    (["--frames", "a", "--tol", "0.05", "--style-name", "lifted"], "--style-name needs --root"),
    (["--frames", "a", "--tol", "0.05", "--style-name", "lifted", "--root", "r"], "--style-name needs --root ROOT .* and --as"),
    (["--frames", "a", "--tol", "0.05", "--style-name", "lifted", "--as", "ins"], "--style-name needs --root"),
    (["--frames", "a", "--tol", "0.05", "--style-name", "a/b", "--root", "r", "--as", "ins"], "--style-name is the name of one directory"),
    (["--frames", "a", "--tol", "0.05", "--style-name", "lifted", "--root", "r", "--as", "seg"], "--as is ins or sem"),
    (["--frames", "a", "--tol", "0.05", "--as", "ins"], "--as belongs to --style-name"),
    (["--frames", "a", "--tol", "0.05", "--near", "0"], "--near"),
    (["--frames", "a", "--tol", "0.05", "--point-size", "4"], "--point-size"),
    (["--frames", "a", "--tol", "0.05", "--workers", "0"], "--workers"),
]


@pytest.mark.parametrize("args, message", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_the_command_refuses_before_any_device_work(args, message, capsys, monkeypatch):
    from seggroup_amd import hip

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the refusal")

    monkeypatch.setattr(hip, "require_device", no_device)
    monkeypatch.setattr(hip, "lib", no_device)
    with pytest.raises(SystemExit) as e:
        M.main(BASE + args)
    assert e.value.code == 2
    assert re.search(message, capsys.readouterr().err), args


def test_the_parameters_in_force():
    p = M.check_command(scannet_frames="d", tol=0.05)
    assert p["image_kind"] == "label-filt" and p["every"] == 1 and p["tol"] == 0.05 and p["min_votes"] == 1 and p["min_share"] == 0.0 and not p["snap"]
    p = M.check_command(frames="d", tol=0, style_name="lifted", root="r", as_="sem", snap=True, min_share=1.0)
    assert p["image_kind"] is None and p["every"] is None and p["tol"] == 0.0 and p["as_"] == "sem" and p["snap"] and p["min_share"] == 1.0
