"""seggroup_amd/boxset.py without a GPU: the packing of scenes into calls with caps small enough to reach every branch,
directly and through boxap.match_batch and boxnms.nms_batch with the device entry replaced by a recorder; the reader on every kind of
box file and what it and its helpers refuse; the offsets validator on one table of bad vectors."""
import numpy as np
import pytest

from seggroup_amd import boxset, hip


def _ranges(costs, caps, max_scenes):
    return list(boxset.pack(costs, caps, max_scenes))


def test_pack_takes_the_next_scene_while_every_limit_holds():
    costs = [[3, 1], [3, 1], [3, 9], [1, 1]]
    assert _ranges(costs, (6, 9), 2) == [(0, 2), (2, 3), (3, 4)]                           # 9 + 1: one more than the second cap
    assert _ranges(costs, (6, 10), 2) == [(0, 2), (2, 4)]                                  # 9 + 1 == 10: an exact fit stays in the batch
    assert _ranges(costs, (6, 10), 9) == [(0, 2), (2, 4)]                                  # 3 + 3 == 6 fits, the third 3 does not
    assert _ranges(costs, (6, 8), 9) == [(0, 2), (2, 3), (3, 4)]                           # a scene that alone exceeds a cap is still taken
    assert _ranges([[3, 1], [3, 1], [1, 1]], (6, 9), 9) == [(0, 2), (2, 3)]                # 6 + 1: one more than the cap starts the next
    assert _ranges([[3, 1], [3, 1], [1, 1]], (7, 9), 9) == [(0, 3)]
    assert _ranges([[0, 0]] * 5, (6, 9), 2) == [(0, 2), (2, 4), (4, 5)]                    # the scene count cuts a batch on its own
    assert _ranges([[7, 0], [7, 0]], (6, 9), 9) == [(0, 1), (1, 2)]                        # each alone exceeds a cap: one batch each
    assert _ranges([], (6, 9), 2) == []
    assert _ranges([(2,), (2,), (2,)], (4,), 9) == [(0, 2), (2, 3)]                        # one cost per scene is a tuple of one


def test_the_batch_drivers_pack_through_it(monkeypatch):
    """match_batch and nms_batch with small limits and their device entry replaced by a recorder: the offsets every call was given are
    the ranges pack yields"""
    from seggroup_amd import boxap, boxnms
    monkeypatch.setattr(boxset, "MAX_BOXES", 6)
    monkeypatch.setattr(boxset, "MAX_SCENES", 2)
    monkeypatch.setattr(boxnms, "MAX_WORDS", 9)
    calls = []

    def best(a, b, cls_a, cls_b, off_a, off_b, device=None, stream=None):
        calls.append((off_a.tolist(), off_b.tolist()))
        assert a.shape == (off_a[-1], 8) and b.shape == (off_b[-1], 8) and cls_a.shape == (off_a[-1],) and cls_b.shape == (off_b[-1],)
        return np.full(a.shape[0], -1, np.int32), np.zeros(a.shape[0])

    monkeypatch.setattr(boxap, "box_best", best)
    sizes = [(3, 1), (3, 1), (3, 9), (1, 1)]
    batch = [boxap.SceneBoxes(np.zeros((ka, 8)), np.full(ka, 5, np.int32), np.zeros((kb, 8)), np.full(kb, 5, np.int32), None) for ka, kb in sizes]
    got = boxap.match_batch(batch)
    assert calls == [([0, 3, 6], [0, 1, 2]), ([0, 3], [0, 9]), ([0, 1], [0, 1])]
    assert got[0].shape == (10,) and got[3].tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] and got[4] == {(0, 5): 1, (1, 5): 1, (2, 5): 9, (3, 5): 1}
    assert boxap.match_batch([])[0].shape == (0,)
    calls.clear()

    def nms(rows, score, iou, cls, off, device=None, stream=None):
        calls.append(off.tolist())
        k = rows.shape[0]
        return boxnms.Nms(np.ones(k, np.int32), np.concatenate([np.arange(b - a) for a, b in zip(off[:-1], off[1:])]).astype(np.int32)
                          if k else np.zeros(0, np.int32), np.zeros(k, np.int32))

    monkeypatch.setattr(boxnms, "box_nms", nms)
    p = boxnms.check_command(None, 0.5, "count", True, None)
    files = [boxnms.SceneFile(np.zeros((k, 8)), np.zeros(k), None, {}) for k in (3, 3, 1, 0, 5)]     # words: 3, 3, 1, 0, 5
    out = boxnms.nms_batch(files, p)
    assert calls == [[0, 3, 6], [0, 1, 1], [0, 5]]                            # 6 boxes fill the first call; two scenes the second
    assert [r.keep.tolist() for r in out] == [[1] * 3, [1] * 3, [1], [], [1] * 5] and out[4].rep.tolist() == [0, 1, 2, 3, 4]
    calls.clear()
    monkeypatch.setattr(boxset, "MAX_SCENES", 9)
    boxnms.nms_batch(files, p)
    assert calls == [[0, 3, 6], [0, 1, 1, 6]]                                 # 3 + 3 + 1 words fit 9, 7 boxes do not fit 6
    calls.clear()
    monkeypatch.setattr(boxset, "MAX_BOXES", 99)
    boxnms.nms_batch(files, p)
    assert calls == [[0, 3, 6, 7, 7], [0, 5]]                                 # the words cut: 7 + 5 > 9


def _npz(path, kind, k, sem=True, values=True, **more):
    """a .boxes.npz of k boxes; `sem`: True (classes 5, 6, ..), False (none) or the array itself"""
    arrays = dict(center=np.arange(3.0 * k).reshape(k, 3), size=np.ones((k, 3)) * 2, R=np.tile(np.eye(3), (k, 1, 1)), kind=np.array(kind),
                  count=np.arange(10, 10 + k))
    if sem is not False:
        arrays["sem"] = np.arange(5, 5 + k).astype(np.int32) if sem is True else sem
    if values:
        arrays["values"] = np.arange(1, k + 1)
    arrays.update(more)
    np.savez(path, **arrays)
    return arrays


@pytest.mark.parametrize("k", (3, 0))
def test_the_reader_on_each_kind_of_file(tmp_path, k):
    for kind in ("aabb", "yaw", "pca"):
        for sem, values in ((True, True), (False, False)):
            path = str(tmp_path / ("%s%d%d.boxes.npz" % (kind, sem, values)))
            arrays = _npz(path, kind, k, sem, values)
            f = boxset.read_boxes(path)
            assert f.path == path and f.kind == kind and sorted(f.arrays) == sorted(arrays)
            assert all(np.array_equal(f.arrays[n], a) and f.arrays[n].dtype == a.dtype for n, a in arrays.items())
            assert f.center.shape == (k, 3) and f.size.shape == (k, 3) and f.R.shape == (k, 3, 3) and f.center.dtype == f.R.dtype == np.float64
            assert f.center.tolist() == arrays["center"].tolist()
            assert (f.sem is None) == (not sem) and (f.values is None) == (not values)
            assert boxset.is_boxes(f) and boxset.box_frames(f).shape == (k, 15)
            assert boxset.file_scores(f, "count").tolist() == list(range(10, 10 + k))
            if sem:
                assert boxset.file_classes(f).tolist() == list(range(5, 5 + k)) and f.values.tolist() == list(range(1, k + 1))
            else:
                with pytest.raises(ValueError, match="holds no `sem`.*; or pass --class-agnostic"):
                    boxset.file_classes(f, "; or pass --class-agnostic")
            if kind == "pca":
                with pytest.raises(ValueError, match="a box of kind pca is not upright") as e:
                    boxset.box_rows(f, path)
                assert str(e.value).startswith(path + ": ")
            else:
                rows = boxset.box_rows(f, path)
                assert rows.shape == (k, 8) and rows[:, :3].tolist() == f.center.tolist() and rows[:, 6:].tolist() == [[1.0, 0.0]] * k
    det = np.concatenate([np.arange(3.0 * k).reshape(k, 3), np.ones((k, 3)), np.arange(5.0, 5 + k).reshape(k, 1)], 1)
    path = str(tmp_path / "s_bbox.npy")
    np.save(path, det)
    f = boxset.read_boxes(path)
    assert f.kind == "aabb" and list(f.arrays) == ["rows"] and np.array_equal(f.arrays["rows"], det) and f.values is None
    assert f.sem.dtype == np.int64 and f.sem.tolist() == list(range(5, 5 + k)) and boxset.file_classes(f).tolist() == f.sem.tolist()
    assert boxset.box_rows(f).tolist() == np.concatenate([det[:, :6], np.ones((k, 1)), np.zeros((k, 1))], 1).tolist()
    assert boxset.box_frames(f).tolist() == boxset.box_frames(det).tolist()
    with pytest.raises(ValueError, match="s_bbox.npy has no scores: .*s_score.npy must hold one per box"):
        boxset.file_scores(f)
    np.save(str(tmp_path / "s_score.npy"), np.arange(k) * 0.5)
    assert boxset.file_scores(f).tolist() == (np.arange(k) * 0.5).tolist()


def test_what_the_reader_refuses(tmp_path):
    path = str(tmp_path / "s_bbox.npy")
    for bad in (np.ones((2, 6)), np.ones((2, 8)), np.ones(7)):
        np.save(path, bad)
        with pytest.raises(ValueError, match=r"s_bbox.npy holds .*, not the \[K,7\] rows \(centre, size, class\) of `boxes --detector-files`"):
            boxset.read_boxes(path)
    np.save(path, np.ones((2, 7)) * 1.5)
    with pytest.raises(ValueError, match="s_bbox.npy: column 6 is the class, a whole number"):
        boxset.read_boxes(path)
    np.save(path, np.ones((2, 7)))
    np.save(str(tmp_path / "s_score.npy"), np.ones(3))
    with pytest.raises(ValueError, match=r"s_score.npy holds \(3,\) values for the 2 boxes of .*s_bbox.npy"):
        boxset.file_scores(boxset.read_boxes(path))
    path = str(tmp_path / "s.boxes.npz")
    _npz(path, "yaw", 3, short=np.arange(2), words=np.array(["a", "b", "c"]), sem=False, values=False)
    f = boxset.read_boxes(path)
    with pytest.raises(ValueError, match=r"s.boxes.npz has no array 'votes' \(it has R, center, count, kind, short, size, words\)"):
        boxset.file_scores(f, "votes")
    for key in ("short", "words", "kind"):
        with pytest.raises(ValueError, match="s.boxes.npz: '%s' holds .*, not one number for each of the 3 boxes" % key):
            boxset.file_scores(f, key)
    with pytest.raises(ValueError, match="holds no `sem` .the class of every box.: `boxes` writes it on its experiment route$"):
        boxset.file_classes(f)
    _npz(path, "yaw", 3, sem=np.arange(2))
    with pytest.raises(ValueError, match="s.boxes.npz: 2 classes for 3 boxes"):
        boxset.file_classes(boxset.read_boxes(path))
    _npz(path, "obb", 3)
    with pytest.raises(ValueError, match="s.boxes.npz: boxes of kind aabb or yaw are needed, not 'obb'"):
        boxset.box_rows(boxset.read_boxes(path), path)
    many = np.broadcast_to(np.zeros((1, 8)), (boxset.MAX_BOXES + 1, 8))
    with pytest.raises(hip.SgError, match="2\\^20") as e:
        boxset.box_rows(many, "who")
    assert e.value.code == hip.SG_EUNSUP
    # the scenes of a tree: listed or found, and a scene that a side lacks refused by name
    for name in ("b.boxes.npz", "a.boxes.npz", "a_bbox.npy", "c.txt"):
        (tmp_path / name).write_bytes(b"")
    assert boxset.scene_files(str(tmp_path), boxset.NPZ_SUFFIX) == {"a", "b", "s"} and boxset.scene_files(str(tmp_path), boxset.NPY_SUFFIX) == {"a", "s"}
    one = [("{}.boxes.npz under --boxes", {"a", "b"})]
    assert boxset.listed_scenes(one) == ["a", "b"] and boxset.listed_scenes(one, ["b", "a"]) == ["b", "a"]
    with pytest.raises(ValueError, match="^scene c has no c.boxes.npz under --boxes$"):
        boxset.listed_scenes(one, ["a", "c"])
    two = one + [("scan under --scans", {"b", "c"})]
    with pytest.raises(ValueError, match="^scene a has no scan under --scans: every scene needs both sides$"):
        boxset.listed_scenes(two)
    with pytest.raises(ValueError, match="^scene c has no c.boxes.npz under --boxes: every scene needs both sides$"):
        boxset.listed_scenes(two, ["b", "c"])
    assert boxset.listed_scenes(two, ["b"]) == ["b"]


def test_the_offsets_validator():
    shape, ascend = r"^who: off_x is \[B\+1\] whole numbers$", "^who: off_x must ascend from 0 to the 6 things$"
    for bad, match in (([[0, 6]], shape), (6, shape), ([], shape), ([0.0, 6.0], shape), ([1, 6], ascend), ([0, 4, 3, 6], ascend), ([0, 5], ascend),
                       ([0, 7], ascend), ([0, -1, 6], ascend)):
        with pytest.raises(ValueError, match=match):
            boxset.offsets(bad, 6, "who", "off_x", "things")
    with pytest.raises(hip.SgError, match="who: 65537 scenes; a call takes at most 2\\^16") as e:
        boxset.offsets([0] * (1 << 16) + [0, 6], 6, "who", "off_x", "things")
    assert e.value.code == hip.SG_EUNSUP
    for good in ([0, 6], [0, 0, 6, 6], np.array([0, 2, 6], np.int64), [0] * (1 << 16) + [6]):
        o = boxset.offsets(good, 6, "who", "off_x", "things")
        assert o.dtype == np.int32 and o.flags.c_contiguous and o.tolist() == list(good)
    assert boxset.offsets([0], 0, "who", "off_x", "things").tolist() == [0]               # no scene at all
    # two sets over the same scenes
    a, b = ([0, 2, 6], 6, "off_a", "boxes"), ([0, 1, 3], 3, "off_b", "points")
    oa, ob = boxset.paired_offsets("who", a, b)
    assert oa.tolist() == [0, 2, 6] and ob.tolist() == [0, 1, 3]
    oa, ob = boxset.paired_offsets("who", (None,) + a[1:], (None,) + b[1:])
    assert oa.tolist() == [0, 6] and ob.tolist() == [0, 3] and oa.dtype == ob.dtype == np.int32
    for x, y, match in (((None,) + a[1:], b, "who: off_a and off_b delimit the same scenes: both or neither"),
                        (a, (None,) + b[1:], "both or neither"), (a, ([0, 3],) + b[1:], "who: off_a and off_b name 2 and 1 scenes"),
                        (a, ([0, 1, 4],) + b[1:], "who: off_b must ascend from 0 to the 3 points")):
        with pytest.raises(ValueError, match=match):
            boxset.paired_offsets("who", x, y)
    # the class vector: checked, and never empty
    assert boxset.class_vector([3, 4], 2, "who", "cls").tolist() == [3, 4, 0] and boxset.class_vector(np.zeros(0, np.int32), 0, "who", "cls").tolist() == [0]
    for bad in ([1, 2, 3], [1.0, 2.0], [[1, 2]]):
        with pytest.raises(ValueError, match=r"^who: cls is one whole number per box, \[2\]$"):
            boxset.class_vector(bad, 2, "who", "cls")
