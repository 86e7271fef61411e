"""sg_click_clusters (csrc/clicks.cpp) without a GPU: the same cluster lists as `labels.group_adjacency_segs` over the dense
matrix -- list order and member order, which the reference's argmax, its unstable argsort and its random draws depend on -- its refusals,
and `generate_weak_labels` from a pair list against the dense path on an instance of 40 equal-sized segments."""
import ctypes as C
import os

import numpy as np
import pytest

import seggraph_ref as G

os.environ.setdefault("SEGGROUP_HOST_ONLY", "1")


def _reference(pairs, seg_ins, S):
    """what the dense path computes: per instance in ascending value, group_adjacency_segs over its ascending segments"""
    from seggroup_amd import labels
    m = G.dense_matrix(pairs, S)
    lists, ins_of = [], []
    for ins in np.unique(seg_ins[seg_ins > 0]):
        got = labels.group_adjacency_segs(m, np.nonzero(seg_ins == ins)[0])
        lists += got
        ins_of += [int(ins)] * len(got)
    return lists, ins_of


def _check(pairs, seg_ins, S, what):
    from seggroup_amd import seggraph
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    off, members, ins = seggraph.click_clusters(pairs, seg_ins, S)
    lists, ins_of = _reference(pairs, np.asarray(seg_ins), S)
    assert off.dtype == members.dtype == ins.dtype == np.int32
    assert G.cluster_lists(off, members) == lists, what
    assert ins.tolist() == ins_of, what
    assert all(l[0] == max(l) for l in lists) and [l[0] for i, l in enumerate(lists)] == sorted(
        [l[0] for l in lists], key=lambda s: (seg_ins[s], s)), "a cluster starts with its highest segment; clusters ascend by it inside an instance"
    return lists


def _unique_pairs(p):
    p = np.asarray(p, np.int64).reshape(-1, 2)
    p = p[p[:, 0] != p[:, 1]]
    return np.unique(np.sort(p, axis=1), axis=0).astype(np.int32) if p.size else np.zeros((0, 2), np.int32)


def test_random_graphs(sg_lib):
    rng = np.random.default_rng(5)
    for trial in range(60):
        S = int(rng.integers(1, 70))
        pairs = _unique_pairs(rng.integers(0, S, (int(rng.integers(0, 3 * S)), 2)))
        seg_ins = rng.choice([0, 0, 1, 2, 3, 7, -4], S) if trial % 3 else rng.integers(1, 3, S)
        _check(pairs, seg_ins, S, f"trial {trial}")


def test_chain_star_and_segments_without_an_instance(sg_lib):
    S = 50
    one = np.ones(S, np.int64)
    chain = np.stack([np.arange(S - 1), np.arange(1, S)], 1)
    assert _check(chain, one, S, "chain") == [list(range(S - 1, -1, -1))]
    back = _unique_pairs(np.stack([np.arange(S - 1), np.arange(1, S)], 1)[::3])
    _check(back, one, S, "broken chain")
    star_low = np.stack([np.zeros(S - 1, np.int64), np.arange(1, S)], 1)                 # the hub is the lowest segment
    assert _check(star_low, one, S, "star, hub 0") == [list(range(S - 1, -1, -1))]
    star_high = np.stack([np.arange(S - 1), np.full(S - 1, S - 1)], 1)                   # ... and the highest
    assert _check(star_high, one, S, "star, hub S-1") == [[S - 1] + list(range(S - 1))]
    # a long chain: O(k) lists and finds, not the reference's k^2 probes
    from seggroup_amd import seggraph
    k = 200000
    off, members, ins = seggraph.click_clusters(np.stack([np.arange(k - 1), np.arange(1, k)], 1), np.ones(k), k)
    assert off.tolist() == [0, k] and np.array_equal(members, np.arange(k - 1, -1, -1)) and ins.tolist() == [1]
    # segments without an instance join nothing and bridge nothing: 0 - 1 - 2 with 1 unlabeled stays two clusters
    assert _check([[0, 1], [1, 2]], np.array([4, 0, 4]), 3, "bridge") == [[0], [2]]
    assert _check([[0, 1], [1, 2]], np.array([4, -1, 4]), 3, "bridge") == [[0], [2]]
    assert _check([[0, 1], [1, 2]], np.array([4, 5, 4]), 3, "two instances") == [[0], [2], [1]]
    off, members, ins = seggraph.click_clusters(np.zeros((0, 2), np.int32), np.zeros(4), 4)
    assert off.tolist() == [0] and members.size == 0 and ins.size == 0
    # the absorbed list keeps its own order: 3 takes [2, 0] whole, then [1]
    assert _check([[0, 2], [0, 3], [1, 3]], np.ones(4, np.int64), 4, "order") == [[3, 2, 0, 1]]


def test_forty_equal_segments(sg_lib):
    """one instance of 40 segments in a 8 x 5 block grid: more than 16 members, where the reference's argsort is no longer stable and the
    member order decides which segments are the "largest\""""
    adj, seg = G.lattice(80, 50, 10)
    seg = np.random.default_rng(3).permutation(40).astype(np.int32)[seg]          # the numbers do not follow the grid
    pairs, _ = G.segment_graph(adj, seg, 40)
    lists = _check(pairs, np.ones(40, np.int64), 40, "grid")
    assert len(lists) == 1 and len(lists[0]) == 40 and lists[0] != sorted(lists[0], reverse=True)
    assert len(_check(pairs[::3], np.ones(40, np.int64), 40, "a third of the grid's pairs")) > 1


def test_refusals(sg_lib):
    from seggroup_amd import hip, seggraph
    ok_ins = np.ones(5, np.int32)
    for pairs, word in (([[1, 1]], "not (lower, higher)"), ([[2, 1]], "not (lower, higher)"), ([[0, 5]], "outside 0..4"), ([[-1, 2]], "outside 0..4"),
                        ([[0, 2], [0, 1]], "do not ascend"), ([[0, 1], [0, 1]], "do not ascend"), ([[1, 2], [0, 3]], "do not ascend")):
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
            seggraph.click_clusters(np.array(pairs, np.int32), ok_ins, 5)
    with pytest.raises(ValueError, match="one instance per segment"):
        seggraph.click_clusters(np.zeros((0, 2), np.int32), ok_ins, 6)
    L = sg_lib
    buf = (C.c_int32 * 64)()
    p, n_c = C.addressof(buf), C.c_int(3)
    assert L.sg_click_clusters(p, 0, p, 0, p, p, p, C.byref(n_c)) == hip.SG_EINVAL
    assert L.sg_click_clusters(None, 1, p, 4, p, p, p, C.byref(n_c)) == hip.SG_EINVAL
    assert L.sg_click_clusters(p, -1, p, 4, p, p, p, C.byref(n_c)) == hip.SG_EINVAL
    assert L.sg_click_clusters(p, 0, p, 4, p, p, p, None) == hip.SG_EINVAL
    assert L.sg_click_clusters(None, 0, p, 4, p, p, p, C.byref(n_c)) == hip.SG_OK and n_c.value == 0


@pytest.mark.parametrize("style,kw", [("maxseg", {}), ("maxseg", {"anno_num": 3}), ("maxseg", {"anno_num": 2, "main_num": 5}), ("rand", {}),
                                      ("mainseg", {"main_num": 20, "anno_num": 4})])
def test_weak_labels_equal_the_dense_path_on_forty_equal_segments(tmp_path, style, kw):
    """an instance of 40 equal-sized segments (plus one of 8 in two parts, and unlabeled vertices): same clicks, files and counts"""
    from seggroup_amd import labels, prepare
    adj, seg = G.lattice(80, 60, 10)                              # 8 x 6 segments of 100 vertices
    V = seg.shape[0]
    ins = np.where(seg < 40, 1, 0)
    ins[np.isin(seg, (40, 41, 42, 45, 46, 47))] = 2                # two parts of three segments
    sem = np.where(ins > 0, ins + 2, 0)
    seg = np.random.default_rng(3).permutation(48).astype(np.int32)[seg]          # the numbers do not follow the grid
    name = "grid40"
    scene = tmp_path / "scans" / name
    scene.mkdir(parents=True)
    col, row = np.arange(V) % 80, np.arange(V) // 80
    quad = np.nonzero((col + 1 < 80) & (row + 1 < 60))[0]
    faces = np.concatenate([np.stack([quad, quad + 1, quad + 81], 1), np.stack([quad, quad + 81, quad + 80], 1)]).astype(np.int32)
    xyz = np.stack([col * 0.04, row * 0.04, np.zeros(V)], 1).astype(np.float32)
    prepare.write_ply(str(scene / (name + "_vh_clean_2.ply")), xyz, np.zeros((V, 3), np.uint8), faces)
    raw = tmp_path / "label" / "real" / "raw" / name
    raw.mkdir(parents=True)
    for ext, vals in (("seg", seg), ("ins", ins), ("sem", sem)):
        (raw / f"{name}.{ext}.txt").write_text("".join("%d\n" % v for v in vals))
    f3 = faces.astype(np.int64)
    graph = G.segment_graph(np.concatenate([f3[:, [0, 1]], f3[:, [0, 2]], f3[:, [1, 2]]]), seg, 48)
    out = {}
    for which, sg in (("dense", "dense"), ("pairs", graph)):
        root = tmp_path / which
        (root / "label" / "real").mkdir(parents=True)
        os.symlink(raw.parent, root / "label" / "real" / "raw")
        ret = labels.generate_weak_labels(str(scene), None, label_style=style, root=str(root), seg_graph=sg, rng=np.random.RandomState(9), **kw)
        d = root / "label" / "seg" / prepare.weak_style_dir(style, kw.get("main_num", -1), kw.get("anno_num", 1)) / "raw" / name
        out[which] = (ret, (d / f"{name}.ins.txt").read_bytes(), (d / f"{name}.sem.txt").read_bytes())
    assert out["dense"] == out["pairs"]
    ret = out["dense"][0]
    assert ret[3:] == (48, 2) and ret[1] == V and ret[2] >= 3, "three clusters of at least 100 vertices are clicked"
