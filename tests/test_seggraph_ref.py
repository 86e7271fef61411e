"""The segment graph without a GPU: the NumPy statement of tests/seggraph_ref.py against tests/ops_ref.py's contraction, the
arguments sg_segment_graph refuses before the first device call, `generate_weak_labels` fed with a graph the caller already has against
the capture of the reference (tests/golden/prep_labels.npz, the fixture recipe of tests/test_labels.py), and the refusals of
`python -m seggroup_amd.prepare`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ops_ref
import seggraph_ref as G
from conftest import ROOT

os.environ.setdefault("SEGGROUP_HOST_ONLY", "1")
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _cases():
    for S in ops_ref.CONTRACT_S:
        adj, seg, N = ops_ref.contract_case(S)
        yield "contract %d" % S, adj[((adj >= 0) & (adj < N)).all(axis=1)], seg, S
    for shape in G.SHAPES:
        yield (shape,) + G.shape_case(shape)
    for E, S in ((0, 3), (1, 2), (65, 1), (4097, 1024), (12289, 2049), (2049, 1 << 20)):
        yield ("E=%d S=%d" % (E, S),) + G.size_case(E, S) + (S,)


def test_statement_is_the_contraction_with_counts():
    for what, adj, seg, S in _cases():
        pairs, cross = G.segment_graph(adj, seg, S)
        assert pairs.dtype == np.int32 and cross.dtype == np.int32 and pairs.shape == (cross.shape[0], 2), what
        assert np.array_equal(pairs, ops_ref.contract(adj, seg, seg.shape[0], S)), what
        a, b = seg[adj[:, 0]], seg[adj[:, 1]]
        assert int(cross.sum()) == int(((a >= 0) & (b >= 0) & (a != b)).sum()), what
        assert (cross >= 1).all() and (pairs[:, 0] < pairs[:, 1]).all(), what
        key = pairs[:, 0].astype(np.int64) << G.bits_for(S) | pairs[:, 1]
        assert (np.diff(key) > 0).all() and (key.size == 0 or int(key.max()).bit_length() <= 40), what


def test_the_shapes_hold_what_they_are_for():
    got = {s: G.segment_graph(*G.shape_case(s)) for s in G.SHAPES}
    assert got["inside"][0].shape[0] == 0
    assert got["one_pair"][0].tolist() == [[5, 9]] and got["one_pair"][1].tolist() == [5000]
    assert got["distinct"][0].shape[0] == 120 * 119 // 2 and (got["distinct"][1] == 1).all()
    assert (G.shape_case("negative")[1] < 0).sum() == 1000 and got["negative"][0].shape[0] > 400
    assert (got["mirrored"][1] % 4 == 0).all()
    adj, seg, S = G.shape_case("mesh")
    assert (seg[adj[:, 0]] != seg[adj[:, 1]]).mean() < 0.25 and S == 12 * 9
    for a, b in zip(got["mesh"], got["shuffled"]):
        assert np.array_equal(a, b)
    assert [2 * G.bits_for(S) for S in G.S_SIZES] == [0, 2, 4, 20, 24, 40]


def test_library_refuses_before_the_first_device_call(sg_lib):
    from seggroup_amd import hip
    buf = (C.c_char * 4096)()                                     # never read: every call below is refused on its arguments
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    n_p = C.c_longlong(7)
    L = sg_lib
    big = 1 << 40
    call = lambda adj, E, seg, V, S, pairs, cross, hp, ws, nbytes: L.sg_segment_graph(adj, E, seg, V, S, pairs, cross, hp, ws, nbytes, None)
    hp = C.byref(n_p)
    for i in range(6):                                            # each pointer in turn
        ptrs = [p, p, p, p, hp, p]
        ptrs[i] = None
        assert call(ptrs[0], 10, ptrs[1], 10, 4, ptrs[2], ptrs[3], ptrs[4], ptrs[5], big) == hip.SG_EINVAL, i
        assert b"null pointer" in L.sg_last_error()
    assert call(p, -1, p, 10, 4, p, p, hp, p, big) == hip.SG_EINVAL
    assert call(p, 10, p, 10, 0, p, p, hp, p, big) == hip.SG_EINVAL
    assert call(p, 10, p, 0, 4, p, p, hp, p, big) == hip.SG_EINVAL and b"V = 0" in L.sg_last_error()
    assert call(p + 8, 10, p, 10, 4, p, p, hp, p, big) == hip.SG_EINVAL and b"16-byte" in L.sg_last_error()
    assert call(p, 10, p, 10, (1 << 20) + 1, p, p, hp, p, big) == hip.SG_EUNSUP and b"1048577" in L.sg_last_error()
    assert call(p, 1 << 31, p, 10, 4, p, p, hp, p, big) == hip.SG_EUNSUP and b"2147483648" in L.sg_last_error()
    assert call(p, (1 << 31) - 1, p, 10, 1 << 20, p, p, hp, p, 1 << 20) == hip.SG_ENOMEM, "the largest call is sized, not refused"
    for E, S in ((0, 1), (1, 2), (5000, 1024), (5000, 1 << 20)):
        need = L.sg_segment_graph_ws_bytes(E, S)
        assert need > 16 * max(E, 1) // (2 if S <= 1 << 16 else 1)
        assert call(p, E, p, 10, S, p, p, hp, p, need - 256) == hip.SG_ENOMEM
        err = L.sg_last_error()
        assert b"(%d < %d)" % (need - 256, need) in err, err
    assert L.sg_segment_graph_ws_bytes(5000, 1 << 20) > L.sg_segment_graph_ws_bytes(5000, 1 << 16), "64-bit keys past 32 key bits"
    for E, S in ((-1, 4), (1 << 31, 4), (10, 0), (10, (1 << 20) + 1)):
        assert L.sg_segment_graph_ws_bytes(E, S) == 0
    # E = 0 is a call like any other: no pair, no device work
    n_p.value = 7
    assert call(p, 0, p, 10, 4, p, p, hp, p, L.sg_segment_graph_ws_bytes(0, 4)) == hip.SG_OK and n_p.value == 0


# ---- generate_weak_labels on a graph the caller already has, against the capture of the reference -------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import torch
    import capture_labels as cl
    from oracle import prep_ref
    from seggroup_amd import labels, prepare, synthetic
    fx = cl.FIXTURE
    scan = synthetic.make_raw_scan(fx["w"], fx["h"], fx["seed"], name=fx["name"], cell=fx["cell"])
    ann = synthetic.make_annotations(scan, 11, blocks_per_row=-(-fx["w"] // fx["cell"]))
    td = str(tmp_path_factory.mktemp("seggraph_labels"))
    scene_path = cl.write_inputs(td, scan, ann)
    prepare.write_ply(os.path.join(scene_path, scan.name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
    mapper = prep_ref.make_mapper(scan.xyz.shape[0], fx["num_points"], scan.perm)
    os.makedirs(os.path.join(td, "data", "resampled", scan.name))
    torch.save(torch.from_numpy(mapper), os.path.join(td, "data", "resampled", scan.name, scan.name + ".map.pth"))
    raw_lab, _ = prep_ref.segment_lists(scan.seg_indices, mapper)
    os.makedirs(os.path.join(td, "label", "real", "raw", scan.name))
    with open(os.path.join(td, "label", "real", "raw", scan.name, scan.name + ".seg.txt"), "w") as f:
        f.write("".join("%d\n" % v for v in raw_lab))
    labels.generate_real_labels(scene_path, root=td)
    f3 = np.asarray(scan.faces, np.int64)
    edges = np.concatenate([f3[:, [0, 1]], f3[:, [0, 2]], f3[:, [1, 2]]])
    graph = G.segment_graph(edges, np.asarray(raw_lab), int(np.max(raw_lab)) + 1)
    return td, scene_path, scan, graph


@pytest.mark.parametrize("draws", ["seed", "rng"])
@pytest.mark.parametrize("style,kw", [("manual", {}), ("maxseg", {}), ("maxseg", {"anno_num": 2}), ("rand", {}), ("mainseg", {"main_num": 3})])
def test_weak_labels_from_a_given_graph_match_the_capture(tree, style, kw, draws):
    import torch
    import capture_labels as cl
    from seggroup_amd import labels
    td, scene_path, scan, graph = tree
    g = np.load(os.path.join(GOLD, "prep_labels.npz"))
    d = cl.style_dir(style, kw)
    if draws == "seed":
        np.random.seed(1)
        rng = None
    else:
        np.random.seed(12345)                                     # not read: the draws come from rng
        rng = np.random.RandomState(1)
    ret = labels.generate_weak_labels(scene_path, None, label_style=style, manual_label_path=os.path.join(td, "manual"), root=td,
                                      seg_graph=graph, rng=rng, **kw)
    assert list(ret) == g[f"{d}.ret"].tolist()
    raw = os.path.join(td, "label", "seg", d, "raw", scan.name)
    assert np.array_equal(np.array(labels.load_labels(os.path.join(raw, scan.name + ".ins.txt"))), g[f"{d}.ins"])
    assert np.array_equal(np.array(labels.load_labels(os.path.join(raw, scan.name + ".sem.txt"))), g[f"{d}.sem"])
    labels.generate_weak_label_pth(scan.name, d, root=td)
    t = torch.load(os.path.join(td, "label", "seg", d, "resampled", scan.name, scan.name + ".label.pth"))
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), g[f"{d}.label_pth"])


def test_the_default_is_the_dense_path_and_other_names_are_refused(tree):
    from seggroup_amd import labels
    td, scene_path, scan, graph = tree
    with pytest.raises(ValueError, match="seg_graph"):
        labels.generate_weak_labels(scene_path, None, label_style="maxseg", root=td, seg_graph="mesh")
    g = np.load(os.path.join(GOLD, "prep_labels.npz"))
    np.random.seed(1)
    assert list(labels.generate_weak_labels(scene_path, None, label_style="rand", root=td, rng=None)) == g["rand.ret"].tolist()
    assert list(labels.generate_weak_labels(scene_path, None, label_style="rand", root=td, rng=np.random.RandomState(1))) == g["rand.ret"].tolist()


def test_a_segment_with_two_instances_is_named(tree):
    from seggroup_amd import labels
    td, scene_path, scan, graph = tree
    raw = os.path.join(td, "label", "real", "raw", scan.name)
    seg = np.array(labels.load_labels(os.path.join(raw, scan.name + ".seg.txt")))
    ins = np.array(labels.load_labels(os.path.join(raw, scan.name + ".ins.txt")))
    pts, sins, distinct = labels.segment_table(seg, ins, on_device=False)
    assert np.array_equal(pts, np.bincount(seg)) and (distinct == 1).all()
    assert all(sins[s] == ins[seg == s][0] for s in range(0, pts.shape[0], 7))
    v = int(np.nonzero(ins > 0)[0][0])
    broken = ins.copy()
    broken[v] = ins.max() + 1
    assert labels.segment_table(seg, broken, on_device=False)[2][seg[v]] == 2
    path = os.path.join(raw, scan.name + ".ins.txt")
    keep = open(path).read()
    try:
        with open(path, "w") as f:
            f.write("".join("%d\n" % x for x in broken))
        with pytest.raises(ValueError, match="segment %d holds 2 instance values" % seg[v]):
            labels.generate_weak_labels(scene_path, None, label_style="maxseg", root=td, seg_graph=graph)
        labels.generate_weak_labels(scene_path, None, label_style="maxseg", root=td)          # the dense default still takes the file
    finally:
        with open(path, "w") as f:
            f.write(keep)


# ---- the command's refusals: argparse ends them before a device is asked for ------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [
    (["--label_style", "manual"], "--manual_label_path"),
    (["--label_style", "mainseg", "--main_num", "2", "--anno_num", "3"], "--anno_num <= --main_num"),
    (["--label_style", "mainseg"], "--main_num >= 1"),
    (["--label_style", "clicks"], "invalid choice"),
    (["--seg-graph", "mesh"], "invalid choice"),
    (["--knn", "5", "--radius", "0.1"], "not allowed with"),
    (["--workers", "0"], "--workers must be in"),
    (["--index", "tree"], "invalid choice"),
    ([], "--data_root"),
])
def test_command_refusals(argv, word, capsys):
    from seggroup_amd import prepare
    with pytest.raises(SystemExit) as e:
        prepare.main((["--data_root", "/nowhere"] if argv else []) + argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_scene_draws_depend_on_seed_and_name_alone():
    import zlib
    from seggroup_amd import prepare
    a = prepare.scene_rng(3, "scene0000_00").randint(0, 1 << 30, 5)
    assert np.array_equal(a, np.random.RandomState(zlib.crc32(b"3/scene0000_00")).randint(0, 1 << 30, 5))
    assert not np.array_equal(a, prepare.scene_rng(4, "scene0000_00").randint(0, 1 << 30, 5))
    assert not np.array_equal(a, prepare.scene_rng(3, "scene0000_01").randint(0, 1 << 30, 5))
    assert prepare.weak_style_dir("mainseg", 3, 2) == "mainseg_3_a2" and prepare.weak_style_dir("maxseg", 3, 1) == "maxseg"
    lines = prepare.summary_lines([(10, 100, 2, 20, 3), (30, 100, 4, 20, 5)], 2)
    assert lines == ["Average labeled points of weak label in all points: 20.00%", "Average labeled segments of weak label in all segments: 15.00%",
                     "Average real labeled points in all points: 3.0000%", "Average instance number per scene: 4.00",
                     "Average labeled segment number per scene: 3.00"]
