"""Geodesic distances without a GPU: tests/geodesic_ref.py on hand cases that are exact, the order-freedom of the rule
itself, the tie class of a unit grid, everything seggroup_amd/geodesic.py and its command refuse before a device call, the host halves
of the module, the command's files on a hand-written tree, and the kernels in the built library."""
import json
import os

import numpy as np
import pytest

import geodesic_ref as R

INF = float("inf")


def _geo(V, seeds, edges, **kw):
    s = np.full(V, -1)
    s[list(seeds)] = 1
    dist, owner = R.geodesic(V, s, np.asarray(edges, np.int64).reshape(-1, 2), **kw)
    return dist.tolist(), owner.tolist()


def test_hand_cases_are_exact():
    # the path 0-1-2-3-4 with both ends seeds: the middle is tied and goes to the lower seed
    assert _geo(5, [0, 4], R.path(5)) == ([0, 1, 2, 1, 0], [0, 0, 0, 4, 4])
    # an absorbed weight: 3 -1.0- 1 -1e-20- 2 -1.0- 0 with the seeds 3 and 0.  D(1) = D(2) = 1 and 1 <-> 2 is a TIGHT CYCLE (1 + 1e-20 == 1
    # both ways), so 1 is reached from the seed 0 over tight arcs although its own best walk comes from 3: owner 0, the lower seed
    assert 1.0 + 1e-20 == 1.0
    assert _geo(4, [0, 3], [[3, 1], [1, 2], [2, 0]], weights=[1.0, 1e-20, 1.0]) == ([0, 1, 1, 0], [0, 0, 0, 3])
    # a zero-weight arc between two seeds: both ways tight, so the higher seed and all it reaches belong to the lower one
    assert _geo(4, [1, 3], [[3, 1], [3, 2], [0, 1]], weights=[0.0, 1.0, 2.0]) == ([2, 0, 1, 0], [1, 1, 1, 1])
    # duplicate rows with different weights in both orientations: the smallest wins, and all of them count
    assert _geo(2, [0], [[0, 1], [1, 0], [0, 1]], weights=[5.0, 2.0, 3.0]) == ([0, 2], [0, 0])
    # a self loop is a no-op, whatever it weighs
    assert _geo(3, [0], [[0, 1], [1, 1], [1, 2]], weights=[1.5, 0.25, 1.5]) == ([0, 1.5, 3.0], [0, 0, 0])
    # an unreached component
    assert _geo(5, [1], [[0, 1], [3, 4]]) == ([1, 0, INF, INF, INF], [1, 1, -1, -1, -1])
    # max_dist exactly at a vertex's distance keeps it (the test is "above"); one ulp below drops it and all behind it
    third = 0.1 + 0.2                                                        # 0.30000000000000004: the rounded sum IS the distance
    w = [0.1, 0.2, 0.5]
    assert _geo(4, [0], R.path(4), weights=w) == ([0, 0.1, third, third + 0.5], [0, 0, 0, 0])
    assert _geo(4, [0], R.path(4), weights=w, max_dist=third) == ([0, 0.1, third, INF], [0, 0, 0, -1])
    assert _geo(4, [0], R.path(4), weights=w, max_dist=float(np.nextafter(third, 0.0))) == ([0, 0.1, INF, INF], [0, 0, -1, -1])
    assert _geo(4, [0], R.path(4), weights=w, max_dist=0.0) == ([0, INF, INF, INF], [0, -1, -1, -1])
    # no seed; every vertex a seed (with a zero weight: O(s) <= s); one vertex; no edge
    assert _geo(3, [], R.path(3)) == ([INF] * 3, [-1] * 3)
    assert _geo(3, [0, 1, 2], R.path(3), weights=[1.0, 0.0]) == ([0, 0, 0], [0, 1, 1])
    assert _geo(1, [0], np.zeros((0, 2))) == ([0], [0]) and _geo(1, [], [[0, 0]]) == ([INF], [-1])
    assert _geo(3, [2], np.zeros((0, 2))) == ([INF, INF, 0], [-1, -1, 2])
    # lengths come from float32 coordinates widened to double: 3-4-5 is exact, and coincident points are a zero weight
    xyz = np.float32([[0, 0, 0], [3, 4, 0], [3, 4, 0], [3, 4, 12]])
    assert _geo(4, [0, 2], R.path(4), xyz=xyz) == ([0, 0, 0, 12], [0, 2, 2, 2])
    assert R.face_sides([[0, 1, 2]]).tolist() == [[0, 1], [1, 2], [0, 2]]
    assert R.stats(4, [-1, 0, -1, -1], [[0, 1], [1, 1], [1, 0], [2, 3]]) == (6, 2, 2)


def test_the_rule_does_not_depend_on_the_order():
    """the in-place relaxation over shuffled arc subsets ends at the restatement's bytes: weights that are random doubles (sums that
    round) and quantised ones (sums that tie), three shuffles each"""
    V = 300
    edges, quant = R.random_graph(V, 1200, 5, isolated=10)
    seeds = np.full(V, -1)
    seeds[[3, 77, 150]] = 0
    for weights in (np.random.RandomState(0).rand(edges.shape[0]), quant):
        src, dst, w = R.arcs(edges, weights=weights)
        want, _ = R.geodesic(V, seeds, edges, weights=weights)
        assert np.isinf(want).sum() >= 10 and np.isfinite(want).sum() > 200
        for shuffle in range(3):
            got = R.relax_shuffled(V, src, dst, w, seeds, np.random.RandomState(100 + shuffle))
            assert got.tobytes() == want.tobytes(), shuffle


def test_ties_go_to_the_lowest_seed():
    """the unit 33 x 33 grid with its corners as seeds: the vertices of the middle row and the middle column are as far from two corners
    (the centre from four), and their owner is the lowest of them"""
    n = 33
    V = n * n
    edges = R.unit_grid(n)
    corners = [0, n - 1, n * (n - 1), V - 1]
    seeds = np.full(V, -1)
    seeds[corners] = 7
    dist, owner = R.geodesic(V, seeds, edges)
    src, dst, w = R.arcs(edges)
    alone = np.stack([R.dijkstra(V, src, dst, w, np.where(np.arange(V) == c, 0, -1)) for c in corners])
    assert np.array_equal(dist, alone.min(0))
    nearest = alone == dist[None, :]                                         # unit weights: reached over tight arcs iff as near as the nearest
    tied = nearest.sum(0) > 1
    assert tied.sum() == 65 and tied[V // 2] and nearest[:, V // 2].all()
    assert np.array_equal(owner, np.asarray(corners)[nearest.argmax(0)])      # argmax: the first, so the lowest, of the tied corners
    assert np.array_equal(R.highest_owners(V, src, dst, w, dist, seeds) != owner, tied)


# ---- the module -------------------------------------------------------------------------------------------------------------------------------
def test_what_the_module_refuses_before_a_device_call():
    """on a machine without a GPU a device call is a RuntimeError: every refusal below is a ValueError before it"""
    from seggroup_amd import geodesic as G
    e, s, f = R.path(4), np.array([0, -1, -1, -1]), np.array([[0, 1, 2], [1, 2, 3]])
    xyz = np.zeros((4, 3), np.float32)
    for args, kw, match in (((0, s[:0]), dict(edges=e), "V is"), ((4.0, s), dict(edges=e), "V is"), ((True, s[:1]), dict(edges=e), "V is"),
                            (((1 << 27) + 1, s), dict(edges=e), "2\\^27"), ((4, s[:3]), dict(edges=e), "seeds"),
                            ((4, s.astype(np.float64)), dict(edges=e), "seeds"), ((4, s.reshape(2, 2)), dict(edges=e), "seeds"),
                            ((4, s), {}, "exactly one"), ((4, s), dict(edges=e, faces=f), "exactly one"), ((4, s), dict(edges=e.ravel()), "edges"),
                            ((4, s), dict(edges=e.astype(np.float32)), "edges"), ((4, s), dict(edges=f), "edges"), ((4, s), dict(faces=e), "faces"),
                            ((4, s), dict(edges=e.astype(np.int64) + (1 << 32)), "int32"),
                            ((4, s), dict(edges=np.broadcast_to(e[:1], ((1 << 26) + 1, 2))), "2\\^26"),
                            ((4, s), dict(faces=np.broadcast_to(f[:1], ((1 << 26) // 3 + 1, 3))), "2\\^26"),
                            ((4, s), dict(edges=e, xyz=xyz, weights=np.ones(3)), "at most one"), ((4, s), dict(faces=f, weights=np.ones(2)), "edges="),
                            ((4, s), dict(edges=e, weights=np.ones(4)), "weights"), ((4, s), dict(edges=e, weights=np.array(["a", "b", "c"])), "weights"),
                            ((4, s), dict(edges=e, xyz=xyz[:3]), "xyz"), ((4, s), dict(edges=e, xyz=xyz[:, :2]), "xyz"), ((4, s), dict(edges=e, xyz=xyz.ravel()), "xyz"),
                            ((4, s), dict(edges=e, max_dist=-1.0), "max_dist"), ((4, s), dict(edges=e, max_dist=float("nan")), "max_dist"),
                            ((4, s), dict(edges=e, max_dist="1"), "max_dist"), ((4, s), dict(edges=e, max_dist=True), "max_dist")):
        with pytest.raises(ValueError, match=match):
            G.geodesic(*args, **kw)
    assert G.check_max_dist(None) == INF and G.check_max_dist(float("inf")) == INF and G.check_max_dist(0) == 0.0
    V, seeds, rows, is_faces, weights, limit = G.check_graph(4, s.tolist(), faces=f, xyz=xyz, max_dist=2)
    assert (V, is_faces, weights, limit) == (4, True, None, 2.0) and seeds.dtype == np.int32 and rows.dtype == np.int32 and rows.shape == (2, 3)


def test_the_library_entry_without_a_device(sg_lib):
    """the envelope of the workspace function, the stats' refusal, and every host check of sg_graph_geodesic: they come before the first
    HIP call, so they are the same answers on a machine without a GPU (the pointers are never followed)"""
    import ctypes as C
    from seggroup_amd import hip
    ws = sg_lib.sg_graph_geodesic_ws_bytes
    assert ws(0, 0) == 0 and ws(-1, 5) == 0 and ws(1, -1) == 0 and ws((1 << 27) + 1, 0) == 0 and ws(1, (1 << 26) + 1) == 0
    assert ws(1, 0) > 0 and ws(1 << 27, 1 << 26) > 28 * (1 << 27) and ws(1000, 3000) < ws(1000, 6000)
    h = (C.c_int64 * 5)()
    assert sg_lib.sg_graph_geodesic_stats(h, 4) == hip.SG_EINVAL and b"sg_graph_geodesic_stats" in sg_lib.sg_last_error()
    assert sg_lib.sg_graph_geodesic_stats(None, 5) == hip.SG_EINVAL
    assert sg_lib.sg_graph_geodesic_stats(h, 5) == 5
    buf = np.zeros(64, np.float64)                                           # a host buffer: an address that is never followed
    p, need = buf.ctypes.data, ws(4, 3)

    def call(edges=p, E=3, V=4, xyz=None, stride=0, weight=None, seed=p, max_dist=INF, dist=p, owner=p, d_ws=p, ws_bytes=need):
        rc = sg_lib.sg_graph_geodesic(edges, E, V, xyz, stride, weight, seed, max_dist, dist, owner, d_ws, ws_bytes, None)
        return rc, sg_lib.sg_last_error().decode()

    for kw, text in ((dict(V=0), "0 vertices"), (dict(E=-1), "-1 edge rows"), (dict(edges=None), "null"), (dict(seed=None), "null"), (dict(dist=None), "null"),
                     (dict(owner=None), "null"), (dict(d_ws=None), "null"), (dict(xyz=p, weight=p, stride=3), "at most one"), (dict(xyz=p, stride=2), "at least 3"),
                     (dict(max_dist=-1e-300), "max_dist"), (dict(max_dist=float("nan")), "max_dist"), (dict(max_dist=-INF), "max_dist"),
                     (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace")):
        rc, msg = call(**kw)
        assert rc == hip.SG_EINVAL and "sg_graph_geodesic" in msg and text in msg, (kw, rc, msg)
    for kw, text in ((dict(V=(1 << 27) + 1), "at most"), (dict(E=(1 << 26) + 1), "2^26")):
        rc, msg = call(**kw)
        assert rc == hip.SG_EUNSUP and "sg_graph_geodesic" in msg and text in msg, (kw, rc, msg)


def _numpy_vote(seg, cols, n_cols):
    """rekey.vote's rows on the host: the distinct ids ascending, per id the column most of its vertices hold, the lowest among equals"""
    ids = np.unique(seg)
    table = np.zeros((ids.shape[0], n_cols), np.int64)
    np.add.at(table, (np.searchsorted(ids, seg), cols), 1)
    return ids, table.argmax(1)


def test_propagate_and_snap_on_hand_arrays():
    from seggroup_amd import geodesic as G
    labels = np.array([9, -1, -1, 4, -1])
    assert G.propagate(labels, np.array([0, 0, 3, 3, -1], np.int32)).tolist() == [9, 9, 4, 4, -1]
    assert G.propagate(labels, np.full(5, -1, np.int32)).tolist() == [-1] * 5
    for bad in (np.array([0, 0, 3]), np.array([0, 0, 3, 3, 5]), np.array([0.0, 0, 3, 3, 1])):
        with pytest.raises(ValueError, match="propagate"):
            G.propagate(labels, bad)
    # segment 7: 9 9 4 -> 9; segment 2: a tie of 4 and 9 -> the lower label; segment 5: 4 against two unreached -> unreached;
    # segment 8: a tie of 9 and unreached -> 9 (the unreached column is the last)
    seg = np.array([7, 7, 7, 2, 2, 5, 5, 5, 8, 8])
    lab = np.array([9, 9, 4, 9, 4, 4, -1, -1, -1, 9])
    cols, values = G.label_columns(lab)
    assert values.tolist() == [4, 9] and cols.tolist() == [1, 1, 0, 1, 0, 0, 2, 2, 2, 1] and cols.dtype == np.int32
    ids, winner = _numpy_vote(seg, cols, 3)
    snapped, moved = G.snapped_labels(seg, lab, values, ids, winner)
    assert snapped.tolist() == [9, 9, 9, 4, 4, -1, -1, -1, 9, 9] and moved == 0.4
    assert G.label_columns(np.array([-1, -1]))[1].shape == (0,) and G.label_columns(np.array([-1, -1]))[0].tolist() == [0, 0]
    with pytest.raises(ValueError, match="snap_to_segments"):
        G.label_columns(np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match="snap_to_segments"):
        G.snap_to_segments(seg[:3], lab)


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def _tree(tmp_path, scenes=("scene0001_00", "scene0002_00")):
    """a hand-written two-scene tree: a strip of two triangles a scene (faces in the PLY), adj.pth, a clicked style and the real labels"""
    import torch
    from seggroup_amd import labels, prepare
    root, scans_dir = str(tmp_path / "root"), str(tmp_path / "scans")
    xyz = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    faces = np.int32([[0, 1, 2], [1, 3, 2]])
    for k, s in enumerate(scenes):
        os.makedirs(os.path.join(scans_dir, s))
        prepare.write_ply(os.path.join(scans_dir, s, s + "_vh_clean_2.ply"), xyz + k, np.zeros((4, 3), np.uint8), faces)
        d = os.path.join(root, "adj", "mesh", "raw", s)
        os.makedirs(d)
        torch.save(torch.from_numpy(R.face_sides(faces).astype(np.int64)), os.path.join(d, s + ".adj.pth"))
        for style, ins, sem in (("seg/clicks", [3, -1, -1, -1], [5, -1, -1, -1]), ("real", [3, 3, 3, 3], [5, 5, 5, 5])):
            labels._write_txt(os.path.join(root, "label", style, "raw", s, s + ".ins.txt"), ins)
            labels._write_txt(os.path.join(root, "label", style, "raw", s, s + ".sem.txt"), sem)
    return root, scans_dir


def test_what_the_command_refuses_and_what_it_names(tmp_path, capsys, sg_lib):
    from seggroup_amd import geodesic as G
    root, scans_dir = _tree(tmp_path)
    out = str(tmp_path / "out")
    base = ["--scans", scans_dir, "--root", root, "--out", out]
    good = base + ["--label_style", "clicks"]
    for argv, text in ((base, "--label_style"), (good + ["--style-name", "clicks"], "--style-name clicks is --label_style"),
                       (good + ["--style-name", "a/b"], "one directory"), (base + ["--label_style", ".."], "one directory"),
                       (good + ["--metric", "euclid"], "--metric"), (good + ["--max-dist", "-0.5"], "max_dist"), (good + ["--max-dist", "nan"], "max_dist"),
                       (good + ["--workers", "0"], "--workers"), (base + ["--label_style", "taps"], "taps"),
                       (good + ["--snap"], "segs.json"), (good + ["--snap"], ".seg.txt")):
        with pytest.raises(SystemExit):
            G.main(argv)
        err = capsys.readouterr().err
        assert text in err, (argv, err)
    # a scene without its graph is named, with the way to get it; and a scene that the list names and the tree does not hold
    adj = os.path.join(root, "adj", "mesh", "raw", "scene0002_00", "scene0002_00.adj.pth")
    os.rename(adj, adj + ".away")
    with pytest.raises(SystemExit):
        G.main(good)
    err = capsys.readouterr().err
    assert "scene0002_00.adj.pth" in err and "prepare" in err
    os.rename(adj + ".away", adj)
    os.remove(os.path.join(root, "label", "real", "raw", "scene0001_00", "scene0001_00.sem.txt"))
    with pytest.raises(SystemExit):
        G.main(good + ["--score"])
    assert "scene0001_00.sem.txt" in capsys.readouterr().err
    assert not os.path.exists(out)                                           # nothing was written by a refused command
    p = G.check_command("clicks", None, None, False, None, False)
    assert p == dict(label_style="clicks", metric="length", max_dist=None, snap=False, style_name=None, score=False)
    assert G.check_command("clicks", "hops", 0.5, True, "geo", True)["max_dist"] == 0.5
    files = G.scene_files(os.path.join(scans_dir, "scene0002_00"), root, p)
    assert files["adj"] == adj and files["ins"].endswith(os.path.join("label", "seg", "clicks", "raw", "scene0002_00", "scene0002_00.ins.txt"))
    # a scene whose .npz OUT holds already is skipped, and a run that skips every scene needs no device
    os.makedirs(out)
    for s in ("scene0001_00", "scene0002_00"):
        np.savez(os.path.join(out, s + G.NPZ_SUFFIX), dist=np.zeros(4), owner=np.zeros(4, np.int32), ins=np.full(4, 3, np.int32), sem=np.full(4, 5, np.int32))
    assert G.main(good) == 0
    assert "0 written, 2 skipped" in capsys.readouterr().out
    doc = json.load(open(os.path.join(out, G.REPORT_NAME)))
    assert doc == {"parameters": dict(label_style="clicks", metric="length", snap=False, score=False), "scenes": {}, "skipped": ["scene0001_00", "scene0002_00"]}
    # --force runs the scenes again: that needs a device
    if sg_lib.sg_device_count() <= 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            G.main(good + ["--force"])
        return
    assert G.main(good + ["--force", "--style-name", "geo", "--workers", "1"]) == 0
    with np.load(os.path.join(out, "scene0002_00" + G.NPZ_SUFFIX)) as z:
        assert sorted(z.files) == ["dist", "ins", "owner", "sem"] and z["owner"].tolist() == [0] * 4 and z["ins"].tolist() == [3] * 4
        assert z["dist"].tolist() == [0.0, 1.0, 1.0, 2.0] and z["sem"].tolist() == [5] * 4
    from seggroup_amd import labels
    assert labels.load_labels(os.path.join(root, "label", "seg", "geo", "raw", "scene0001_00", "scene0001_00.ins.txt")) == [3] * 4


def test_the_kernels_are_in_the_library_and_use_no_scratch(sg_lib):
    import sys
    from conftest import ROOT
    from seggroup_amd import hip
    for name in ("sg_graph_geodesic_ws_bytes", "sg_graph_geodesic", "sg_graph_geodesic_stats"):
        assert name in hip.SIGNATURES and hasattr(sg_lib, name)
    # geodesic.TILE, which places the GPU tests' sizes, is the kernel's tile
    import re
    from seggroup_amd import geodesic as G
    src = open(os.path.join(ROOT, "seggroup_amd", "csrc", "kernels_geodesic.hip")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    assert re.search(r"constexpr int kTile = kBlock;", src) and G.TILE == block
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_report
    if not os.path.exists(os.path.join(scratch_report.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    kernels = scratch_report.kernels_of_library(hip.LIB_PATH)
    for needle, count in (("k_gd_keys", 1), ("k_gd_rows", 1), ("k_gd_arcs", 1), ("k_gd_init", 1), ("k_gd_relax", 2), ("k_gd_tight", 1), ("k_gd_finish", 1)):
        mine = [(n, b, s) for n, b, _, s in kernels if needle in n]
        assert len(mine) == count and not any(b or s for _, b, s in mine), (needle, mine)
