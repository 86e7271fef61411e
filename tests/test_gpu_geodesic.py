"""Geodesic distances on the GPU (seggroup_amd/geodesic.py) against tests/geodesic_ref.py: dist and owner EQUAL to the
restatement -- the rules are exact and order-free --, the refusals, and the command as the training-free baseline on a U-shaped strip."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import geodesic_ref as R
import pcseg_ref as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


def _seeds(V, where, value=3):
    s = np.full(V, -1, np.int32)
    s[np.asarray(where, np.int64)] = value
    return s


def _same(got, want, what=""):
    dist, owner = want
    assert got.dist.dtype == np.float64 and got.owner.dtype == np.int32 and got.dist.shape == dist.shape and got.owner.shape == owner.shape, what
    bad = np.flatnonzero(got.dist.view(np.int64) != dist.view(np.int64))
    assert bad.size == 0, (what, "dist", bad.size, bad[:8].tolist(), got.dist[bad[:8]].tolist(), dist[bad[:8]].tolist())
    bad = np.flatnonzero(got.owner != owner)
    assert bad.size == 0, (what, "owner", bad.size, bad[:8].tolist(), got.owner[bad[:8]].tolist(), owner[bad[:8]].tolist())


def _check(V, seeds, edges=None, faces=None, xyz=None, weights=None, max_dist=None, want=None, what=""):
    """one call against the restatement, the stats of the call included (the launch counts are informative) -> (result, stats)"""
    from seggroup_amd import geodesic as G
    got = G.geodesic(V, seeds, edges=edges, faces=faces, xyz=xyz, weights=weights, max_dist=max_dist, device=DEV)
    stats = G.last_stats()
    rows = R.face_sides(faces) if faces is not None else edges
    _same(got, want if want is not None else R.geodesic(V, seeds, rows, xyz, weights, max_dist), what)
    arcs, tight, reached = R.stats(V, seeds, rows, xyz, weights, max_dist)
    assert (stats["arcs"], stats["tight_arcs"], stats["reached"]) == (arcs, tight, reached), (what, stats)
    assert rows.shape[0] == 0 or (stats["distance_launches"] >= 1 and stats["owner_launches"] >= 1), (what, stats)
    print(what, stats)
    return got, stats


def _tangle(V, seed):
    """a graph on V vertices that holds every one of them: a path in shuffled order and V random chords, quantised weights"""
    rng = np.random.RandomState(seed)
    edges = np.concatenate([R.path(V, rng.permutation(V)), rng.randint(0, V, (V, 2)).astype(np.int32)])
    return edges, rng.randint(0, 6, edges.shape[0]) / 4.0


def test_sizes_and_tile_edges():
    """either side of a wave and of the tile a workgroup owns, and two tiles + 1"""
    from seggroup_amd import geodesic as G
    assert G.TILE == 256
    for V in (1, 2, 63, 64, 65, G.TILE - 1, G.TILE, G.TILE + 1, 2 * G.TILE + 1):
        edges, w = _tangle(V, V) if V > 1 else (np.zeros((0, 2), np.int32), np.zeros(0))
        for where in ([0], [V - 1], sorted({0, V // 2, V - 1})):
            seeds = _seeds(V, where)
            _check(V, seeds, edges, weights=w, what=("weights", V, where))
            _check(V, seeds, edges, what=("hops", V, where))


@pytest.fixture(scope="module")
def sheet():
    """the jittered 40 x 40 sheet and its restatements, once: {(metric, seeds): (seed vector, dist, owner)}"""
    xyz, faces = R.grid_mesh(40, 40, 1)
    edges = R.face_sides(faces)
    rng = np.random.RandomState(9)
    out = {}
    for n in (1, 5, 50):
        seeds = _seeds(1600, rng.choice(1600, n, replace=False))
        out["length", n] = (seeds,) + R.geodesic(1600, seeds, edges, xyz=xyz)
        out["hops", n] = (seeds,) + R.geodesic(1600, seeds, edges)
    return xyz, faces, edges, out


@pytest.mark.parametrize("n", (1, 5, 50))
def test_a_jittered_sheet_by_every_metric_and_both_sources(sheet, n):
    xyz, faces, edges, known = sheet
    seeds, dist, owner = known["length", n]
    assert np.isfinite(dist).all() and np.unique(owner).shape[0] == n
    for source in (dict(edges=edges), dict(faces=faces)):
        _check(1600, seeds, xyz=xyz, want=(dist, owner), what=("length", n, list(source)), **source)
        _check(1600, seeds, want=known["hops", n][1:], what=("hops", n, list(source)), **source)
    _check(1600, seeds, edges=edges, weights=R.lengths(edges, xyz), want=(dist, owner), what=("weights", n))
    wide = np.concatenate([xyz, np.full((1600, 3), np.nan, np.float32)], 1)          # rows of 6 floats: only the first three are read
    _check(1600, seeds, edges=edges, xyz=wide, want=(dist, owner), what=("stride 6", n))


def test_a_path_in_shuffled_and_in_index_order():
    """4,097 vertices and one seed at an end.  Shuffled, a launch carries the distance about one hop (a tile writes back after its sweeps):
    thousands of launches, so the batches of launches and the changed word.  In index order a tile advances as many hops a launch as it has
    inner sweeps: one in the build, so all V + 1 launches of the bound."""
    V = 4097
    perm = np.random.RandomState(2).permutation(V)
    for name, order in (("shuffled", perm), ("in order", np.arange(V))):
        edges = R.path(V, order)
        want = np.empty(V)
        want[order] = np.arange(V)
        got, stats = _check(V, _seeds(V, [order[0]]), edges, what=name)
        assert np.array_equal(got.dist, want) and (got.owner == order[0]).all()
        assert 8 < stats["distance_launches"] <= V + 1 and 8 < stats["owner_launches"] <= V + 1      # more than one batch: the loop and the changed word


def test_a_star_of_degree_5000():
    """the centre's row is longer than a lane walks: it is split over a wave"""
    V = 5001
    edges = R.star(5000)
    for where in ([17], [0], [4999, 5000]):
        _check(V, _seeds(V, where), edges, what=("hops", where))
        _check(V, _seeds(V, where), edges, weights=np.random.RandomState(1).randint(0, 9, 5000) / 8.0, what=("weights", where))
    moved = (edges.astype(np.int64) + 300) % V                                # the centre in the middle of a tile
    _check(V, _seeds(V, [2, 4000]), moved.astype(np.int32), what="centre 300")


def test_a_random_graph_with_duplicates_self_loops_and_unreached_vertices():
    V = 5000
    edges, w = R.random_graph(V, 20000, 3, isolated=100)
    seeds = _seeds(V, np.random.RandomState(1).choice(V, 40, replace=False))
    assert (edges[:, 0] == edges[:, 1]).sum() >= 400
    got, _ = _check(V, seeds, edges, weights=w, what="quantised")
    assert 60 <= np.isinf(got.dist).sum() < 1000 and (got.owner[np.isinf(got.dist)] == -1).all()
    src, dst, ww = R.arcs(edges, weights=w)
    assert (R.highest_owners(V, src, dst, ww, got.dist, seeds) != got.owner).sum() > 100     # ties: what the owner rule is about
    _check(V, seeds, edges, weights=np.random.RandomState(4).rand(20000), what="random doubles")
    _check(V, seeds, edges, what="hops")


def test_the_unit_grid_and_its_tie_class():
    n = 33
    V = n * n
    edges = R.unit_grid(n)
    seeds = _seeds(V, [0, n - 1, n * (n - 1), V - 1])
    got, _ = _check(V, seeds, edges, what="unit grid")
    src, dst, w = R.arcs(edges)
    tied = R.highest_owners(V, src, dst, w, got.dist, seeds) != got.owner
    assert tied.sum() == 65 and got.owner[V // 2] == 0 and (got.owner[tied] < V - 1).all()


def test_coincident_points_are_zero_lengths():
    xyz, faces = R.grid_mesh(30, 30, 3)
    xyz[1::4] = xyz[0:-1:4]                                                  # every fourth vertex sits on its neighbour
    xyz[500:560] = xyz[500]
    edges = R.face_sides(faces)
    assert (R.lengths(edges, xyz) == 0.0).sum() > 200
    seeds = _seeds(900, [3, 501, 540, 899])
    got, stats = _check(900, seeds, faces=faces, xyz=xyz, what="coincident")
    assert (got.dist[500:560] == 0.0).all() and (got.owner[500:560] == 501).all()     # the seeds 501 and 540 sit on one point: the lower owns it


def test_max_dist_against_the_mask(sheet):
    xyz, faces, edges, known = sheet
    seeds, dist, owner = known["length", 5]
    at = float(np.sort(dist)[800])
    for limit in (at, float(np.nextafter(at, 0.0)), 0.0, float(dist.max()), 1e300, INF):
        got, _ = _check(1600, seeds, faces=faces, xyz=xyz, max_dist=limit, want=R.mask(dist, owner, limit), what=("max_dist", limit))
        assert np.isfinite(got.dist).sum() == (dist <= limit).sum()
    assert (dist <= at).sum() == 801 and (dist <= np.nextafter(at, 0.0)).sum() == 800
    hops = known["hops", 5]
    _check(1600, seeds, edges=edges, max_dist=7, want=R.mask(hops[1], hops[2], 7), what="7 hops")


def test_same_bytes_on_a_second_call_and_a_second_stream(sheet):
    import torch
    from seggroup_amd import geodesic as G
    xyz, faces, _, known = sheet
    seeds, dist, owner = known["length", 50]
    first = G.geodesic(1600, seeds, faces=faces, xyz=xyz, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    for stream in (None, side, side):
        again = G.geodesic(1600, seeds, faces=faces, xyz=torch.from_numpy(xyz).to(DEV), device=DEV, stream=stream)
        assert again.dist.tobytes() == first.dist.tobytes() and again.owner.tobytes() == first.owner.tobytes()
    _same(first, (dist, owner))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raw(edges, V, seeds, xyz=None, weights=None, max_dist=INF, E=None, stride=None, null=(), ws_bytes=None):
    """the library itself, past the module's own checks -> (return code, sg_last_error)"""
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    d_e = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32)).to(DEV)
    d_s = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.int32)).to(DEV)
    d_x = None if xyz is None else torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(DEV)
    d_w = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(DEV)
    n = int(d_s.shape[0])
    d_dist, d_owner = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.sg_graph_geodesic_ws_bytes(n, int(d_e.shape[0]))), 256), dtype=torch.uint8, device=DEV)
    ptrs = dict(edges=d_e.data_ptr(), seed=d_s.data_ptr(), dist=d_dist.data_ptr(), owner=d_owner.data_ptr(), ws=ws.data_ptr())
    for name in null:
        ptrs[name] = None
    rc = lib.sg_graph_geodesic(ptrs["edges"], int(d_e.shape[0]) if E is None else E, V, hip.ptr(d_x), (xyz.shape[1] if xyz is not None else 0) if stride is None else stride,
                               hip.ptr(d_w), ptrs["seed"], max_dist, ptrs["dist"], ptrs["owner"], ptrs["ws"], ws.numel() if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, lib.sg_last_error().decode()


def test_refusals_leave_the_next_calls_right():
    from seggroup_amd import geodesic as G
    from seggroup_amd import hip
    xyz, faces = R.grid_mesh(9, 7, 5)
    V = 63
    edges = R.face_sides(faces)
    lens = R.lengths(edges, xyz)
    seeds = _seeds(V, [4, 60])
    want_len, want_hops = R.geodesic(V, seeds, edges, xyz=xyz), R.geodesic(V, seeds, edges)

    def valid():
        _same(G.geodesic(V, seeds, edges=edges, xyz=xyz, device=DEV), want_len)
        _same(G.geodesic(V, seeds, faces=faces, device=DEV), want_hops)

    valid()
    # through the flag word: the module passes these on, and the library names itself
    for row, value in ((5, (-1, 3)), (0, (2, V)), (edges.shape[0] - 1, (1 << 30, 0)), (7, (-(1 << 31), -(1 << 31)))):
        bad = edges.copy()
        bad[row] = value
        with pytest.raises(ValueError, match="outside 0..62") as e:
            G.geodesic(V, seeds, edges=bad, xyz=xyz, device=DEV)
        assert "sg_graph_geodesic" in str(e.value)
        valid()
    for value in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        bad = lens.copy()
        bad[11] = value
        with pytest.raises(ValueError, match="weight") as e:
            G.geodesic(V, seeds, edges=edges, weights=bad, device=DEV)
        assert "sg_graph_geodesic" in str(e.value)
        valid()
    for vertex, column, value in ((int(edges[3, 0]), 0, np.nan), (int(edges[20, 1]), 2, np.inf), (V - 1, 1, -np.inf)):
        bad = xyz.copy()
        bad[vertex, column] = value
        with pytest.raises(ValueError, match="coordinate") as e:
            G.geodesic(V, seeds, edges=edges, xyz=bad, device=DEV)
        assert "sg_graph_geodesic" in str(e.value)
        valid()
    # a coordinate that is not finite at a vertex NO row names is not an edge's end: valid
    lone = np.concatenate([xyz, np.full((1, 3), np.nan, np.float32)])
    got = G.geodesic(V + 1, np.append(seeds, -1), edges=edges, xyz=lone, device=DEV)
    _same(got, (np.append(want_len[0], INF), np.append(want_len[1], -1).astype(np.int32)))
    # what the module refuses itself goes to the library directly
    w3 = xyz[:, :3]
    for kw, text in ((dict(V=0), "vertices"), (dict(V=-5), "vertices"), (dict(E=-1), "edge rows"), (dict(xyz=w3, stride=2), "at least 3"),
                     (dict(xyz=w3, stride=0), "at least 3"), (dict(xyz=w3, weights=lens), "at most one"), (dict(max_dist=-1e-9), "max_dist"),
                     (dict(max_dist=float("nan")), "max_dist"), (dict(max_dist=-INF), "max_dist"), (dict(null=("edges",)), "null"),
                     (dict(null=("seed",)), "null"), (dict(null=("dist",)), "null"), (dict(null=("owner",)), "null"), (dict(null=("ws",)), "null"),
                     (dict(ws_bytes=256), "workspace"), (dict(ws_bytes=0), "workspace")):
        kw.setdefault("V", V)
        rc, msg = _raw(edges, seeds=seeds, **kw)
        assert rc == hip.SG_EINVAL and "sg_graph_geodesic" in msg and text in msg, (kw, rc, msg)
        valid()
    rc, msg = _raw(edges, V, seeds, xyz=w3)
    assert rc == 0, msg
    rc, msg = _raw(edges[:0], V, seeds, null=("edges",))                        # E = 0 needs no edge pointer
    assert rc == 0, msg
    got = G.geodesic(V, seeds, edges=edges[:0], device=DEV)
    assert np.array_equal(got.owner, np.where(seeds >= 0, np.arange(V), -1)) and np.array_equal(got.dist, np.where(seeds >= 0, 0.0, INF))
    assert G.last_stats() == dict(arcs=0, distance_launches=0, owner_launches=0, tight_arcs=0, reached=2)
    none = G.geodesic(V, np.full(V, -1), edges=edges, xyz=xyz, device=DEV)
    assert np.isinf(none.dist).all() and (none.owner == -1).all() and G.last_stats()["reached"] == 0


def test_limits_are_refused_without_a_launch():
    """SG_EUNSUP comes from the host checks, before anything is read on the device: the buffers here are one element long"""
    from seggroup_amd import geodesic as G
    from seggroup_amd import hip
    one = np.zeros((1, 2), np.int32)
    for kw, text in ((dict(V=(1 << 27) + 1), "at most"), (dict(V=1, E=(1 << 26) + 1), "2^26")):
        rc, msg = _raw(one, seeds=np.zeros(1, np.int32), **kw)
        assert rc == hip.SG_EUNSUP and "sg_graph_geodesic" in msg and text in msg, (kw, rc, msg)
        _same(G.geodesic(1, [0], edges=one, device=DEV), (np.zeros(1), np.zeros(1, np.int32)))
        _same(G.geodesic(2, [-1, 5], edges=np.array([[1, 0]]), device=DEV), (np.array([1.0, 0.0]), np.array([1, 1], np.int32)))


def test_snap_to_segments_on_the_device():
    from seggroup_amd import geodesic as G
    seg = np.array([7, 7, 7, 2, 2, 5, 5, 5, 8, 8])
    lab = np.array([9, 9, 4, 9, 4, 4, -1, -1, -1, 9])
    snapped, moved = G.snap_to_segments(seg, lab, device=DEV)
    assert snapped.tolist() == [9, 9, 9, 4, 4, -1, -1, -1, 9, 9] and moved == 0.4


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def test_the_baseline_on_a_u_shaped_strip(tmp_path):
    """A U-shaped strip of 206 vertices, 0.01 apart along it: vertex k = 0..100 runs DOWN the left arm from its tip (0, 0, 1) to (0, 0, 0),
    k = 101..104 crosses the bottom, k = 105..205 runs UP the right arm from (0.05, 0, 0) to its tip (0.05, 0, 1): two arms 1 long and
    0.05 apart.  Its graph is the path, written as `prepare` writes a face-less scan's (a vertex-only PLY, adj.pth).  Two clicks: k = 0,
    the tip of the left arm, instance 1 (a chair, 5), and k = 135, 0.3 up the right arm, instance 2 (a table, 7).
    ALONG the strip vertex k is 0.01 k from the first click and 0.01 |k - 135| from the second: k <= 67 goes to the first (68 vertices),
    k >= 68 to the second (138); the farthest vertex is the right tip, 0.70 from the second click.
    IN SPACE the left arm at height z is nearer the second click once 0.0025 + (z - 0.3)^2 < (1 - z)^2, z < 0.648: k = 36..100; the right
    arm is nearer the FIRST click for z > 0.652: k = 171..205.  So the Euclidean nearest click disagrees on k = 36..67 and 171..205:
    32 + 35 = 67 of the 206 vertices.
    The real labels: instance 1 is k <= 102, instance 2 the rest, so the baseline is wrong on k = 68..102 and nowhere else."""
    import torch
    from seggroup_amd import evaluate, geodesic as G, labels
    scene = "scene0031_00"
    z = np.arange(101) * 0.01
    xyz = np.concatenate([np.stack([np.zeros(101), np.zeros(101), z[::-1]], 1), np.stack([np.arange(1, 5) * 0.01, np.zeros(4), np.zeros(4)], 1),
                          np.stack([np.full(101, 0.05), np.zeros(101), z], 1)]).astype(np.float32)
    V = 206
    assert xyz.shape == (V, 3) and xyz[0].tolist() == [0, 0, 1] and np.allclose(xyz[135], [0.05, 0, 0.3]) and np.allclose(xyz[205], [0.05, 0, 1])
    clicks = np.array([0, 135])
    ins_weak, sem_weak = np.full(V, -1), np.full(V, -1)
    ins_weak[clicks], sem_weak[clicks] = (1, 2), (5, 7)
    k = np.arange(V)
    want_ins, want_sem = np.where(k <= 67, 1, 2), np.where(k <= 67, 5, 7)
    real_ins, real_sem = np.where(k <= 102, 1, 2), np.where(k <= 102, 5, 7)
    d = np.linalg.norm(xyz[:, None, :].astype(np.float64) - xyz[clicks][None].astype(np.float64), axis=2)
    euclid = np.array([1, 2])[d.argmin(1)]
    assert np.flatnonzero(euclid != want_ins).tolist() == list(range(36, 68)) + list(range(171, 206)) and (euclid != want_ins).sum() == 67
    root, scans_dir, out = str(tmp_path / "root"), str(tmp_path / "scans"), str(tmp_path / "out")
    os.makedirs(os.path.join(scans_dir, scene))
    P.write_vertex_only_ply(os.path.join(scans_dir, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))
    os.makedirs(os.path.join(root, "adj", "mesh", "raw", scene))
    torch.save(torch.from_numpy(R.path(V).astype(np.int64)), os.path.join(root, "adj", "mesh", "raw", scene, scene + ".adj.pth"))
    for style, ins, sem in (("seg/clicks", ins_weak, sem_weak), ("real", real_ins, real_sem)):
        labels._write_txt(os.path.join(root, "label", style, "raw", scene, scene + ".ins.txt"), ins)
        labels._write_txt(os.path.join(root, "label", style, "raw", scene, scene + ".sem.txt"), sem)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    argv = ["--scans", scans_dir, "--root", root, "--label_style", "clicks", "--out", out, "--score", "--style-name", "geo", "--workers", "1"]
    r = subprocess.run([sys.executable, "-m", "seggroup_amd.geodesic"] + argv, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    # every vertex took the label of the click nearest ALONG the strip
    with np.load(os.path.join(out, scene + G.NPZ_SUFFIX)) as f:
        assert sorted(f.files) == ["dist", "ins", "owner", "sem"]
        assert np.array_equal(f["ins"], want_ins) and np.array_equal(f["sem"], want_sem) and np.array_equal(f["owner"], np.where(k <= 67, 0, 135))
        dist, _ = R.geodesic(V, ins_weak, R.path(V), xyz=xyz)
        assert f["dist"].tobytes() == dist.tobytes() and abs(dist.max() - 0.70) < 1e-6 and dist.argmax() == 205
    geo = os.path.join(root, "label", "seg", "geo", "raw", scene)
    assert labels.load_labels(os.path.join(geo, scene + ".ins.txt")) == want_ins.tolist()
    assert labels.load_labels(os.path.join(geo, scene + ".sem.txt")) == want_sem.tolist()
    doc = json.load(open(os.path.join(out, G.REPORT_NAME)))
    entry = doc["scenes"][scene]
    assert doc["parameters"] == dict(label_style="clicks", metric="length", snap=False, style_name="geo", score=True) and doc["skipped"] == []
    assert (entry["vertices"], entry["seeds"], entry["reached"], entry["unreached"]) == (206, 2, 206, 0) and entry["largest_distance"] == float(dist.max())
    assert entry["distance_launches"] >= 1 and entry["owner_launches"] >= 1 and entry["resampled"].startswith("not written")
    # the printed accuracy is the one evaluate.eval_vectors gives for those vectors
    gt = np.stack([real_sem, real_ins], 1).astype(np.int32)
    m = evaluate.eval_vectors(gt, {"final": (want_ins.astype(np.int32), want_sem.astype(np.int32))}, ["final"], torch.device(DEV))
    assert entry["accuracy"]["ins"] == float(m[0, 161]) and entry["accuracy"]["sem"] == float(m[0, 160]) and doc["score"]["scenes"] == 1
    acc = evaluate.accumulate([m], ["final"])["final"]
    assert np.array_equal(np.asarray(doc["score"]["v"]), acc.v, equal_nan=True)          # a class without vertices is NaN in both
    printed = re.search(r"Instance Acc: ([0-9.]+)%\s+Semantic Acc: ([0-9.]+)%", r.stdout)
    assert printed and printed.group(1) == "%.2f" % (acc.summary()["acc_ins"] * 100) and printed.group(2) == "%.2f" % (acc.summary()["acc_sem"] * 100)
    assert "AP_50%" in r.stdout
    # a second run writes nothing without --force
    r = subprocess.run([sys.executable, "-m", "seggroup_amd.geodesic"] + argv, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "0 written, 1 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
