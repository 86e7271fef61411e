"""The segment graph on the GPU: sg_segment_graph BIT-EQUAL to the NumPy statement (tests/seggraph_ref.py) at the sort's and
the scans' tile edges, for every number of radix passes and on every shape of rows; against sg_contract_point_edges; the same bytes on two
streams; the device's refusals; the workspace guard; `generate_weak_labels(seg_graph="scan")` against the capture of the reference and
on a face-less scan, where the dense default clicks nearly every segment; `python -m seggroup_amd.prepare` in a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ops_ref
import seggraph_ref as G
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
ISENT = -77


def _call(adj, seg, S, stream=None, V=None):
    """the C entry point on exactly its workspace, outputs pre-filled: -> (rc, pairs, cross); nothing outside P rows and the workspace is
    written"""
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    adj = np.ascontiguousarray(np.asarray(adj, np.int64).reshape(-1, 2))
    E = adj.shape[0]
    with torch.cuda.stream(stream):
        d_adj = torch.from_numpy(adj if E else np.zeros((1, 2), np.int64)).to("cuda:0")
        d_seg = torch.from_numpy(np.ascontiguousarray(seg, dtype=np.int32)).to("cuda:0")
        d_pairs = torch.full((max(E, 1) + 16, 2), ISENT, dtype=torch.int32, device="cuda:0")
        d_cross = torch.full((max(E, 1) + 16,), ISENT, dtype=torch.int32, device="cuda:0")
        nbytes = int(lib.sg_segment_graph_ws_bytes(E, S))
        ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
        n_p = C.c_longlong(-5)
        torch.cuda.current_stream().synchronize()
        rc = lib.sg_segment_graph(d_adj.data_ptr(), E, d_seg.data_ptr(), int(d_seg.shape[0]) if V is None else V, S, d_pairs.data_ptr(),
                                  d_cross.data_ptr(), C.byref(n_p), ws.data_ptr(), nbytes, None if stream is None else stream.cuda_stream)
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all().item()), "sg_segment_graph wrote past its workspace"
        h_pairs, h_cross = d_pairs.cpu().numpy(), d_cross.cpu().numpy()
    if rc < 0:
        assert n_p.value == 0 and (h_pairs == ISENT).all() and (h_cross == ISENT).all(), "a refused call leaves no output"
        return rc, None, None
    P = int(n_p.value)
    assert 0 <= P <= E and (h_pairs[P:] == ISENT).all() and (h_cross[P:] == ISENT).all(), "wrote past pair %d" % P
    return rc, h_pairs[:P], h_cross[:P]


def _same(got, want, what):
    assert got[0] == 0, what
    for g, w, name in zip(got[1:], want, ("pairs", "cross")):
        assert g.dtype == np.int32 and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {name}"


@pytest.mark.parametrize("E", G.E_SIZES)
def test_bit_equal_at_every_tile_edge(E):
    for S in (3, 1024, 1 << 20):                                  # 32-bit keys of one pass and of two, 64-bit keys of four
        adj, seg = G.size_case(E, S)
        _same(_call(adj, seg, S), G.segment_graph(adj, seg, S), f"E = {E}, S = {S}")


@pytest.mark.parametrize("S", G.S_SIZES)
def test_bit_equal_for_every_number_of_key_bits(S):
    for E in (4097, 12289):
        adj, seg = G.size_case(E, S, seed=1)
        want = G.segment_graph(adj, seg, S)
        _same(_call(adj, seg, S), want, f"E = {E}, S = {S}")
        assert (want[0].shape[0] == 0) == (S == 1)
        if S > 1:
            assert want[0][0, 0] == 0 and want[0][:, 1].max() == S - 1, "the highest key bit is in use"


@pytest.mark.parametrize("shape", G.SHAPES)
def test_bit_equal_on_every_shape(shape):
    from seggroup_amd import seggraph
    adj, seg, S = G.shape_case(shape)
    want = G.segment_graph(adj, seg, S)
    _same(_call(adj, seg, S), want, shape)
    pairs, cross = seggraph.segment_graph(adj, seg, device="cuda:0") if seg.max() == S - 1 else seggraph.segment_graph(adj, seg, S, device="cuda:0")
    assert pairs.tobytes() == want[0].tobytes() and cross.tobytes() == want[1].tobytes() and pairs.dtype == cross.dtype == np.int32
    if shape == "one_pair":
        assert cross.tolist() == [adj.shape[0]]
    if shape == "inside":
        assert pairs.shape == (0, 2) and cross.shape == (0,)


def test_python_form_takes_no_rows_and_tensors():
    import torch
    from seggroup_amd import seggraph
    pairs, cross = seggraph.segment_graph(np.zeros((0, 2), np.int64), np.array([0, 1, 2]), device="cuda:0")
    assert pairs.shape == (0, 2) and cross.shape == (0,) and pairs.dtype == np.int32
    adj, seg, S = G.shape_case("mesh")
    want = G.segment_graph(adj, seg, S)
    st = torch.cuda.Stream(device="cuda:0")
    pairs, cross = seggraph.segment_graph(torch.from_numpy(adj).to("cuda:0"), torch.from_numpy(seg), S, device="cuda:0", stream=st)
    assert np.array_equal(pairs, want[0]) and np.array_equal(cross, want[1])
    with pytest.raises(ValueError):
        seggraph.segment_graph(np.zeros((4, 3), np.int64), seg, device="cuda:0")


def test_pair_list_equals_the_bitmap_contraction():
    """sg_contract_point_edges keeps one bit per pair (S <= 46,340): the same rows, where it reaches"""
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    for S in (181, 2900):
        adj, seg, N = ops_ref.contract_case(S)
        adj = adj[((adj >= 0) & (adj < N)).all(axis=1)]
        rc, pairs, cross = _call(adj, seg, S)
        d_adj, d_seg = torch.from_numpy(adj).to("cuda:0"), torch.from_numpy(seg).to("cuda:0")
        cap = adj.shape[0]
        out = torch.empty((cap, 2), dtype=torch.int32, device="cuda:0")
        cnt = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        ws = torch.empty(int(lib.sg_contract_ws_bytes(S)), dtype=torch.uint8, device="cuda:0")
        hip.check(lib.sg_contract_point_edges(d_adj.data_ptr(), adj.shape[0], d_seg.data_ptr(), N, S, out.data_ptr(), cap, cnt.data_ptr(),
                                              ws.data_ptr(), ws.numel(), None))
        torch.cuda.synchronize()
        n = int(cnt[0].item())
        assert rc == 0 and n == pairs.shape[0] and np.array_equal(out[:n].cpu().numpy(), pairs), S
        assert int(cross.sum()) == int((seg[adj[:, 0]] != seg[adj[:, 1]])[(seg[adj] >= 0).all(axis=1)].sum())


def test_same_bytes_on_two_streams():
    import torch
    adj, seg, S = G.shape_case("shuffled")
    big_adj, big_seg = G.size_case(12289, 2049, seed=3)
    first = _call(adj, seg, S), _call(big_adj, big_seg, 2049)
    for st in (torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")):
        again = _call(adj, seg, S, stream=st), _call(big_adj, big_seg, 2049, stream=st)
        for a, b in zip(first, again):
            assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_device_refusals():
    from seggroup_amd import hip, seggraph
    lib = hip.lib()
    adj, seg, S = G.shape_case("mesh")
    V = seg.shape[0]
    for where in (0, adj.shape[0] - 1):
        for col in (0, 1):
            for bad in (-1, V, 2 ** 40):
                x = adj.copy()
                x[where, col] = bad
                assert _call(x, seg, S)[0] == hip.SG_EINVAL
                assert b"a vertex index is outside 0..%d" % (V - 1) in lib.sg_last_error()
    for where in (0, V - 1):
        for bad in (S, 2 ** 31 - 1):
            s = seg.copy()
            s[where] = bad
            assert _call(adj, s, S)[0] == hip.SG_EINVAL
            assert b"a segment number is outside 0..%d" % (S - 1) in lib.sg_last_error()
    with pytest.raises(hip.SgError) as ei:
        seggraph.segment_graph(adj, seg, S - 1, device="cuda:0")
    assert ei.value.code == hip.SG_EINVAL and "segment number" in str(ei.value)
    # the scan is shorter than its rows say: V is the bound, not the length of the array
    assert _call(adj, seg, S, V=V - 1)[0] == hip.SG_EINVAL
    _same(_call(adj, seg, S), G.segment_graph(adj, seg, S), "and the next call is a call like any other")


# ---- simulated clicks from the scan's own graph ------------------------------------------------------------------------------------------------
def _scan_dir(td, scan, ann, faces=None):
    import capture_labels as cl
    from seggroup_amd import prepare
    scene_path = cl.write_inputs(td, scan, ann)
    prepare.write_ply(os.path.join(scene_path, scan.name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces if faces is None else faces)
    return scene_path


def _label_files(root, style_dir, name):
    from seggroup_amd import labels
    raw = os.path.join(root, "label", "seg", style_dir, "raw", name)
    return (np.array(labels.load_labels(os.path.join(raw, name + ".ins.txt"))), np.array(labels.load_labels(os.path.join(raw, name + ".sem.txt"))))


@pytest.fixture(scope="module")
def captured(tmp_path_factory):
    """the scan of tools/capture_labels.py, prepared up to its adjacency files"""
    import capture_labels as cl
    from seggroup_amd import prepare, synthetic
    fx = cl.FIXTURE
    scan = synthetic.make_raw_scan(fx["w"], fx["h"], fx["seed"], name=fx["name"], cell=fx["cell"])
    ann = synthetic.make_annotations(scan, 11, blocks_per_row=-(-fx["w"] // fx["cell"]))
    td = str(tmp_path_factory.mktemp("captured"))
    scene_path = _scan_dir(td, scan, ann)
    assert prepare.prepare_scene(scene_path, 5, fx["num_points"], root=td, perm=scan.perm, device="cuda:0") is None
    return td, scene_path, scan


@pytest.mark.parametrize("style,kw", [("manual", {}), ("maxseg", {}), ("maxseg", {"anno_num": 2}), ("rand", {}), ("mainseg", {"main_num": 3})])
def test_scan_graph_clicks_match_the_capture(captured, style, kw):
    import torch
    import capture_labels as cl
    from seggroup_amd import prepare
    td, scene_path, scan = captured
    fx = cl.FIXTURE
    g = np.load(os.path.join(GOLDEN, "prep_labels.npz"))
    d = cl.style_dir(style, kw)
    ret = prepare.prepare_scene(scene_path, 5, fx["num_points"], root=td, perm=scan.perm, device="cuda:0", label_style=style,
                                manual_label_path=os.path.join(td, "manual"), seg_graph="scan", rng=np.random.RandomState(1), **kw)
    assert list(ret) == g[f"{d}.ret"].tolist()
    ins, sem = _label_files(td, d, scan.name)
    assert np.array_equal(ins, g[f"{d}.ins"]) and np.array_equal(sem, g[f"{d}.sem"])
    t = torch.load(os.path.join(td, "label", "seg", d, "resampled", scan.name, scan.name + ".label.pth"))
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), g[f"{d}.label_pth"])


def test_faceless_scan_is_clicked_over_its_point_graph(tmp_path):
    """a 60 x 40 lattice scan without its faces: the kNN-10 graph stands in for the mesh.  The dense matrix of no faces is all zeros, every
    segment its own cluster, every segment of 100 vertices clicked; the scan's graph gives one click per connected part."""
    import torch
    from seggroup_amd import labels, prepare, synthetic
    scan = synthetic.make_raw_scan(60, 40, 33, name="cloud0033_00", cell=10)
    ann = synthetic.make_annotations(scan, 11, blocks_per_row=6)
    td = str(tmp_path)
    scene_path = _scan_dir(td, scan, ann, faces=np.zeros((0, 3), np.int32))
    dense = prepare.prepare_scene(scene_path, 0, 2000, root=td, perm=scan.perm, device="cuda:0", label_style="maxseg")
    dense_files = _label_files(td, "maxseg", scan.name)
    got = prepare.prepare_scene(scene_path, 0, 2000, root=td, perm=scan.perm, device="cuda:0", label_style="maxseg", seg_graph="scan")
    got_files = _label_files(td, "maxseg", scan.name)
    raw = os.path.join(td, "label", "real", "raw", scan.name)
    seg = np.array(labels.load_labels(os.path.join(raw, scan.name + ".seg.txt")))
    adj = torch.load(os.path.join(td, "adj", "mesh", "raw", scan.name, scan.name + ".adj.pth")).numpy()
    assert adj.shape[0] > 5 * scan.xyz.shape[0], "the kNN-10 graph of the points"
    want = labels.generate_weak_labels(scene_path, None, label_style="maxseg", root=td, seg_graph=G.segment_graph(adj, seg))
    want_files = _label_files(td, "maxseg", scan.name)
    assert got == want and all(np.array_equal(a, b) for a, b in zip(got_files, want_files))
    assert got[3:] == dense[3:] and got[1] == dense[1]
    print("clicked segments: dense", dense[2], "scan graph", got[2], "of", got[3], "segments in", got[4], "instances")
    assert got[4] <= got[2] < dense[2], "fewer clicks than one per segment: that is the gap"
    assert (got_files[0] != -1).sum() < (dense_files[0] != -1).sum()


def _tree_bytes(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dirpath, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_command_over_three_scans(tmp_path):
    from seggroup_amd import prepare, synthetic
    data = str(tmp_path / "scannet")
    scans_ = {}
    for i, (w, h, faceless) in enumerate(((60, 40, False), (48, 40, False), (60, 40, True))):
        scan = synthetic.make_raw_scan(w, h, 50 + i, name=f"scene{i:04d}_00", cell=10)
        ann = synthetic.make_annotations(scan, 11 + i, blocks_per_row=-(-w // 10))
        _scan_dir(data, scan, ann, faces=np.zeros((0, 3), np.int32) if faceless else None)
        scans_[scan.name] = scan
    os.makedirs(os.path.join(data, "scans", "not_a_scan"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = {}
    for workers in (1, 3):
        out = str(tmp_path / f"out{workers}")
        cmd = [sys.executable, "-m", "seggroup_amd.prepare", "--data_root", data, "--root", out, "--num_points", "2000", "--label_style", "rand",
               "--seed", "4", "--workers", str(workers)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        outs[workers] = (out, r.stdout)
    a, b = _tree_bytes(outs[1][0]), _tree_bytes(outs[3][0])
    assert sorted(a) == sorted(b)
    assert [k for k in a if a[k] != b[k]] == [], "the tree depends on --workers"
    # the lines and the report against the counts
    out, stdout = outs[3]
    doc = json.load(open(os.path.join(out, prepare.REPORT_NAME)))
    names = sorted(scans_)
    assert sorted(doc["scenes"]) == names and doc["label_style"] == "rand" and doc["seg_graph"] == "scan" and doc["seed"] == 4
    lines = stdout.splitlines()
    for i, name in enumerate(names):
        assert "[%04d/3] Dealing with %s..." % (i, name) in lines and "[%04d/3] Finish %s!" % (i, name) in lines
    rets = [tuple(doc["scenes"][n][k] for k in ("labeled_points", "points", "labeled_segments", "segments", "instances")) for n in names]
    tail = [ln for ln in lines if ln.startswith("Average")]
    assert tail == prepare.summary_lines(rets, 3) and lines[-2] == "Finish all!"
    for name, ret in zip(names, rets):
        assert ret[1] == scans_[name].xyz.shape[0] and ret[4] <= ret[2] <= ret[3]
    # one mesh directly: the same draws, the same files
    name = names[1]
    direct = str(tmp_path / "direct")
    rng = prepare.scene_rng(4, name)
    perm = rng.permutation(scans_[name].xyz.shape[0])
    ret = prepare.prepare_scene(os.path.join(data, "scans", name), 1, 2000, root=direct, perm=perm, device="cuda:0", label_style="rand",
                                seg_graph="scan", rng=rng)
    assert tuple(ret) == rets[1]
    d = _tree_bytes(direct)
    assert len(d) == 14 and len(a) == 3 * len(d) + 1 and all(a[k] == v for k, v in d.items()), [k for k, v in d.items() if a.get(k) != v]
