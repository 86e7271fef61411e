"""Label visualisation on the GPU against the colours captured from the reference (tests/golden/visualize_*) and the NumPy restatement
pinned to them (tests/visualize_ref.py): the vector form through the two public functions, the table form against the vector form, the
PLY record kernel (16-byte and generic records, single and batched), SegModel(visualize=True) and the inference driver's -v."""
import hashlib
import os
import random
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, make_fixture_scene
import visualize_ref as ref

pytestmark = pytest.mark.gpu

INDEX, ARRAYS = ref.load_cases()
CASES = INDEX["cases"]
PALETTE = np.asarray(INDEX["colors"], dtype=np.uint8)


def _write_mesh(path, V, seed=1, faces=40):
    from seggroup_amd import prepare
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((V, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (V, 3)).astype(np.uint8)
    fc = rng.integers(0, V, (faces, 3)).astype(np.int32)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    prepare.write_ply(path, xyz, rgb, fc)
    return xyz, rgb, fc


def _read_colours(path, xyz, fc):
    """The colours of a written mesh; everything else must be the source's, bit for bit."""
    from seggroup_amd import prepare
    gx, gc, gf = prepare.mesh_arrays(prepare.read_ply(path))
    assert gx.tobytes() == xyz.tobytes() and np.array_equal(gf, fc)
    return gc


# ---- vector form, through the reference's two functions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=["%03d-%s-%s" % (i, c["fn"], c.get("label_type", "grouping")) for i, c in enumerate(CASES)])
def test_public_functions_equal_reference_capture(tmp_path, ci):
    import torch
    from seggroup_amd import visualize
    c = CASES[ci]
    want = ARRAYS[c["colours"]]
    V = want.shape[0]
    d = tmp_path / "results" / "scene0000_00" / "epoch_1"
    d.mkdir(parents=True)
    mesh = str(tmp_path / "raw" / "scene0000_00_vh_clean_2.ply")
    xyz, _, fc = _write_mesh(mesh, V, seed=ci)

    def put(name, vec, npy=False):
        p = str(d / name)
        if npy:
            p = p[:-4] + ".npy"
            np.save(p, np.asarray(vec, dtype=np.int32))
        else:
            with open(p, "w") as f:
                f.write("".join("%d\n" % v for v in vec))
        return p
    if c["fn"] == "labels":
        label_file = put(c["label_file"], ref.case_vector(c["labels"], ARRAYS), npy=ci % 3 == 1)
        sem = put("sem_for_ins.txt", ref.case_vector(c["sem"], ARRAYS)) if "sem" in c else None
        adj = None
        if "adj" in c:
            adj = str(d / "adj.pth")
            torch.save(torch.from_numpy(np.asarray(ARRAYS[c["adj"]], dtype=np.int64)), adj)
        if "random_seed" in c:
            random.seed(c["random_seed"])
        out = visualize.visualize_labels(mesh, label_file, c["label_type"], shuffle=c["shuffle"], adj_path=adj, sem_labels=sem)
    else:
        ins = put("grouping.ins.txt", ref.case_vector(c["ins"], ARRAYS))
        seg = put("grouping.seg.txt", ref.case_vector(c["seg"], ARRAYS))
        out = visualize.visualize_grouping_process(mesh, ins, seg, shuffle=c["shuffle"], seed=c["seed"])
    assert out == str(d / c["output"])
    assert os.listdir(d / "visualize") == [os.path.basename(c["output"])]
    got = _read_colours(out, xyz, fc)
    assert np.array_equal(got, want), "%d of %d vertices differ" % (int((got != want).any(1).sum()), V)


def test_vector_form_errors_and_edges(tmp_path):
    import torch
    from seggroup_amd import hip, visualize
    with pytest.raises(ValueError):                                  # a semantic label without a colour (the reference raises IndexError)
        visualize.colour_vector(np.array([1, 41, 2], np.int32), "semantic")
    with pytest.raises(ValueError):                                  # grouping: no vertex with instance label -1
        visualize.colour_vector(np.array([3, 4], np.int32), hip.COLOUR_GROUPING, second=np.array([1, 2], np.int32))
    # negative labels other than -1 keep Python's modulo; one vertex; all vertices equal
    lab = np.array([-5, -2, 0, 1, 40, 41, 81, -1, 2**31 - 1, -2**31], np.int32)
    got = visualize.colour_vector(lab, "instance").cpu().numpy()
    assert np.array_equal(got, ref.colour_indices(lab, "instance"))
    got = visualize.colour_vector(lab, "segment").cpu().numpy()
    assert np.array_equal(got, ref.colour_indices(lab, "segment"))
    assert visualize.colour_vector(np.array([7], np.int32), "segment").cpu().tolist() == [1]
    assert visualize.colour_vector(np.full(1000, -1, np.int32), "segment", shuffle=True).cpu().sum().item() == 0
    mesh = str(tmp_path / "m.ply")
    _write_mesh(mesh, 10)
    np.save(str(tmp_path / "short.npy"), np.zeros(9, np.int32))
    with pytest.raises(ValueError):                                  # label count != vertex count (the reference exits)
        visualize.visualize_labels(mesh, str(tmp_path / "short.npy"), "semantic")
    assert not os.path.exists(tmp_path / "visualize")
    assert torch.cuda.is_available()


# ---- table form ---------------------------------------------------------------------------------------------------------------------------
def _table_against_vector(tables, sov, seed):
    """Every row's colours through the table form equal the vector form (and the restatement) on the expanded vector, for both widths of
    seg_of_vertex; segment rows plain and shuffled."""
    import torch
    from seggroup_amd import hip, visualize
    tables = np.ascontiguousarray(tables, dtype=np.int32)
    sov = np.ascontiguousarray(sov, dtype=np.int32)
    nvec, S = tables.shape
    types = visualize.VECTOR_TYPES[:nvec]
    expanded = np.where(sov[None, :] >= 0, tables[:, np.clip(sov, 0, S - 1)], -1).astype(np.int32)
    d_tab = torch.from_numpy(tables).cuda()
    sov16 = torch.from_numpy(np.where(sov < 0, 0xFFFF, sov).astype(np.uint16).view(np.int16)).cuda()
    slot = np.where(sov >= 0, sov, S)
    for shuffle_all in (False, True):
        shuffled = [shuffle_all and t == hip.COLOUR_SEGMENT for t in types]
        for width, d_sov in ((4, torch.from_numpy(sov).cuda()), (2, sov16)):
            random.seed(seed)
            cidx = visualize.colour_tables(d_tab, d_sov, types, shuffled, sov_width=width).cpu().numpy()
            assert cidx.shape == (nvec, S + 1) and cidx.max() <= 40
            random.seed(seed)
            for r in range(nvec):
                name = {hip.COLOUR_SEGMENT: "segment", hip.COLOUR_INSTANCE: "instance", hip.COLOUR_SEMANTIC: "semantic"}[types[r]]
                state = random.getstate()
                vec = visualize.colour_vector(expanded[r], name, shuffle=shuffled[r]).cpu().numpy()
                random.setstate(state)
                want = ref.colour_indices(expanded[r], name, shuffle=shuffled[r])
                assert np.array_equal(vec, want), (r, width, shuffle_all)
                assert np.array_equal(cidx[r][slot], want), (r, width, shuffle_all)
    return expanded


def test_table_form_constructed_case():
    """One table entry no vertex maps to (its value must not count in the rank), vertices without a segment (their -1 must count)."""
    from seggroup_amd import hip, visualize
    import torch
    rng = np.random.default_rng(4)
    S, V = 90, 3000
    tables = np.stack([rng.integers(0, 70, S) * 5 + 2 if t == hip.COLOUR_SEGMENT else rng.integers(-1, 41, S) for t in visualize.VECTOR_TYPES])
    tables[0, 17] = 1                                              # lower than every other value of row 0: it would shift every rank
    tables[3, 17] = -1                                             # a -1 only at the absent entry
    sov = rng.integers(0, S, V)
    sov[sov == 17] = 18                                            # entry 17 has no vertex
    sov[rng.integers(0, V, 200)] = -1
    _table_against_vector(tables, sov, seed=21)
    # without vertices that lack a segment the -1 does not occur: the lowest occurring value has rank 0
    sov2 = np.where(sov < 0, 3, sov)
    exp = _table_against_vector(tables, sov2, seed=22)
    cidx = visualize.colour_tables(torch.from_numpy(tables.astype(np.int32)).cuda(), torch.from_numpy(sov2.astype(np.int32)).cuda(),
                                   visualize.VECTOR_TYPES, None).cpu().numpy()
    lowest = int(np.unique(exp[0])[0])
    assert cidx[0][np.nonzero(tables[0] == lowest)[0][0]] == 1
    with pytest.raises(ValueError):                                  # an occurring semantic value without a colour
        bad = tables.astype(np.int32).copy()
        bad[2, 5] = 77
        visualize.colour_tables(torch.from_numpy(bad).cuda(), torch.from_numpy(sov2.astype(np.int32)).cuda(), visualize.VECTOR_TYPES, None)
    bad[2, 5], bad[2, 17] = 3, 77                                    # ... but not one no vertex maps to
    visualize.colour_tables(torch.from_numpy(bad).cuda(), torch.from_numpy(sov2.astype(np.int32)).cuda(), visualize.VECTOR_TYPES, None)


@pytest.mark.parametrize("fixture", ["tiny_dup_4k", "scannet_profile"])
def test_table_form_equals_vector_form_on_scenes(golden_index, weight_sets, fixture):
    """Tables and seg_of_vertex of real forwards: V != N with a non-identity unmap (tiny_dup_4k; the ScanNet-shaped synthetic profile)."""
    from seggroup_amd import hip, synthetic
    from seggroup_amd.model import Pipeline
    from seggroup_amd.scene import DeviceScene
    if fixture == "scannet_profile":
        sc = synthetic.make_scene(6000, 60, 90210, seg_profile="scannet")
    else:
        sc = make_fixture_scene(golden_index, fixture)
    assert sc.unmap.shape[0] != sc.data.shape[0] and not np.array_equal(sc.unmap[:10], np.arange(10))
    ds = DeviceScene.from_synthetic(sc, device="cuda:0")
    pipe = Pipeline(weight_sets["ins_infer"], ds.N, ds.S, ds.E0, ds.V, device="cuda:0")
    try:
        res = pipe.forward(ds, hip.MODE_INS_INFER, want_tables=True)
        tab, sov = res.compact()
        exp = _table_against_vector(tab, sov, seed=5)
        assert np.array_equal(exp, res.labels[:14])
        if fixture == "tiny_dup_4k":
            g = load_golden(fixture)
            assert all(np.array_equal(exp[i], g["ins.label." + n]) for i, n in enumerate(hip.LABEL_NAMES))
    finally:
        pipe.close()


# ---- the record kernel ----------------------------------------------------------------------------------------------------------------------
REC16 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
REC16_SWAPPED = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("alpha", "u1"), ("blue", "u1"), ("red", "u1"), ("green", "u1")])
REC27 = np.dtype([("x", "<f4"), ("blue", "u1"), ("y", "<f4"), ("z", "<f4"), ("nx", "<i2"), ("ny", "<i2"), ("nz", "<i2"), ("alpha", "u1"),
                  ("green", "u1"), ("red", "u1"), ("quality", "u1", (5,))])


def _offsets(rec):
    return tuple(rec.fields[k][1] for k in ("red", "green", "blue"))


def _want_rows(block, rec, cidx_rows):
    return np.stack([ref.patched_block(block, rec.itemsize, _offsets(rec), PALETTE[c]) for c in cidx_rows])


@pytest.mark.parametrize("rec", [REC16, REC16_SWAPPED, REC27], ids=["scannet16", "swapped16", "generic27"])
@pytest.mark.parametrize("V", [1, 63, 65, 1000, 5000])
def test_records_equal_source_with_three_bytes_patched(rec, V):
    import torch
    from seggroup_amd import visualize
    assert rec.itemsize in (16, 27)
    rng = np.random.default_rng(V)
    block = rng.integers(0, 256, V * rec.itemsize).astype(np.uint8)
    src = torch.from_numpy(block).cuda()
    for S, nrows in ((37, 14), (12000, 14), (700, 3)):             # table rows in LDS; 14 x 12,001 bytes: beyond the LDS budget; fewer rows
        cidx = rng.integers(0, 41, (14, S + 1)).astype(np.uint8)
        sov = rng.integers(-1, S, V).astype(np.int32)
        rows = list(rng.permutation(14)[:nrows])
        per_vertex = cidx[:, np.where(sov >= 0, sov, S)]
        want = _want_rows(block, rec, per_vertex[rows])
        d_cidx = torch.from_numpy(cidx).cuda()
        for width, d_sov in ((4, torch.from_numpy(sov).cuda()),
                             (2, torch.from_numpy(np.where(sov < 0, 0xFFFF, sov).astype(np.uint16).view(np.int16)).cuda())):
            got = visualize.vertex_records(src, V, rec.itemsize, _offsets(rec), d_cidx, rows, seg_of_vertex=d_sov, S=S, sov_width=width)
            assert np.array_equal(got.cpu().numpy(), want), (S, nrows, width)
        # vector form: the same colours given per vertex
        got = visualize.vertex_records(src, V, rec.itemsize, _offsets(rec), torch.from_numpy(np.ascontiguousarray(per_vertex)).cuda(), rows)
        assert np.array_equal(got.cpu().numpy(), want), (S, nrows, "vector")


@pytest.mark.parametrize("rec", [REC16, REC27], ids=["scannet16", "generic27"])
def test_batched_records_equal_single(rec):
    import ctypes as C
    import torch
    from seggroup_amd import hip, visualize
    lib = hip.lib()
    rng = np.random.default_rng(9)
    Vs, Ss = [1, 63, 65, 1000, 4097, 0, 777], [5, 40, 3, 900, 1500, 7, 64]
    rows = [0, 3, 6, 9, 13, 1]
    stride = rec.itemsize
    al = lambda x: (x + 15) // 16 * 16                                         # noqa: E731
    blocks = [rng.integers(0, 256, V * stride).astype(np.uint8) for V in Vs]
    sovs = [rng.integers(-1, S, V).astype(np.int32) for V, S in zip(Vs, Ss)]
    cidxs = [rng.integers(0, 41, (14, S + 1)).astype(np.uint8) for S in Ss]
    desc, src_off, sov_off, cidx_off, out_off = [], 0, 0, 0, 0
    for V, S in zip(Vs, Ss):
        desc.append([src_off, V, sov_off, S, cidx_off, S + 1, out_off])
        src_off += al(V * stride); sov_off += V; cidx_off += 14 * (S + 1); out_off += al(len(rows) * V * stride)
    src_all = np.zeros(max(src_off, 16), np.uint8)
    for d, b in zip(desc, blocks):
        src_all[d[0]:d[0] + b.size] = b
    d_src, d_sov = torch.from_numpy(src_all).cuda(), torch.from_numpy(np.concatenate(sovs)).cuda()
    d_cidx = torch.from_numpy(np.concatenate([c.reshape(-1) for c in cidxs])).cuda()
    d_desc = torch.from_numpy(np.asarray(desc, dtype=np.int64)).cuda()
    d_out = torch.zeros(max(out_off, 16), dtype=torch.uint8, device="cuda")
    off = _offsets(rec)
    hip.check(lib.sg_ply_vertex_records_device_batch(len(Vs), d_desc.data_ptr(), max(Vs), max(Ss), d_src.data_ptr(), stride, off[0], off[1], off[2],
                                                     d_sov.data_ptr(), 4, d_cidx.data_ptr(), len(rows), (C.c_int * len(rows))(*rows),
                                                     d_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    out = d_out.cpu().numpy()
    for i, (V, S) in enumerate(zip(Vs, Ss)):
        if V == 0:
            continue
        single = visualize.vertex_records(torch.from_numpy(blocks[i]).cuda(), V, stride, off, torch.from_numpy(cidxs[i]).cuda(), rows,
                                          seg_of_vertex=torch.from_numpy(sovs[i]).cuda(), S=S).cpu().numpy()
        got = out[desc[i][6]:desc[i][6] + len(rows) * V * stride].reshape(len(rows), V * stride)
        assert np.array_equal(got, single), i
        assert np.array_equal(single, _want_rows(blocks[i], rec, cidxs[i][rows][:, np.where(sovs[i] >= 0, sovs[i], S)])), i
    # untouched bytes between the scenes' blocks stay zero
    used = np.zeros(out.size, bool)
    for d, V in zip(desc, Vs):
        used[d[6]:d[6] + len(rows) * V * stride] = True
    assert not out[~used].any()


def test_record_arguments_are_checked():
    import ctypes as C
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rows = (C.c_int * 1)(0)
    call = lambda stride, r, g, b, nrows=1, ld=100: lib.sg_ply_vertex_records_device(                                 # noqa: E731
        buf.data_ptr(), 10, stride, r, g, b, None, 4, 0, buf.data_ptr(), ld, nrows, rows, buf.data_ptr(), None)
    assert call(16, 12, 13, 16) == hip.SG_EINVAL       # a colour byte outside the record
    assert call(16, 12, 12, 14) == hip.SG_EINVAL       # two channels on one byte
    assert call(16, 12, 13, 14, nrows=17) == hip.SG_EINVAL
    assert call(16, 12, 13, 14, ld=9) == hip.SG_EINVAL  # a row narrower than the scene


# ---- SegModel(visualize=True) -------------------------------------------------------------------------------------------------------------------
def _digest_dir(d, skip=("visualize",)):
    out = {}
    for f in sorted(os.listdir(d)):
        if f not in skip:
            out[f] = hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest()
    return out


@pytest.mark.parametrize("mode", ["ins_infer", "sem_infer"])
def test_segmodel_visualize_writes_the_reference_set(tmp_path, golden_index, weight_sets, mode):
    from seggroup_amd import hip
    from seggroup_amd.model import SegModel
    from seggroup_amd.scene import DeviceScene
    sc = make_fixture_scene(golden_index, "tiny_4k")
    gold = load_golden("tiny_4k")
    key = "ins" if mode == "ins_infer" else "sem"
    names = hip.LABEL_NAMES[:14 if mode == "ins_infer" else 6]
    mesh_root = str(tmp_path / "raw")
    ds = DeviceScene.from_synthetic(sc, device="cuda:0")
    xyz, _, fc = _write_mesh(os.path.join(mesh_root, "scans", ds.name, ds.name + "_vh_clean_2.ply"), ds.V, seed=2, faces=500)
    runs = {}
    for tag, vis_on, seed in (("plain", False, 5), ("vis", True, 5), ("again", True, 5), ("other", True, 6)):
        net = SegModel(exp_name=tag, visualize=vis_on, data_root=str(tmp_path), mesh_root=mesh_root, **{mode: True})
        net.load_weights(weight_sets[mode])
        net.epoch = mode
        random.seed(seed)
        res = net.forward_scene(ds)
        net.flush()
        runs[tag] = (net.output_root(ds.name), res)
    d_plain, r_plain = runs["plain"]
    d_vis, r_vis = runs["vis"]
    assert not os.path.exists(os.path.join(d_plain, "visualize"))
    # the label files and the metrics do not notice the visualisation
    assert _digest_dir(d_plain) == _digest_dir(d_vis) and len(_digest_dir(d_vis)) == 2 * len(names)
    assert np.array_equal(r_plain.iou_sem, r_vis.iou_sem) and np.array_equal(r_plain.iou_ins, r_vis.iou_ins)
    assert np.array_equal(r_plain.acc, r_vis.acc, equal_nan=True)
    assert sorted(os.listdir(os.path.join(d_vis, "visualize"))) == sorted(n + ".ply" for n in names)
    # every file against the restatement applied to the reference's own label vectors; layers 2, 3, 4 draw their shuffles in this order
    random.seed(5)
    for n in names:
        kind = {"seg": "segment", "ins": "instance", "sem": "semantic"}[n.split(".")[1]]
        want = PALETTE[ref.colour_indices(gold[f"{key}.label.{n}"], kind, shuffle=n in ("layer_2.seg", "layer_3.seg", "layer_4.seg"))]
        got = _read_colours(os.path.join(d_vis, "visualize", n + ".ply"), xyz, fc)
        assert np.array_equal(got, want), n
    # the same scene and seed again: identical bytes; another seed: only the shuffled layers change
    vis_files = lambda tag: _digest_dir(os.path.join(runs[tag][0], "visualize"), skip=())                             # noqa: E731
    assert vis_files("vis") == vis_files("again")
    changed = {f for f in vis_files("vis") if vis_files("vis")[f] != vis_files("other")[f]}
    assert changed == {n + ".ply" for n in names if n in ("layer_2.seg", "layer_3.seg", "layer_4.seg")}


# ---- the inference driver's -v ------------------------------------------------------------------------------------------------------------------
def _vis_rank_worker(rank, world, root, mesh_root, port, exp, q):
    sys.path.insert(0, ROOT)
    from seggroup_amd import infer
    args = infer.build_parser().parse_args(["-n", exp, "--ins_infer", "--root", root, "--backend", "gloo", "--port", str(port), "--batch", "3",
                                            "--inflight", "8", "-j", "2", "-v", "--mesh_root", mesh_root, "--seed", "4"])
    r = infer.run_worker(rank, world, args)
    if rank == 0:
        q.put(int(r["n"]))


def test_driver_visualize_does_not_depend_on_engine_shape_or_ranks(tmp_path, golden_index, weight_sets):
    import torch
    import torch.multiprocessing as mp
    from seggroup_amd import hip, infer, synthetic, weights
    root, mesh_root = str(tmp_path / "tree"), str(tmp_path / "raw")
    scenes = []
    for i in range(7):
        if i == 0:
            e = golden_index["tiny_4k"]
            scenes.append(synthetic.make_scene(e["n"], e["s"], e["seed"], name="scene0000_00", **e["kw"]))
        else:
            scenes.append(synthetic.make_scene(3000 + 401 * i, 30 + 5 * i, 87000 + i, name=f"scene{i:04d}_00",
                                               **({"dup_frac": 0.05, "raw_vertices": 3500 + 401 * i} if i % 3 == 0 else {})))
    synthetic.write_reference_tree(root, scenes)
    names = [s.name for s in scenes]
    meshes = {s.name: _write_mesh(os.path.join(mesh_root, "scans", s.name, s.name + "_vh_clean_2.ply"), s.unmap.shape[0], seed=i, faces=300)
              for i, s in enumerate(scenes)}
    for exp in ("plain", "v1", "v2"):
        ck = os.path.join(root, "checkpoints", exp, "models")
        os.makedirs(ck)
        torch.save({"state_dict": weights.to_full_state_dict(weight_sets["ins_infer"])}, os.path.join(ck, "last.t7"))
    common = ["--ins_infer", "--root", root, "--world-size", "1", "-j", "2", "--seed", "4"]
    infer.run_worker(0, 1, infer.build_parser().parse_args(["-n", "plain", "--batch", "5", "--inflight", "4"] + common))
    with pytest.raises(FileNotFoundError):                           # a missing mesh stops the run before it starts
        infer.run_worker(0, 1, infer.build_parser().parse_args(["-n", "v1", "--batch", "5", "--inflight", "4", "-v", "--mesh_root", root] + common))
    infer.run_worker(0, 1, infer.build_parser().parse_args(["-n", "v1", "--batch", "5", "--inflight", "4", "-v", "--mesh_root", mesh_root] + common))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_vis_rank_worker, args=(r, 2, root, mesh_root, port, "v2", q)) for r in range(2)]
    for p in procs:
        p.start()
    assert q.get(timeout=600) == len(names)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    gold = load_golden("tiny_4k")
    for n in names:
        dirs = {exp: os.path.join(root, "results", exp, n, "ins_infer") for exp in ("plain", "v1", "v2")}
        assert not os.path.exists(os.path.join(dirs["plain"], "visualize"))
        # everything outside visualize/ is what a run without -v writes
        assert _digest_dir(dirs["plain"]) == _digest_dir(dirs["v1"]) == _digest_dir(dirs["v2"]) and len(_digest_dir(dirs["v1"])) == 28
        a, b = _digest_dir(os.path.join(dirs["v1"], "visualize"), skip=()), _digest_dir(os.path.join(dirs["v2"], "visualize"), skip=())
        assert sorted(a) == sorted(nm + ".ply" for nm in hip.LABEL_NAMES)
        assert a == b, (n, [f for f in a if a[f] != b[f]])
        xyz, _, fc = meshes[n]
        src = open(os.path.join(mesh_root, "scans", n, n + "_vh_clean_2.ply"), "rb").read()
        for nm in hip.LABEL_NAMES:
            path = os.path.join(dirs["v1"], "visualize", nm + ".ply")
            assert os.path.getsize(path) == len(src)
            got = _read_colours(path, xyz, fc)
            lab = np.load(os.path.join(dirs["v1"], nm + ".npy"))
            if n == names[0]:
                assert np.array_equal(lab, gold["ins.label." + nm])
            kind = {"seg": "segment", "ins": "instance", "sem": "semantic"}[nm.split(".")[1]]
            if nm in ("layer_2.seg", "layer_3.seg", "layer_4.seg"):
                # the reference's rule (shuffle the distinct labels, colour by position) with the driver's documented generator:
                # random.Random seeded by "<--seed>/<scene>/<vector>", whatever the engine's shape, the batch order or the rank
                d = np.unique(lab).tolist()
                random.Random("4/%s/%s" % (n, nm)).shuffle(d)
                pos = {v: i for i, v in enumerate(d)}
                want = PALETTE[np.array([0 if v == -1 else pos[v] % 40 + 1 for v in lab.tolist()])]
                assert np.array_equal(got, want), (n, nm)
            else:
                assert np.array_equal(got, PALETTE[ref.colour_indices(lab, kind)]), (n, nm)


# ---- the training driver's -v -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_step", [1, 2])
def test_train_driver_visualize(tmp_path, golden_index, per_step):
    """`python -m seggroup_amd.train -v`: every epoch's exported vectors also as meshes under epoch_<n>/visualize/, coloured like the label
    files written beside them; the label files are those of a run without -v (same seed, one epoch: the same parameters throughout)."""
    from seggroup_amd import hip, synthetic, train
    root, mesh_root = str(tmp_path / "tree"), str(tmp_path / "raw")
    scenes = []
    for i, name in enumerate(("tiny_4k", "tiny_dup_4k")):
        e = golden_index[name]
        scenes.append(synthetic.make_scene(e["n"], e["s"], e["seed"], name=f"scene{i:04d}_00", **e["kw"]))
    synthetic.write_reference_tree(root, scenes)
    meshes = {s.name: _write_mesh(os.path.join(mesh_root, "scans", s.name, s.name + "_vh_clean_2.ply"), s.unmap.shape[0], seed=i, faces=100)
              for i, s in enumerate(scenes)}
    common = ["--root", root, "--epochs", "1", "--out-format", "npy", "--lr", "0.0002", "--seed", "3", "--scenes-per-step", str(per_step)]
    for exp, extra in (("plain", []), ("vis", ["-v", "--mesh_root", mesh_root])):
        for d in (f"checkpoints/{exp}/models", f"results/{exp}"):
            os.makedirs(os.path.join(root, d), exist_ok=True)
        r = train.run_worker(0, 1, train.build_parser().parse_args(["-n", exp] + common + extra))
        assert r["scenes"] == 2
    with pytest.raises(FileNotFoundError):
        train.run_worker(0, 1, train.build_parser().parse_args(["-n", "vis"] + common + ["-v", "--mesh_root", root]))
    for s in scenes:
        d_plain, d_vis = (os.path.join(root, "results", exp, s.name, "epoch_last") for exp in ("plain", "vis"))
        assert _digest_dir(d_plain) == _digest_dir(d_vis) and len(_digest_dir(d_vis)) == 14
        assert not os.path.exists(os.path.join(d_plain, "visualize"))
        assert sorted(os.listdir(os.path.join(d_vis, "visualize"))) == sorted(n + ".ply" for n in hip.LABEL_NAMES)
        xyz, _, fc = meshes[s.name]
        for nm in hip.LABEL_NAMES:
            got = _read_colours(os.path.join(d_vis, "visualize", nm + ".ply"), xyz, fc)
            lab = np.load(os.path.join(d_vis, nm + ".npy"))
            kind = {"seg": "segment", "ins": "instance", "sem": "semantic"}[nm.split(".")[1]]
            if nm in ("layer_2.seg", "layer_3.seg", "layer_4.seg"):
                d = np.unique(lab).tolist()
                random.Random("3/%s/%s" % (s.name, nm)).shuffle(d)
                pos = {v: i for i, v in enumerate(d)}
                want = PALETTE[np.array([0 if v == -1 else pos[v] % 40 + 1 for v in lab.tolist()])]
            else:
                want = PALETTE[ref.colour_indices(lab, kind)]
            assert np.array_equal(got, want), (s.name, nm)
