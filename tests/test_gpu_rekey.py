"""Re-keying annotations on the GPU: sg_segment_vote BIT-EQUAL to the NumPy statement (tests/rekey_ref.py) at the sort's
and the scans' tile edges and on every shape of rows and columns; its refusals; determinism across streams; whole scans against that
statement, against the source tree's label files and against what the reference's own scripts made of the tree
(tests/golden/rekey_expected.json); a re-keyed scan through prepare_scene -> pack -> SegModel.forward; the command line in a child
process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rekey_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 12289]      # the sort's tile is 4,096 keys, the scans' 2,048; three tiles and one
FIELDS = ("row_ids", "row_count", "winner", "winner_count", "distinct", "tied", "first_vertex", "rank", "vertex_winner")


def _shapes(v):
    """name -> (row ids, columns, n_cols) for V vertices"""
    rng = np.random.default_rng(1000 + v)
    some = np.unique(rng.integers(0, 2 ** 31, max(v // 9, 1)))
    out = {
        "random ids below 2^31": (some[rng.integers(0, some.shape[0], v)], rng.integers(0, 5, v), 5),
        "one row holds everything": (np.full(v, 2 ** 31 - 1), rng.integers(0, 3, v), 3),
        "every vertex its own row": (rng.permutation(v) * 3 + 1, rng.integers(0, 4, v), 4),
        "one column": (some[rng.integers(0, some.shape[0], v)], np.zeros(v, np.int64), 1),
        "two columns": (rng.integers(0, max(v // 50, 1), v), rng.integers(0, 2, v), 2),
        "as many columns as vertices": (rng.integers(0, max(v // 7, 1), v) * 5, rng.permutation(v), v),
        "one row, every column once": (np.full(v, 7), rng.permutation(v), v),
    }
    # rows in which two and three columns tie: row r holds t(r) columns (from a random start) the same number of times, and a loser once
    reps = 3
    rows, cols = [], []
    r = 0
    while len(rows) + 10 <= v:
        t, start = 2 + r % 2, int(rng.integers(0, 6))
        for j in range(t):
            rows += [r * 11] * reps
            cols += [(start + 2 * j) % 9] * reps
        rows.append(r * 11)
        cols.append((start + 1) % 9)
        r += 1
    if rows:
        pad = v - len(rows)
        rows, cols = np.array(rows + [10 ** 9] * pad), np.array(cols + [8] * pad)
        order = rng.permutation(v)
        out["two and three columns tie"] = (rows[order], cols[order], 9)
    return out


@pytest.mark.parametrize("v", SIZES)
def test_vote_is_bit_equal_to_the_statement(v):
    from seggroup_amd import rekey
    for name, (ids, cols, n_cols) in _shapes(v).items():
        want = R.vote(ids, cols, n_cols)
        got = rekey.vote(ids, cols, n_cols, device="cuda:0").host()
        for f in FIELDS:
            g = getattr(got, f)
            assert g.dtype == np.int32 and g.tobytes() == want[f].tobytes(), f"V = {v}, {name}: {f}"
        if name == "two and three columns tie":
            assert want["tied"].sum() >= max((v - 10) // 10, 1) and (want["distinct"] >= 3).any()
        rank, row_ids, row_count = rekey.rank_ids(ids, device="cuda:0")
        assert np.array_equal(rank.cpu().numpy(), want["rank"]) and np.array_equal(row_ids.cpu().numpy(), want["row_ids"])
        assert np.array_equal(row_count.cpu().numpy(), want["row_count"])


def test_wide_keys_take_the_64_bit_path():
    """rows x columns needs more than 32 key bits: 4,097 distinct rows (13 bits) and n_cols = 2^31 - 1 (31 bits)"""
    from seggroup_amd import rekey
    v = 4097 + 60
    rng = np.random.default_rng(5)
    ids = np.concatenate([np.arange(4097) * 5, rng.integers(0, 40, 60) * 5])
    cols = np.concatenate([rng.integers(0, 2 ** 31 - 1, 4097), np.full(60, 2 ** 31 - 2)])
    order = rng.permutation(v)
    want = R.vote(ids[order], cols[order], 2 ** 31 - 1)
    got = rekey.vote(ids[order], cols[order], 2 ** 31 - 1, device="cuda:0").host()
    for f in FIELDS:
        assert getattr(got, f).tobytes() == want[f].tobytes(), f
    assert want["tied"].sum() > 0 and want["winner"].max() == 2 ** 31 - 2


def test_bad_ids_and_columns_are_refused_by_the_device_check():
    import ctypes as C
    import torch
    from seggroup_amd import hip, rekey
    ids, cols = np.arange(5000) % 37, np.arange(5000) % 6
    for where in (0, 4999):
        for bad in (-1, -2 ** 31):
            x = ids.copy()
            x[where] = bad
            with pytest.raises(hip.SgError) as ei:
                rekey.vote(x, cols, 6, device="cuda:0")
            assert ei.value.code == hip.SG_EINVAL and "negative" in str(ei.value)
            with pytest.raises(hip.SgError) as ei:
                rekey.rank_ids(x, device="cuda:0")
            assert ei.value.code == hip.SG_EINVAL and "negative" in str(ei.value)
        for bad in (6, -1, 2 ** 31 - 1):
            c = cols.copy()
            c[where] = bad
            with pytest.raises(hip.SgError) as ei:
                rekey.vote(ids, c, 6, device="cuda:0")
            assert ei.value.code == hip.SG_EINVAL and "outside 0..5" in str(ei.value)
    with pytest.raises(ValueError):
        rekey.vote(ids, cols[:-1], 6, device="cuda:0")
    with pytest.raises(ValueError):
        rekey.vote(ids, cols, 0, device="cuda:0")
    with pytest.raises(ValueError):
        rekey.vote(ids.astype(np.float32), cols, 6, device="cuda:0")
    # the workspace is the caller's: too small a one is refused, not overrun
    lib = hip.lib()
    d = torch.zeros((11, 5000), dtype=torch.int32, device="cuda:0")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    n_r = C.c_int(0)
    assert lib.sg_segment_vote(d[0].data_ptr(), d[1].data_ptr(), 5000, 6, *[d[2 + i].data_ptr() for i in range(9)], C.byref(n_r), ws.data_ptr(),
                               ws.numel(), None) == hip.SG_ENOMEM
    assert b"workspace too small" in lib.sg_last_error()


def test_two_runs_on_two_streams_give_identical_bytes():
    import torch
    from seggroup_amd import rekey
    for name, (ids, cols, n_cols) in _shapes(12289).items():
        a = rekey.vote(ids, cols, n_cols, device="cuda:0", stream=torch.cuda.Stream(device="cuda:0")).host()
        b = rekey.vote(ids, cols, n_cols, device="cuda:0", stream=torch.cuda.Stream(device="cuda:0")).host()
        for f in FIELDS:
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (name, f)


# ---- whole scans ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_case():
    scan, ann = R.source_scan()
    return scan, ann, R.clicks_with_points(scan, ann), json.load(open(os.path.join(GOLDEN, "rekey_expected.json")))


def _source_tree(root, scan, ann, manual):
    from seggroup_amd import prepare
    sp = R.write_tree(root, scan, ann["tsv"], scan.seg_indices, dict(aggregation=ann["aggregation"], manual=manual))
    prepare.write_ply(os.path.join(sp, scan.name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
    return sp


def _same_as_statement(res, ref):
    for f in FIELDS:
        assert getattr(res.new_vote, f).tobytes() == ref["vote"][f].tobytes(), f
    assert res.aggregation == ref["aggregation"] and res.manual == ref["manual"] and res.clicks == ref["clicks"]
    assert res.report == ref["report"]


@pytest.mark.parametrize("which", R.SEGMENTATIONS)
def test_scan_rekeyed_onto_another_segmentation(scan_case, which, tmp_path):
    from seggroup_amd import labels, prepare, rekey
    from seggroup_amd.synthetic import _CATEGORIES
    scan, ann, manual, exp = scan_case
    new = R.new_segmentation(scan, which)
    ref = R.rekey(scan.seg_indices, new, ann["aggregation"], manual, scan.name)
    res = rekey.rekey_arrays(scan.seg_indices, new, ann["aggregation"], manual, scene_name=scan.name, device="cuda:0")
    _same_as_statement(res, ref)
    assert res.report == exp[which]["report"]
    ins, sem = rekey.vertex_labels(res, dict(_CATEGORIES))
    assert R.digest(ins) == exp[which]["real.ins"] and R.digest(sem) == exp[which]["real.sem"]
    if which == "cell14":                                          # the bare-list click file that make_annotations writes
        plain = rekey.rekey_arrays(scan.seg_indices, new, ann["aggregation"], ann["manual"], scene_name=scan.name, device="cuda:0")
        _same_as_statement(plain, R.rekey(scan.seg_indices, new, ann["aggregation"], ann["manual"], scan.name))
    # the files: rekey_scan over the source tree, read by the project's producers
    src_root, out = str(tmp_path / "src"), str(tmp_path / "out")
    sp = _source_tree(src_root, scan, ann, manual)
    report = rekey.rekey_scan(sp, out, new, manual_label_path=os.path.join(src_root, "manual_label"), device="cuda:0")
    assert report == ref["report"]
    osp = os.path.join(out, "scans", scan.name)
    assert sorted(os.listdir(osp)) == sorted([scan.name + ".aggregation.json", scan.name + rekey.SEGS_SUFFIX, scan.name + "_vh_clean_2.ply"])
    assert os.path.islink(os.path.join(osp, scan.name + "_vh_clean_2.ply"))
    assert sorted(os.listdir(out)) == ["manual_label", "scannetv2-labels.combined.tsv", "scans"]
    assert json.load(open(os.path.join(osp, scan.name + ".aggregation.json"))) == ref["aggregation"]
    assert json.load(open(os.path.join(out, "manual_label", scan.name + ".json"))) == ref["manual"]
    assert prepare.load_seg_labels(os.path.join(osp, scan.name + rekey.SEGS_SUFFIX)) == new.tolist()
    prepare.prepare_scene(osp, 0, 2000, root=out, perm=scan.perm, device="cuda:0", label_style="manual",
                          manual_label_path=os.path.join(out, "manual_label"))
    ret = {"manual": None, "maxseg": None}
    for style in ret:
        ret[style] = labels.generate_weak_labels(osp, None, label_style=style, manual_label_path=os.path.join(out, "manual_label"), root=out)
        assert list(ret[style]) == exp[which][f"{style}.ret"], style
        for k in ("ins", "sem"):
            got = np.array(labels.load_labels(os.path.join(out, "label", "seg", style, "raw", scan.name, f"{scan.name}.{k}.txt")))
            assert R.digest(got) == exp[which][f"{style}.{k}"], (style, k)
    raw = os.path.join(out, "label", "real", "raw", scan.name)
    real = {k: open(os.path.join(raw, f"{scan.name}.{k}.txt"), "rb").read() for k in ("ins", "sem")}
    for k in ("ins", "sem"):
        assert R.digest(np.array(real[k].split(), dtype=np.int64)) == exp[which][f"real.{k}"], k
    if which in ("identity", "refine"):                            # byte-identical to the label files of the source tree
        labels.generate_real_labels(sp, root=src_root)
        for k in ("ins", "sem"):
            assert open(os.path.join(src_root, "label", "real", "raw", scan.name, f"{scan.name}.{k}.txt"), "rb").read() == real[k], k
    # a second run refuses, force overwrites, copy_mesh copies
    with pytest.raises(FileExistsError):
        rekey.rekey_scan(sp, out, new, device="cuda:0")
    if which == "cell5":
        assert rekey.rekey_scan(sp, out, new, manual_label_path=os.path.join(src_root, "manual_label"), force=True, copy_mesh=True,
                                device="cuda:0") == ref["report"]
        mesh = os.path.join(osp, scan.name + "_vh_clean_2.ply")
        assert not os.path.islink(mesh) and open(mesh, "rb").read() == open(os.path.join(sp, scan.name + "_vh_clean_2.ply"), "rb").read()
        assert not [f for _, _, fs in os.walk(out) for f in fs if ".tmp." in f], "the temporary names are gone"


def test_all_four_label_styles_read_the_rekeyed_tree(scan_case, tmp_path):
    """the tree rekey_scan wrote, once per label style: every style finds its inputs and labels vertices.  manual, maxseg and rand go
    through prepare_scene; mainseg takes main_num, which prepare_scene does not pass on, so its two producers are called as
    prepare_weak_label.py calls them"""
    import torch
    from seggroup_amd import labels, prepare, rekey
    scan, ann, manual, _ = scan_case
    src_root, out = str(tmp_path / "src"), str(tmp_path / "out")
    sp = _source_tree(src_root, scan, ann, manual)
    rekey.rekey_scan(sp, out, R.new_segmentation(scan, "cell14"), manual_label_path=os.path.join(src_root, "manual_label"), device="cuda:0")
    osp = os.path.join(out, "scans", scan.name)
    for style in ("manual", "maxseg", "rand", "mainseg_3"):
        np.random.seed(1)
        if style == "mainseg_3":
            labels.generate_weak_labels(osp, None, label_style="mainseg", main_num=3, root=out)
            labels.generate_weak_label_pth(scan.name, style, root=out)
        else:
            prepare.prepare_scene(osp, 0, 2000, root=out, perm=scan.perm, device="cuda:0", label_style=style,
                                  manual_label_path=os.path.join(out, "manual_label"))
        weak = torch.load(os.path.join(out, "label", "seg", style, "resampled", scan.name, scan.name + ".label.pth")).numpy()
        assert weak.shape == (2000, 2) and (weak[:, 1] >= 0).any() and (weak[:, 1] < 0).any(), style
        assert ((weak[:, 0] >= 0) == (weak[:, 1] >= 0)).all(), style


def test_lattice_of_80k_vertices():
    """several blocks in every kernel: 320 x 250 vertices, 7 x 7 source blocks, re-keyed onto 10 x 10 blocks and onto single vertices"""
    from seggroup_amd import rekey, synthetic
    scan = synthetic.make_raw_scan(320, 250, 9, name="scene0009_00", cell=7, dup_frac=0.0, degenerate_faces=0)
    ann = synthetic.make_annotations(scan, 3, blocks_per_row=-(-320 // 7))
    other = synthetic.make_raw_scan(320, 250, 9, name="scene0009_00", cell=10, dup_frac=0.0, degenerate_faces=0)
    assert scan.xyz.shape[0] == 80000
    for new in (other.seg_indices, np.arange(80000)[::-1] * 2):
        ref = R.rekey(scan.seg_indices, new, ann["aggregation"], ann["manual"], scan.name)
        res = rekey.rekey_arrays(scan.seg_indices, new, ann["aggregation"], ann["manual"], scene_name=scan.name, device="cuda:0")
        _same_as_statement(res, ref)
        sv = R.vote(scan.seg_indices, ref["vote"]["rank"], ref["vote"]["row_ids"].shape[0])
        for f in FIELDS:
            assert getattr(res.src_vote, f).tobytes() == sv[f].tobytes(), f
    assert ref["report"]["new_segments"] == 80000 and ref["report"]["unchanged"] == 80000


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _room_tree(root, name, w, h, seed):
    """a make_room_scan mesh carrying annotations: the source segmentation cuts the floor, the wall and the box into a left and a right
    half; the floor is one object, the wall's halves are two, the box is one; four clicks, one of them with its raw vertex"""
    from seggroup_amd import prepare, synthetic
    room = synthetic.make_room_scan(w, h, seed, jitter=1e-3, name=name)
    part = (np.asarray(room.seg_indices, dtype=np.int64) - 3) // 7                      # 0 floor, 1 wall, 2 box
    right = (np.arange(w * h) % w) >= w // 2
    seg = ((part * 2 + right) * 7 + 3).astype(np.int32)
    scan = synthetic.RawScan(name, room.xyz, room.rgb, room.faces, seg, room.perm)
    sid = lambda p, r: int((p * 2 + r) * 7 + 3)
    groups = [dict(id=0, objectId=0, segments=[sid(0, 0), sid(0, 1)], label="floor"), dict(id=1, objectId=1, segments=[sid(1, 0)], label="wall"),
              dict(id=2, objectId=2, segments=[sid(1, 1)], label="wall"), dict(id=3, objectId=3, segments=[sid(2, 0), sid(2, 1)], label="table")]
    manual = {"1": [sid(0, 0)], "2": [sid(1, 0)], "3": {str(sid(1, 1)): int(np.nonzero(seg == sid(1, 1))[0][5])}, "4": [sid(2, 1)]}
    ann = dict(aggregation={"sceneId": name, "segGroups": groups}, manual=manual, tsv=synthetic.make_annotations(scan, 0, blocks_per_row=3)["tsv"])
    sp = R.write_tree(root, scan, ann["tsv"], seg, dict(aggregation=ann["aggregation"], manual=ann["manual"]))
    prepare.write_ply(os.path.join(sp, name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
    return scan, ann


def test_rekeyed_scan_reaches_the_forward(tmp_path, weight_sets):
    """a scan segmented here at kThresh 0.05, its annotations carried over -> prepare_scene with the click files and with maxseg -> pack
    -> SegModel.forward returns labels"""
    import overseg_ref
    from seggroup_amd import cache, prepare, rekey
    from seggroup_amd.model import SegModel
    src_root = str(tmp_path / "src")
    scan, ann = _room_tree(src_root, "scene0031_00", 72, 60, 31)
    v = scan.xyz.shape[0]
    for style in ("manual", "maxseg"):
        root = str(tmp_path / style)
        base = os.path.join(root, "dataset", "scannet")
        report = rekey.rekey_scan(os.path.join(src_root, "scans", scan.name), base, k_thresh=0.05, seg_min_verts=20,
                                  manual_label_path=os.path.join(src_root, "manual_label"), device="cuda:0")
        osp = os.path.join(base, "scans", scan.name)
        doc = json.load(open(os.path.join(osp, scan.name + rekey.SEGS_SUFFIX)))
        want = overseg_ref.segment_mesh(scan.xyz, scan.faces, 0.05, 20)
        assert doc["params"] == {"kThresh": "0.050000", "segMinVerts": "20"} and np.array_equal(np.asarray(doc["segIndices"], np.int32), want)
        ref = R.rekey(scan.seg_indices, want, ann["aggregation"], ann["manual"], scan.name)
        assert report == ref["report"] and report["annotated_after"] > 0 and report["clicks"]["total"] > 0
        n = 2500
        prepare.prepare_scene(osp, 0, n, root=base, perm=scan.perm, device="cuda:0", label_style=style,
                              manual_label_path=os.path.join(base, "manual_label"))
        ds = cache.load_pack(cache.pack_scene(root, scan.name, label_style=style), device="cuda:0")
        assert (ds.N, ds.V) == (n, v)
        net = SegModel(exp_name="t", ins_infer=True, data_root=root)
        net.load_weights(weight_sets["ins_infer"])
        net.epoch = "ins_infer"
        res = net.forward_scene(ds, write=False)
        assert len(res.labels) == 14 and all(l.shape == (v,) for l in res.labels)
        assert (res.labels[12] >= 0).any(), "labelled vertices come back"


def test_command_line_in_a_child_process(tmp_path):
    from seggroup_amd import rekey
    src_root = str(tmp_path / "src")
    cases = {}
    for i, (w, h) in enumerate(((60, 50), (72, 40), (48, 48))):
        cases[f"scene{i:04d}_00"] = _room_tree(src_root, f"scene{i:04d}_00", w, h, 40 + i)
    os.makedirs(os.path.join(src_root, "scans", "not_a_scan"))
    out = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "seggroup_amd.rekey", "--scans", os.path.join(src_root, "scans"), "--out", out, "--k-thresh", "0.05",
           "--seg-min-verts", "10", "--manual_label_path", os.path.join(src_root, "manual_label"), "--workers", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines] == sorted(cases) + ["total of 3 scenes"]
    doc = json.load(open(os.path.join(out, "rekey_report.json")))
    import overseg_ref
    for rep, (name, (scan, ann)) in zip(doc["scenes"], sorted(cases.items())):
        new = overseg_ref.segment_mesh(scan.xyz, scan.faces, 0.05, 10)
        assert rep == R.rekey(scan.seg_indices, new, ann["aggregation"], ann["manual"], name)["report"], name
        assert json.load(open(os.path.join(out, "scans", name, name + rekey.SEGS_SUFFIX)))["params"] == {"kThresh": "0.050000", "segMinVerts": "10"}
    assert doc["total"]["V"] == sum(c[0].xyz.shape[0] for c in cases.values()) and doc["total"]["scenes"] == 3
    # again: nothing is overwritten; --new-segs-from takes files as they are, byte for byte
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "exists (force=True overwrites)" in r.stderr
    out2 = str(tmp_path / "out2")
    cmd2 = [sys.executable, "-m", "seggroup_amd.rekey", "--scans", os.path.join(src_root, "scans"), "--out", out2, "--new-segs-from",
            os.path.join(out, "scans"), "--report", str(tmp_path / "r2.json")]
    r = subprocess.run(cmd2, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    for name in cases:
        a, b = (os.path.join(o, "scans", name, name + rekey.SEGS_SUFFIX) for o in (out, out2))
        assert open(a, "rb").read() == open(b, "rb").read()
    d2 = json.load(open(str(tmp_path / "r2.json")))
    assert not os.path.exists(os.path.join(out2, "rekey_report.json")) and not os.path.exists(os.path.join(out2, "manual_label"))
    strip = lambda rep: {k: v for k, v in rep.items() if k != "clicks"}
    assert [strip(x) for x in doc["scenes"]] == d2["scenes"]
