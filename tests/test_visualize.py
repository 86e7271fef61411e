"""Label visualisation without a GPU: the yardstick (tests/visualize_ref.py) against the colours captured from the reference, the public
surface of seggroup_amd.visualize, and the host entry points (PLY plan, PLY writer job, label dilation).  The host-only tests also run
against the sanitizer build: tools/run_asan_host_tests.sh tests/test_visualize.py."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import visualize_ref as ref

INDEX, ARRAYS = ref.load_cases()
CASES = INDEX["cases"]


def _case_id(c):
    src = c.get("labels") or c["ins"]
    return "%s-%s-%s%s" % (c["fn"], c.get("label_type", "grouping"), src.get("array") or src["golden"] + "." + src["key"],
                           "-shuffled" if c["shuffle"] else "")


# ---- the yardstick itself (passes without the feature: it checks what the GPU tests compare against) ------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) + "-%d" % i for i, c in enumerate(CASES)])
def test_restatement_equals_reference_capture(case):
    got = ref.colours(ref.case_indices(case, ARRAYS), INDEX["colors"])
    want = ARRAYS[case["colours"]]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), "%d of %d vertices differ" % (int((got != want).any(1).sum()), got.shape[0])


def test_capture_covers_the_corners():
    seg = ARRAYS["hand.seg_wrap"]
    assert (seg == -1).any() and (seg == 0).any() and np.unique(seg).shape[0] > 41
    assert np.unique(ref.case_vector(dict(golden="small_20k", key="ins.label.layer_1.seg"), ARRAYS)).shape[0] > 40
    assert {1, 2} <= set(ARRAYS["hand.ins_sem"].tolist())
    assert set(range(-1, 41)) <= set(ARRAYS["hand.sem_all"].tolist())
    lab, adj = ARRAYS["hand.adj_labels"], ARRAYS["hand.adj_pairs"]
    assert lab.shape[0] <= 4000
    labelled = set(np.nonzero(lab != -1)[0].tolist())
    nb = {}
    for a, b in adj:
        nb.setdefault(int(a), set()).add(int(b))
        nb.setdefault(int(b), set()).add(int(a))
    shared = [(i, j) for i in labelled for j in labelled if i < j and lab[i] != lab[j] and nb.get(i, set()) & nb.get(j, set())]
    assert shared, "no two labelled vertices with different labels share a neighbour"
    assert {(c["shuffle"], c["seed"]) for c in CASES if c["fn"] == "grouping"} == {(False, 0), (True, 0), (True, 3)}


# ---- public surface ---------------------------------------------------------------------------------------------------------------------
def test_palette_and_signatures_match_the_reference():
    from seggroup_amd import visualize
    assert [list(c) for c in visualize.colors] == INDEX["colors"]
    assert visualize.num_colors == INDEX["num_colors"] == 40
    for name, params in INDEX["signatures"].items():
        sig = inspect.signature(getattr(visualize, name))
        got = [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.default is not inspect.Parameter.empty]
               for p in sig.parameters.values()]
        assert got == params, name
        assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())


def test_output_path_is_the_reference_choice():
    from seggroup_amd import visualize
    for c in CASES:
        assert visualize.output_path(os.path.join("results", "exp", "scene0000_00", "epoch_1", c["label_file"])) == \
            os.path.join("results", "exp", "scene0000_00", "epoch_1", c["output"])


def test_shuffle_positions_follow_the_global_generator():
    import random
    from seggroup_amd import visualize
    random.seed(11)
    d = list(range(100, 137))
    random.shuffle(d)
    random.seed(11)
    pos = visualize.draw_positions(37)
    assert [d.index(100 + k) for k in range(37)] == pos.tolist()
    assert visualize.draw_positions(0).shape == (0,)


def test_scene_generators_depend_on_seed_scene_and_layer_only():
    from seggroup_amd import hip, visualize
    a, b = visualize.scene_generators(1, "scene0000_00"), visualize.scene_generators(1, "scene0000_00")
    assert [g is not None for g in a] == [n in ("layer_2.seg", "layer_3.seg", "layer_4.seg") for n in hip.LABEL_NAMES]
    draws = lambda gs: [g.random() for g in gs if g is not None]        # noqa: E731
    da = draws(a)
    assert da == draws(b) and len(set(da)) == 3
    assert da != draws(visualize.scene_generators(2, "scene0000_00")) and da != draws(visualize.scene_generators(1, "scene0001_00"))


@pytest.mark.parametrize("module", ["seggroup_amd.infer", "seggroup_amd.train"])
def test_drivers_honour_v(module):
    r = subprocess.run([sys.executable, "-m", module, "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "(ignored)" not in r.stdout
    assert "--mesh_root" in r.stdout and "--visualize" in r.stdout


def test_segmodel_takes_mesh_root_and_fails_before_gpu_work_without_a_mesh(tmp_path):
    from seggroup_amd.model import SegModel
    sig = inspect.signature(SegModel.__init__)
    assert list(sig.parameters)[1:6] == ["exp_name", "cuda", "visualize", "sem_infer", "ins_infer"]
    assert sig.parameters["mesh_root"].default == "/data1/antao/Documents/Datasets/ScanNet_raw"
    net = SegModel(exp_name="x", visualize=True, ins_infer=True, data_root=str(tmp_path), mesh_root=str(tmp_path / "raw"))

    class _Scene:
        name, V = "scene0000_00", 10
    with pytest.raises(FileNotFoundError):
        net.forward_scene(_Scene())


# ---- sg_ply_plan ----------------------------------------------------------------------------------------------------------------------------
def _plan(sg_lib, path):
    from seggroup_amd import hip
    plan = (C.c_longlong * 10)()
    rc = sg_lib.sg_ply_plan(os.fsencode(str(path)), plan)
    return rc, list(plan), (sg_lib.sg_last_error() or b"").decode() if rc != hip.SG_OK else ""


def _mesh(n=50, f=30, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, n, (f, 3)).astype(np.int32)


def test_ply_plan_of_a_scannet_shaped_file(sg_lib, tmp_path):
    from seggroup_amd import prepare
    xyz, rgb, faces = _mesh()
    p = tmp_path / "a.ply"
    prepare.write_ply(str(p), xyz, rgb, faces)
    rc, plan, _ = _plan(sg_lib, p)
    assert rc == 0
    size = os.path.getsize(p)
    hdr = open(p, "rb").read().index(b"end_header\n") + len(b"end_header\n")
    assert plan == [hdr, 50, 16, 12, 13, 14, hdr + 50 * 16, size - hdr - 50 * 16, size, hdr]
    assert plan[7] == 30 * 13


def test_ply_plan_with_comment_normals_and_another_property_order(sg_lib, tmp_path):
    n = 7
    rec = np.dtype([("blue", "u1"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<i2"), ("ny", "<i2"), ("nz", "<i2"), ("alpha", "u1"),
                    ("red", "u1"), ("quality", "<f8"), ("green", "u1")])
    hdr = ("ply\r\nformat binary_little_endian 1.0\ncomment made by a test\nobj_info x\nelement vertex %d\nproperty uchar blue\nproperty float x\n"
           "property float32 y\nproperty float z\nproperty short nx\nproperty int16 ny\nproperty short nz\nproperty uint8 alpha\nproperty uchar red\n"
           "property double quality\nproperty uchar green\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n" % n).encode()
    p = tmp_path / "b.ply"
    tail = b"\x03" + np.arange(3, dtype="<i4").tobytes() + b"\x03" + np.arange(3, dtype="<i4").tobytes()
    p.write_bytes(hdr + np.zeros(n, rec).tobytes() + tail)
    rc, plan, msg = _plan(sg_lib, p)
    assert rc == 0, msg
    assert rec.itemsize == 30
    assert plan[:8] == [len(hdr), n, 30, rec.fields["red"][1], rec.fields["green"][1], rec.fields["blue"][1], len(hdr) + n * 30, len(tail)]


def test_ply_plan_with_an_element_in_front_of_the_vertices(sg_lib, tmp_path):
    hdr = (b"ply\nformat binary_little_endian 1.0\nelement camera 2\nproperty float fx\nproperty double fy\nelement vertex 3\nproperty float x\n"
           b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    p = tmp_path / "c.ply"
    p.write_bytes(hdr + bytes(2 * 12) + bytes(3 * 7))
    rc, plan, msg = _plan(sg_lib, p)
    assert rc == 0, msg
    assert plan[:8] == [len(hdr) + 24, 3, 7, 4, 5, 6, len(hdr) + 24 + 21, 0] and plan[9] == len(hdr)


_GOOD = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
         "property uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n")
MALFORMED = {
    "truncated_header": _GOOD[:_GOOD.index("property uchar blue")].encode(),
    "ascii": _GOOD.replace("binary_little_endian", "ascii").encode() + b"0 0 0 1 2 3 255\n" * 4,
    "big_endian": _GOOD.replace("binary_little_endian", "binary_big_endian").encode() + bytes(64),
    "list_in_vertex": _GOOD.replace("property uchar alpha\n", "property list uchar int extra\n").encode() + bytes(64),
    "ushort_colour": _GOOD.replace("property uchar green", "property ushort green").encode() + bytes(68),
    "count_beyond_file": _GOOD.replace("element vertex 4", "element vertex 400000").encode() + bytes(64),
    "count_overflows": _GOOD.replace("element vertex 4", "element vertex 99999999999999999999999").encode() + bytes(64),
    "no_red": _GOOD.replace("property uchar red", "property uchar r").encode() + bytes(64),
    "not_ply": b"plx\n" + _GOOD[4:].encode() + bytes(64),
    "huge_leading_element": _GOOD.replace("element vertex 4", "element pad 1099511627776\nproperty double a\nelement vertex 4").encode() + bytes(64),
    "empty": b"",
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_ply_plan_rejects_malformed_files(sg_lib, tmp_path, name):
    from seggroup_amd import hip, visualize
    p = tmp_path / (name + ".ply")
    p.write_bytes(MALFORMED[name])
    rc, plan, msg = _plan(sg_lib, p)
    assert rc == hip.SG_EINVAL and msg, (rc, msg)
    assert plan == [0] * 10
    with pytest.raises(ValueError):
        visualize.ply_plan(str(p))


def test_ply_plan_of_a_missing_file(sg_lib, tmp_path):
    from seggroup_amd import hip
    assert _plan(sg_lib, tmp_path / "nothing.ply")[0] == hip.SG_EINVAL
    assert sg_lib.sg_ply_plan(None, None) == hip.SG_EINVAL


# ---- sg_writer_submit_ply ---------------------------------------------------------------------------------------------------------------
def test_writer_job_writes_head_block_tail(sg_lib, tmp_path):
    from seggroup_amd import prepare, visualize
    xyz, rgb, faces = _mesh(200, 120, seed=5)
    src_path = tmp_path / "scene_vh_clean_2.ply"
    prepare.write_ply(str(src_path), xyz, rgb, faces)
    src = visualize.read_source(str(src_path))
    assert (src.V, src.stride, src.offsets) == (200, 16, (12, 13, 14))
    new_rgb = np.random.default_rng(6).integers(0, 256, (3, 200, 3)).astype(np.uint8)
    blocks = np.stack([ref.patched_block(src.block, 16, src.offsets, c) for c in new_rgb])
    out_dir = tmp_path / "results" / "epoch_1"
    out_dir.mkdir(parents=True)
    paths = [str(out_dir / "visualize" / ("layer_%d.seg.ply" % i)) for i in range(3)]
    w = sg_lib.sg_writer_create(2, 8)
    try:
        visualize.write_plys(src, blocks, paths, writer=w, tag=0)
    finally:
        sg_lib.sg_writer_destroy(w)
    assert sorted(os.listdir(out_dir / "visualize")) == ["layer_0.seg.ply", "layer_1.seg.ply", "layer_2.seg.ply"]    # no temporary left
    raw = open(src_path, "rb").read()
    for i, p in enumerate(paths):
        got = open(p, "rb").read()
        assert len(got) == len(raw)
        assert got[:len(src.head)] == raw[:len(src.head)] and got[len(raw) - len(src.tail):] == raw[len(raw) - len(src.tail):]
        m = prepare.read_ply(p)
        gx, gc, gf = prepare.mesh_arrays(m)
        assert gx.tobytes() == xyz.tobytes() and np.array_equal(gf, faces)
        assert np.array_equal(gc, new_rgb[i])
        assert (np.asarray(m["vertex"]["alpha"]) == 255).all()


def test_writer_job_reports_an_unwritable_directory(sg_lib, tmp_path):
    from seggroup_amd import hip
    w = sg_lib.sg_writer_create(1, 4)
    try:
        blob = b"abc"
        assert sg_lib.sg_writer_submit_ply(w, os.fsencode(str(tmp_path / "no" / "such" / "visualize" / "x.ply")), blob, 3, blob, 3, None, 0, -1) == 0
        assert sg_lib.sg_writer_flush(w) == hip.SG_EINVAL
        assert sg_lib.sg_writer_submit_ply(w, None, blob, 3, blob, 3, None, 0, -1) == hip.SG_EINVAL
        assert sg_lib.sg_writer_submit_ply(w, b"x.ply", None, 3, blob, 3, None, 0, -1) == hip.SG_EINVAL
    finally:
        sg_lib.sg_writer_destroy(w)


def test_plydata_source_is_the_file_write_ply_writes(tmp_path):
    from seggroup_amd import prepare, visualize
    xyz, rgb, faces = _mesh(33, 9, seed=8)
    p = tmp_path / "m.ply"
    prepare.write_ply(str(p), xyz, rgb, faces)
    a, b = visualize.read_source(str(p)), visualize.source_from_plydata(prepare.read_ply(str(p)))
    assert (a.head, a.tail, a.stride, a.offsets) == (b.head, b.tail, b.stride, b.offsets) and np.array_equal(a.block, b.block)


# ---- sg_dilate_labels -------------------------------------------------------------------------------------------------------------------
def test_dilate_equals_the_restatement_and_the_capture(sg_lib):
    from seggroup_amd import visualize
    lab, adj = ARRAYS["hand.adj_labels"], ARRAYS["hand.adj_pairs"]
    got = visualize.dilate_labels(lab, adj)
    assert got.dtype == np.int32 and np.array_equal(got, ref.dilate(lab, adj))
    assert (got != lab).sum() > 100 and np.array_equal(lab, ARRAYS["hand.adj_labels"])         # the input is not touched
    case = next(c for c in CASES if c.get("adj") and c["label_type"] == "instance")
    assert np.array_equal(ref.colours(ref.colour_indices(got, "instance"), INDEX["colors"]), ARRAYS[case["colours"]])
    # order dependence: a chain 0 - 1 - 2 with labels (5, 7, -1): 0 hands 5 to 1, then 1 hands the 5 it holds by then on to 0 and 2
    # (handing on the value it STARTED with would give [7, 5, 7])
    assert visualize.dilate_labels(np.array([5, 7, -1]), np.array([[0, 1], [1, 2]])).tolist() == [5, 5, 5]
    # (-1, 7, 5): 1 hands 7 to 0 and 2, then 2 -- a source since the start -- hands the 7 it holds by then back to 1
    assert visualize.dilate_labels(np.array([-1, 7, 5]), np.array([[0, 1], [1, 2]])).tolist() == [7, 7, 7]
    # a vertex that only BECOMES labelled is no source: (-1, -1, 4) on the chain leaves vertex 0 alone
    assert visualize.dilate_labels(np.array([-1, -1, 4]), np.array([[0, 1], [1, 2]])).tolist() == [-1, 4, 4]
    assert visualize.dilate_labels(np.array([3, -1]), np.zeros((0, 2), np.int64)).tolist() == [3, -1]


def test_dilate_rejects_a_bad_csr(sg_lib):
    from seggroup_amd import hip, visualize
    lab = np.zeros(3, np.int32)
    ok_ptr = np.array([0, 1, 2, 2], np.int64)
    for ptr, idx in ((np.array([0, 2, 1, 2], np.int64), np.array([1, 0], np.int32)), (ok_ptr, np.array([1, 3], np.int32)),
                     (ok_ptr, np.array([1, -1], np.int32)), (np.array([1, 1, 2, 2], np.int64), np.array([1, 0], np.int32))):
        assert sg_lib.sg_dilate_labels(lab.ctypes.data, 3, ptr.ctypes.data, idx.ctypes.data) == hip.SG_EINVAL
    with pytest.raises(ValueError):
        visualize.dilate_labels(lab, np.array([[0, 3]]))
