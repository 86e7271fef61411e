"""The point-cloud over-segmenter over the radius graph on the GPU: sg_radius_neighbours_grid, sg_pointcloud_normals_csr,
sg_pcseg_edges_radius and sg_pcseg_scan_radius against the NumPy statement (tests/pcseg_radius_ref.py) and the committed digests
(tests/golden/pcseg_radius_expected.json), bit for bit: the lists, the normals, the lexicographic edges and weights, the sorted order and
the final ids.  Then the cell edges, the capacity protocol, strides, a caller's viewpoint, two streams, the refusals, the Python forms, a
face-less scan of the clumped room through prepare_scene to SegModel.forward, and the command line."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import components_ref as CR
import pcseg_radius_ref as Q
import pcseg_ref as P
import radius_ref as RR
from conftest import GOLDEN, ROOT
from test_gpu_radius import FORCED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_specks = {}


def _expected():
    return json.load(open(os.path.join(GOLDEN, "pcseg_radius_expected.json")))["cases"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype}, the statement has {want.shape} {want.dtype}"
    bad = np.nonzero((_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(1))[0] if got.size else np.zeros(0, np.int64)
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} rows differ, first at {bad[:5]}"


def _run(xyz, radius, cell=None, viewpoint=None, stream=None):
    """every stage the library leaves on the device, as arrays, and the ids"""
    from seggroup_amd import oversegment
    r = oversegment.pointcloud_edges(xyz, radius=radius, cell=cell, viewpoint=viewpoint, device=DEV, stream=stream)
    got = {k: v.cpu().numpy() for k, v in r.items()}
    got["ids"] = oversegment.segment_pointcloud(xyz, radius=radius, cell=cell, viewpoint=viewpoint, device=DEV, stream=stream)
    return got


def _check(got, ref, seg, what):
    """lists, normals, the sorted list and the ids against the statement; the lexicographic list is the sorted one put back in (a, b)
    order -- every edge occurs once -- and the upper halves of the rows"""
    _same_bits(got["indptr"], ref["off"], what + ": off")
    _same_bits(got["indices"], ref["idx"], what + ": idx")
    _same_bits(got["normals"], ref["normals"], what + ": normals")
    _same_bits(got["edges"], ref["edges"], what + ": sorted edges")
    _same_bits(got["w"], ref["w"], what + ": sorted weights")
    lex = np.lexsort((got["edges"][:, 1], got["edges"][:, 0]))
    _same_bits(np.ascontiguousarray(got["edges"][lex]), ref["lex_edges"], what + ": lexicographic edges")
    _same_bits(np.ascontiguousarray(got["w"][lex]), ref["lex_w"], what + ": lexicographic weights")
    _same_bits(Q.edges_of(got["indptr"], got["indices"]), ref["lex_edges"], what + ": the upper halves of the rows")
    _same_bits(got["ids"], seg, what + ": ids")


def _fixture(got, name):
    lex = np.lexsort((got["edges"][:, 1], got["edges"][:, 0]))
    r = dict(off=got["indptr"], idx=got["indices"], normals=got["normals"], lex_edges=got["edges"][lex], lex_w=got["w"][lex], edges=got["edges"],
             w=got["w"])
    exp = _expected()[name]
    for key, val in Q.stage_digests(r, got["ids"]).items():
        assert val == exp[key], f"{name}: {key}"


def _case_test(name):
    xyz, radius, ref, seg = Q.case(name)
    got = _run(xyz, radius)
    _check(got, ref, seg, name)
    _fixture(got, name)


@pytest.mark.parametrize("n", RR.SIZES)
@pytest.mark.parametrize("tag", sorted(RR.LINE_RADII))
def test_lines_with_no_neighbour_a_path_and_one_row_of_everything(n, tag):
    _case_test("line_%d_%s" % (n, tag))


@pytest.mark.parametrize("name", ["two_clumps", "room_j0", "room_j5e-4", "room_j2e-3", "room_dup", "all_equal", "ball_300", "room_20k"])
def test_every_stage_is_bit_equal_to_the_statement(name):
    _case_test(name)
    _, _, ref, _ = Q.case(name)
    if name == "all_equal":
        assert (np.diff(ref["off"]) == 31).all()
    if name == "ball_300":
        assert (np.diff(ref["off"]) == 299).all(), "every row longer than a tile of 256 candidates"


def test_the_clumped_room_comes_apart_into_its_planes():
    """the reason for the feature: 12 points per lattice site, where the kNN graph at k = 10 has no edge out of a clump"""
    _case_test("clumped_room")
    xyz, plane = Q.clumped_room()
    from seggroup_amd import oversegment
    seg = oversegment.segment_pointcloud(xyz, radius=Q.CLUMPED_RADIUS, device=DEV)
    assert np.unique(seg).shape[0] == 16 and P.purity(seg, plane) == 1.0
    knn = oversegment.segment_pointcloud(xyz, 10, device=DEV, index="grid")
    sizes = np.unique(knn, return_counts=True)[1]
    assert sizes.shape[0] >= 1000 and sizes.max() <= 12, "the kNN path is unchanged: every clump its own segment"


# ---- cell edges ---------------------------------------------------------------------------------------------------------------------------
def _speck_ref():
    if not _specks:
        _specks["xyz"] = CR.speck_cloud()[0]
        _specks["ref"] = Q.sorted_edges(_specks["xyz"], 0.06)
        _specks["ids"] = P.merge(_specks["ref"]["edges"], _specks["ref"]["w"], _specks["xyz"].shape[0], 0.01, 20)
    return _specks["xyz"], _specks["ref"], _specks["ids"]


def test_the_cell_edge_cannot_change_a_byte():
    from seggroup_amd import components as M
    xyz, ref, seg = _speck_ref()
    _check(_run(xyz, 0.06), ref, seg, "the library's cell")
    assert M.radius_stats()["R"] == 1
    for cell, rings in FORCED[0.06]:
        got = _run(xyz, 0.06, cell=cell)
        assert M.radius_stats()["R"] == rings, "the forced cell needs a block of more than one ring"
        _check(got, ref, seg, "cell %g" % cell)
    indptr, indices = M.radius_neighbours(xyz, 0.06, cell=100.0, device=DEV)
    assert M.radius_stats()["cells"] == [1, 1, 1]
    _same_bits(indptr.cpu().numpy(), ref["off"], "one cell: off")
    _same_bits(indices.cpu().numpy(), ref["idx"], "one cell: idx")


# ---- the capacity protocol ------------------------------------------------------------------------------------------------------------------
def test_capacity_protocol(sg_lib):
    import torch
    from seggroup_amd import hip
    from seggroup_amd.device import workspace as _ws
    xyz, _, ref, _ = Q.case("room_dup")
    n, want_t = xyz.shape[0], int(ref["off"][-1])
    d_x = torch.from_numpy(xyz).to(DEV)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    t = C.c_int64(-1)
    call = sg_lib.sg_radius_neighbours_grid
    ws = _ws(sg_lib.sg_radius_neighbours_ws_bytes(n, 0), DEV)
    assert call(d_x.data_ptr(), 3, n, Q.ROOM_RADIUS, 0.0, 0, off.data_ptr(), None, C.byref(t), ws.data_ptr(), ws.numel(), None) == hip.SG_ENOMEM
    assert t.value == want_t, "the query form returns T"
    _same_bits(off.cpu().numpy(), ref["off"], "the query form leaves a valid off")
    ws = _ws(sg_lib.sg_radius_neighbours_ws_bytes(n, want_t), DEV)
    idx = torch.full((want_t,), -5, dtype=torch.int32, device=DEV)
    off.fill_(-7)
    t.value = -1
    assert call(d_x.data_ptr(), 3, n, Q.ROOM_RADIUS, 0.0, want_t - 1, off.data_ptr(), idx.data_ptr(), C.byref(t), ws.data_ptr(), ws.numel(),
                None) == hip.SG_ENOMEM
    assert t.value == want_t and b"pairs; the caller's lists hold" in sg_lib.sg_last_error()
    assert bool((idx == -5).all()), "one pair short: d_idx is untouched"
    _same_bits(off.cpu().numpy(), ref["off"], "one pair short: off is written all the same")
    assert call(d_x.data_ptr(), 3, n, Q.ROOM_RADIUS, 0.0, want_t, off.data_ptr(), idx.data_ptr(), C.byref(t), ws.data_ptr(), ws.numel(),
                None) == hip.SG_OK
    _same_bits(idx.cpu().numpy(), ref["idx"], "capacity = T")
    # the segmenter's form of the same protocol
    e, edges, w, nrm = C.c_int(-1), torch.empty((want_t // 2, 2), dtype=torch.int32, device=DEV), torch.empty(want_t // 2, device=DEV), \
        torch.empty((n, 3), device=DEV)
    ws = _ws(sg_lib.sg_pcseg_ws_bytes_radius(n, want_t - 2), DEV)
    t.value = -1
    assert sg_lib.sg_pcseg_edges_radius(d_x.data_ptr(), n, Q.ROOM_RADIUS, 0.0, want_t - 2, None, None, None, nrm.data_ptr(), edges.data_ptr(),
                                        w.data_ptr(), C.byref(e), C.byref(t), ws.data_ptr(), ws.numel(), None) == hip.SG_ENOMEM
    assert (t.value, e.value) == (want_t, 0)


# ---- smaller checks ---------------------------------------------------------------------------------------------------------------------------
def test_rows_of_4_and_6_floats():
    from seggroup_amd import components as M
    xyz, _, ref, _ = Q.case("room_dup")
    for cols in (4, 6):
        wide = np.full((xyz.shape[0], cols), np.nan, np.float32)                # what lies behind the coordinates is never read
        wide[:, :3] = xyz
        indptr, indices = M.radius_neighbours(wide, Q.ROOM_RADIUS, device=DEV)
        _same_bits(indptr.cpu().numpy(), ref["off"], "rows of %d floats: off" % cols)
        _same_bits(indices.cpu().numpy(), ref["idx"], "rows of %d floats: idx" % cols)


def test_a_callers_viewpoint_turns_the_normals():
    xyz, radius, ref0, _ = Q.case("room_j5e-4")
    at = (0.4, 0.3, 30.0)
    ref = Q.sorted_edges(xyz, radius, viewpoint=at)
    assert (ref["normals"] != ref0["normals"]).any(), "the viewpoint of this test turns some normals"
    _check(_run(xyz, radius, viewpoint=at), ref, P.merge(ref["edges"], ref["w"], xyz.shape[0], 0.01, 20), "viewpoint")
    from seggroup_amd import hip, oversegment
    nrm = oversegment.pointcloud_normals(xyz, radius=radius, viewpoint=at, device=DEV)
    _same_bits(nrm.cpu().numpy(), ref["normals"], "pointcloud_normals(radius=)")
    with pytest.raises(hip.SgError) as ei:
        oversegment.pointcloud_normals(xyz, radius=radius, viewpoint=(0.0, np.inf, 0.0), device=DEV)
    assert ei.value.code == hip.SG_EINVAL and "viewpoint" in str(ei.value)


def test_voxel_thinning_combines_with_the_radius_graph():
    """a grid that leaves every point alone gives the un-thinned ids; on the clumped room a grid of the jitter's scale takes the clumps apart
    first, and the radius graph of the representatives is the statement's on them"""
    from seggroup_amd import oversegment, thin
    xyz, radius, _, seg = Q.case("room_j5e-4")
    _same_bits(oversegment.segment_pointcloud(xyz, radius=radius, voxel=0.01, device=DEV), seg, "a voxel that thins nothing")
    xyz, _ = Q.clumped_room()
    got = oversegment.segment_pointcloud(xyz, radius=Q.CLUMPED_RADIUS, voxel=0.013, device=DEV)
    rep, top, _ = thin.thin_cloud(xyz, 0.013, device=DEV)
    rep, top = rep.cpu().numpy(), top.cpu().numpy()
    assert rep.shape[0] < xyz.shape[0] // 4, "the grid thins the clumps"
    want = rep[Q.segment_pointcloud(xyz[rep], Q.CLUMPED_RADIUS)[top]].astype(np.int32)
    _same_bits(got, want, "thinned first")


def test_two_streams_on_two_threads_give_the_same_bytes_as_alone():
    import torch
    names = ("room_dup", "clumped_room")
    for name in names:
        Q.case(name)
    jobs, errors = {}, []

    def work(name):
        try:
            xyz, radius, _, _ = Q.case(name)
            stream = torch.cuda.Stream(device=DEV)
            jobs[name] = [_run(xyz, radius, stream=stream) for _ in range(2)]
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(name,)) for name in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name in names:
        _, _, ref, seg = Q.case(name)
        for got in jobs[name]:
            _check(got, ref, seg, name + " beside another stream")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_leave_the_library_usable():
    import torch
    from seggroup_amd import components as M
    from seggroup_amd import hip, oversegment
    xyz, radius, ref, seg = Q.case("room_dup")
    n = xyz.shape[0]
    x = xyz.copy()
    x[n - 1, 1] = np.nan
    for call in (lambda: M.radius_neighbours(x, radius, device=DEV), lambda: oversegment.pointcloud_edges(x, radius=radius, device=DEV),
                 lambda: oversegment.segment_pointcloud(x, radius=radius, device=DEV)):
        with pytest.raises(hip.SgError) as ei:
            call()
        assert ei.value.code == hip.SG_EINVAL and "not finite" in str(ei.value)
    _check(_run(xyz, radius), ref, seg, "after a NaN")
    # a caller's table: an entry outside 0..N-1, offsets that do not ascend, offsets past off[N]
    off, idx = ref["off"], ref["idx"]
    good = oversegment.pointcloud_normals(xyz, radius=radius, lists=(off, idx), device=DEV)
    _same_bits(good.cpu().numpy(), ref["normals"], "a caller's table")
    bad_idx = idx.copy()
    bad_idx[idx.shape[0] // 2] = n
    bad_off = off.copy()
    bad_off[n // 2] = off[n // 2 + 1] + 3
    far_off = off.copy()
    far_off[n // 3] = 1 << 40
    for lists, text in (((off, bad_idx), "names a point outside"), ((bad_off, idx), "do not ascend"), ((far_off, idx), "do not ascend")):
        with pytest.raises(hip.SgError) as ei:
            oversegment.pointcloud_normals(xyz, radius=radius, lists=lists, device=DEV)
        assert ei.value.code == hip.SG_EINVAL and text in str(ei.value)
    torch.cuda.synchronize()
    _check(_run(xyz, radius), ref, seg, "after the corrupt tables")


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------
def test_python_forms():
    import torch
    from seggroup_amd import components as M
    xyz, ref, _ = _speck_ref()
    n = xyz.shape[0]
    indptr, indices = M.radius_neighbours(xyz, 0.06, device=DEV)
    assert indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int64 and indices.dtype == torch.int32
    assert indptr.shape == (n + 1,) and indices.shape == (int(ref["off"][-1]),)
    cnt = M.neighbour_counts(xyz, 0.06, device=DEV)
    assert torch.equal(indptr[1:] - indptr[:-1], cnt.long()) and int(indptr[0]) == 0
    upper = Q.edges_of(indptr.cpu().numpy(), indices.cpu().numpy())
    by_edges = M.components(n, edges=upper, device=DEV)
    by_radius = M.components(n, radius=0.06, xyz=xyz, device=DEV)
    assert by_edges[2] == by_radius[2] and torch.equal(by_edges[0], by_radius[0]) and torch.equal(by_edges[1], by_radius[1])
    # a tensor on the device, and a radius with no pair at all
    indptr2, indices2 = M.radius_neighbours(torch.from_numpy(xyz).to(DEV), 0.06, device=DEV)
    assert torch.equal(indptr2, indptr) and torch.equal(indices2, indices)
    indptr0, indices0 = M.radius_neighbours(RR.jittered_line(65), 0.05, device=DEV)
    assert indices0.shape == (0,) and not bool(indptr0.any())


def test_stage_times_are_reported_under_their_names(sg_lib):
    from seggroup_amd import oversegment
    xyz, radius, ref, _ = Q.case("room_dup")
    sg_lib.sg_pcseg_radius_set_timing(1)
    try:
        got = oversegment.pointcloud_edges(xyz, radius=radius, device=DEV)
    finally:
        sg_lib.sg_pcseg_radius_set_timing(0)
    us = (C.c_float * 13)()
    assert sg_lib.sg_pcseg_radius_stage_times(us, 13) == 13
    assert all(v > 0.0 for v in us), list(us)
    _same_bits(got["indices"].cpu().numpy(), ref["idx"], "a timed call")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _clumped_scan(directory, name):
    xyz, plane = Q.clumped_room()
    rgb = np.stack([plane * 20 + 40, 200 - plane * 15, plane * 9 + 10], 1).astype(np.uint8)
    os.makedirs(os.path.join(directory, name))
    P.write_vertex_only_ply(os.path.join(directory, name, name + "_vh_clean_2.ply"), xyz, rgb)
    return xyz


def test_faceless_scan_of_the_clumped_room_reaches_the_forward(tmp_path, weight_sets):
    """vertices only -> prepare_scene(oversegment=True, radius=0.06) -> the reference's tree -> pack -> SegModel.forward: the segs.json is
    the statement's, the raw adjacency is the statement's edge list, the resampled one its rows through the unmapper, and the labels
    equal the oracle's on the same prepared inputs."""
    import torch
    from oracle import cpu_ref
    from seggroup_amd import cache, hip, oversegment, prepare, synthetic
    from seggroup_amd.model import SegModel
    from seggroup_amd.scene import seg_from_lists
    name, root, n = "scene0041_00", str(tmp_path), 3000
    base = os.path.join(root, "dataset", "scannet")
    xyz = _clumped_scan(os.path.join(base, "scans"), name)
    sp = os.path.join(base, "scans", name)
    _, _, ref, want = Q.case("clumped_room")
    perm = np.random.RandomState(5).permutation(xyz.shape[0])
    prepare.prepare_scene(sp, 0, n, root=base, perm=perm, device=DEV, oversegment=True, label_style=None, radius=Q.CLUMPED_RADIUS)
    doc = json.load(open(os.path.join(sp, oversegment.segs_json_name(name))))
    assert doc["sceneId"] == name and np.array_equal(np.asarray(doc["segIndices"], np.int32), want) and np.unique(want).shape[0] == 16
    unmap = torch.load(os.path.join(base, "data", "resampled", name, name + ".unmap.pth")).numpy()
    raw = torch.load(os.path.join(base, "adj", "mesh", "raw", name, name + ".adj.pth")).numpy()
    adj = torch.load(os.path.join(base, "adj", "mesh", "resampled", name, name + ".adj.pth")).numpy()
    assert raw.dtype == np.int64 and np.array_equal(raw, ref["lex_edges"].astype(np.int64)), "the raw adjacency is the statement's edge list"
    # as the kNN rows are turned: self rows of the RAW list dropped (the statement has none), through the unmapper, per-row sorted, unique
    assert (raw[:, 0] < raw[:, 1]).all()
    assert adj.dtype == np.int64 and np.array_equal(adj, np.unique(np.sort(unmap[raw], axis=1), axis=0))
    lists = json.load(open(os.path.join(base, "label", "real", "resampled", name, name + ".seg.json")))
    seg = seg_from_lists(lists, n)
    s = int(seg.max()) + 1
    weak = np.full((n, 2), -1, np.int64)
    for k, g in enumerate(range(0, s, max(s // 9, 1))):
        weak[seg == g] = (k % 5 + 1, k)
    gt = np.stack([np.maximum(weak[unmap, 0], 0) + 1, np.maximum(weak[unmap, 1], 0) + 1], 1).astype(np.int64)
    for sub, arr in ((("label", "seg", "manual", "resampled"), weak), (("label", "real", "raw"), gt)):
        dd = os.path.join(base, *sub, name)
        os.makedirs(dd, exist_ok=True)
        torch.save(torch.from_numpy(arr), os.path.join(dd, name + ".label.pth"))
    ds = cache.load_pack(cache.pack_scene(root, name), device=DEV)
    assert (ds.N, ds.S, ds.V) == (n, s, xyz.shape[0])
    net = SegModel(exp_name="t", ins_infer=True, data_root=root)
    net.load_weights(weight_sets["ins_infer"])
    net.epoch = "ins_infer"
    res = net.forward_scene(ds, write=False)
    data = torch.load(os.path.join(base, "data", "resampled", name, name + ".pcl.pth")).numpy()
    oracle = cpu_ref.forward_scene(synthetic.Scene(name, data, weak, seg, adj, unmap, gt), weight_sets["ins_infer"], "ins_infer")
    assert res.trace == oracle["trace"]
    for i in range(14):
        assert res.labels[i].shape == (xyz.shape[0],)
        assert np.array_equal(res.labels[i], oracle["labels"][hip.LABEL_NAMES[i]].astype(np.int32)), hip.LABEL_NAMES[i]


def test_command_line_in_a_child_process(tmp_path):
    from seggroup_amd import oversegment
    name = "scene0042_00"
    by_cli, by_call = str(tmp_path / "cli"), str(tmp_path / "call")
    xyz = _clumped_scan(by_cli, name)
    _clumped_scan(by_call, name)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "seggroup_amd.oversegment", "--workers", "1", "--scans", by_cli, "--radius", str(Q.CLUMPED_RADIUS)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "1 written, 0 skipped" in r.stdout, (r.stdout + r.stderr)[-3000:]
    p = oversegment.oversegment_scan(os.path.join(by_call, name), device=DEV, radius=Q.CLUMPED_RADIUS)
    got = open(os.path.join(by_cli, name, oversegment.segs_json_name(name)), "rb").read()
    assert got == open(p, "rb").read()
    assert np.array_equal(np.asarray(json.loads(got)["segIndices"], np.int32), Q.case("clumped_room")[3])
