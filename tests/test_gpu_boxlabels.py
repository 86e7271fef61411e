"""Points in boxes and box labels on the GPU (seggroup_amd/boxlabels.py) against tests/boxlabels_ref.py: sg_points_in_boxes
EQUAL to the restatement at every shape, in batches, on faces and ties, the same bytes on every call, the refusals, the loop closed with
`boxes`, and the command on a lattice scene whose label files are worked out by hand."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boxes_ref as BR
import boxlabels_ref as R
import pcseg_ref as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# a workgroup takes 256 points of one scene and stages 128 boxes at a time: the sizes either side of each
POINTS = (0, 1, 255, 256, 257, 1000)
BOXES = (0, 1, 2, 127, 128, 129, 300)
SMALL_FROM = 65                               # from this many boxes on, sizes are drawn from 0.05 .. 0.5: the three classes of points stay populated


def _boxes(seed, k, smax=1.55):
    """k boxes in a 2 m cube, float32-valued centres, sizes 0.05 .. smax, even boxes with a yaw, odd boxes with a QR frame; a tenth repeat
    an earlier box, a twentieth have a zero size"""
    rng = np.random.RandomState(seed)
    out = np.zeros((k, 15))
    for j in range(k):
        c = (rng.rand(3) * 2.0).astype(np.float32).astype(np.float64)
        s = 0.05 + (smax - 0.05) * rng.rand(3)
        if rng.rand() < 0.05:
            s[rng.randint(0, 3)] = 0.0
        if j % 2 == 0:
            frame = R.yaw_frame(rng.rand() * 2.0 * np.pi)
        else:
            frame, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out[j] = R.row(*c, *s, R=frame)
        if j and rng.rand() < 0.1:
            out[j] = out[rng.randint(0, j)]
    return out


def _points(seed, n):
    return (np.random.RandomState(seed).rand(n, 3) * 2.0).astype(np.float32)


def _gpu(xyz, boxes, margin=0.0, off_p=None, off_b=None, stream=None):
    from seggroup_amd import boxlabels
    r = boxlabels.points_in_boxes(xyz, boxes, margin, off_p, off_b, device=DEV, stream=stream, held=True)
    out = tuple(t.cpu().numpy() for t in r)
    assert all(t.dtype == np.int32 for t in out)
    return out


def _same(got, want, what=""):
    for name, g, w in zip(("count", "first", "inner", "held"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, int((g != w).sum()))


@pytest.fixture(scope="module")
def cloud():
    """the reference once: 1,000 points against 300 boxes of either size range; every smaller shape is a corner of one of the two matrices"""
    xyz = _points(5, 1000)
    sets = {False: _boxes(6, 300), True: _boxes(7, 300, 0.5)}
    return xyz, sets, {small: R.inside_matrix(xyz, b) for small, b in sets.items()}


@pytest.mark.parametrize("k", BOXES)
def test_equals_the_restatement_at_every_shape(cloud, k):
    xyz, sets, matrices = cloud
    small = k >= SMALL_FROM
    inside, vol = matrices[small]
    for n in POINTS:
        count, first, inner = R.scene_outputs(inside[:n, :k], vol[:k])
        _same(_gpu(xyz[:n], sets[small][:k]), (count, first, inner, inside[:n, :k].sum(0).astype(np.int32)), (n, k))
        if n == 1000 and small:
            assert (count == 0).any() and (count == 1).any() and (count > 1).any() and (first != inner).any(), (n, k)


def test_without_the_counts_per_box(cloud):
    from seggroup_amd import boxlabels
    xyz, sets, matrices = cloud
    r = boxlabels.points_in_boxes(xyz, sets[True], device=DEV)
    assert r.held is None
    _same(tuple(t.cpu().numpy() for t in r[:3]), R.scene_outputs(*matrices[True]))
    wide = np.concatenate([xyz, np.full((1000, 3), np.nan, np.float32)], 1)             # a stride of 6: what lies behind xyz is not read
    _same(_gpu(wide, sets[True])[:3], R.scene_outputs(*matrices[True]))


@pytest.mark.parametrize("scenes", (1, 2, 7))
def test_in_batches(scenes):
    n_p = [300, 0, 257, 5, 0, 700, 256][:scenes]
    n_b = [9, 4, 0, 130, 0, 3, 1][:scenes]                                  # scenes empty on the point side, the box side, and both
    xyz, boxes = _points(8, sum(n_p)), _boxes(9, sum(n_b))
    off_p, off_b = np.concatenate([[0], np.cumsum(n_p)]), np.concatenate([[0], np.cumsum(n_b)])
    want = R.points_in_boxes(xyz, boxes, 0.0, off_p, off_b)
    _same(_gpu(xyz, boxes, 0.0, off_p, off_b), want)
    if scenes == 7:
        assert want[0][300:557].max() == 0 and want[1][300:557].max() == -1          # the scene without boxes
        assert (want[0][:300] > 0).any() and (want[0][557:] > 0).any()
        bad = xyz.copy()
        bad[400] = np.nan                                                    # a point of the scene WITHOUT boxes may hold anything
        _same(_gpu(bad, boxes, 0.0, off_p, off_b), want)
    _same(_gpu(xyz, boxes, 0.125, off_p, off_b), R.points_in_boxes(xyz, boxes, 0.125, off_p, off_b))


def test_faces_edges_and_corners():
    """the hand cases of tests/test_boxlabels_ref.py on the device: a lattice point on a face is inside, one step out it is not"""
    step = 0.25
    box, turned = R.row(1, 1, 0.5, 2, 1, 1), R.row(1, 1, 0.5, 1, 2, 1, R=R.QUARTER)
    on = np.array([[2, 1, 0.5], [2, 1.5, 0.5], [2, 1.5, 1], [0, 0.5, 0], [1, 1, 0.5]], np.float32)
    off = np.array([[2.25, 1, 0.5], [2.25, 1.75, 0.5], [2.25, 1.75, 1.25], [-0.25, 0.25, -0.25], [1, 1, 1.25]], np.float32)
    for b in (box, turned):
        assert _gpu(on, b[None])[0].tolist() == [1] * 5 and _gpu(off, b[None])[0].tolist() == [0] * 5
        assert _gpu(off, b[None], step)[0].tolist() == [1] * 5 and _gpu(off, b[None], step / 2)[0].tolist() == [0] * 5
    cub = BR.lattice_cuboid()                                                # 585 points filling [0,3] x [0,2] x [0,1]
    for margin in (0.0, step):
        tight = R.row(1.5, 1, 0.5, 3 - 2 * margin, 2 - 2 * margin, 1 - 2 * margin)       # with the margin, the cuboid's own box again
        got = _gpu(cub, np.stack([tight, R.row(1.5, 1, 0.5, 3, 2, 0), R.row(1.5, 1, 0.5, 2.5, 1.5, 0.5)]), margin)
        _same(got, R.points_in_boxes(cub, np.stack([tight, R.row(1.5, 1, 0.5, 3, 2, 0), R.row(1.5, 1, 0.5, 2.5, 1.5, 0.5)]), margin))
        assert got[3][0] == 585 and got[3][1] == (117 if margin == 0.0 else 117 * 3)    # the sheet z = 0.5 holds its plane: 13 x 9 points


def test_ties_go_to_the_lowest_index():
    boxes = _boxes(11, 200)
    boxes[:, 0] += 10.0                                                      # away from the points
    same = R.row(1, 1, 1, 2, 1, 1)
    boxes[150] = boxes[31] = boxes[97] = same                                # three identical boxes
    boxes[20] = R.row(1, 1, 1, 1, 2, 1)                                      # another shape of the same volume, (1*2)*1 == (2*1)*1
    boxes[180] = R.row(1, 1, 1, 4, 4, 4)
    boxes[10] = R.row(1, 1, 1, 0.5, 0.5, 0.5)
    xyz = np.array([[1, 1, 1], [1.75, 1, 1], [1, 1.75, 1], [2.5, 2.5, 2.5], [9, 9, 9]], np.float32)
    count, first, inner, held = _gpu(xyz, boxes)
    assert count.tolist() == [6, 4, 2, 1, 0] and first.tolist() == [10, 31, 20, 180, -1] and inner.tolist() == [10, 31, 20, 180, -1]
    assert held[[10, 20, 31, 97, 150, 180]].tolist() == [1, 2, 2, 2, 2, 4]
    _same((count, first, inner, held), R.points_in_boxes(xyz, boxes))
    count, first, inner, _ = _gpu(xyz[:1], boxes[11:])                       # without the small one: the lowest of the equal volumes
    assert (count.tolist(), first.tolist(), inner.tolist()) == ([5], [9], [9])


def test_same_bytes_on_a_second_call_and_a_second_stream(cloud):
    import torch
    xyz, sets, _ = cloud
    first = _gpu(xyz, sets[True], 0.01)
    side = torch.cuda.Stream(device=DEV)
    for stream in (None, side):
        again = _gpu(xyz, sets[True], 0.01, stream=stream)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first))


# ---- the refusals of the library ------------------------------------------------------------------------------------------------------------
def _raw(xyz, boxes, off_p, off_b, margin=0.0, n=None, k=None, stride=3, null=(), short_ws=0):
    """the library itself, past the module's own checks -> (return code, sg_last_error)"""
    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    off_p, off_b = np.asarray(off_p, np.int32), np.asarray(off_b, np.int32)
    scenes = off_p.shape[0] - 1
    n, k = xyz.shape[0] if n is None else n, boxes.shape[0] if k is None else k
    d_xyz, d_box = torch.from_numpy(xyz).to(DEV), torch.from_numpy(boxes).to(DEV)
    out = torch.zeros((3, max(xyz.shape[0], 1)), dtype=torch.int32, device=DEV)
    need = int(lib.sg_points_in_boxes_ws_bytes(xyz.shape[0], boxes.shape[0], min(scenes, 1 << 16)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    ptr = dict(xyz=d_xyz.data_ptr(), box=d_box.data_ptr(), count=out[0].data_ptr(), first=out[1].data_ptr(), inner=out[2].data_ptr(), ws=ws.data_ptr(),
               off_p=off_p.ctypes.data, off_b=off_b.ctypes.data)
    ptr.update({name: None for name in null})
    rc = lib.sg_points_in_boxes(ptr["xyz"], stride, n, ptr["box"], k, ptr["off_p"], ptr["off_b"], scenes, margin, ptr["count"], ptr["first"],
                                ptr["inner"], None, ptr["ws"], need - short_ws, None)
    torch.cuda.synchronize()
    return rc, lib.sg_last_error().decode()


def test_refusals_leave_the_next_call_right(cloud):
    from seggroup_amd import boxlabels, hip
    xyz, sets, matrices = cloud
    xyz, boxes = xyz[:300].copy(), sets[False][:12].copy()
    want = R.scene_outputs(matrices[False][0][:300, :12], matrices[False][1][:12])
    off_p, off_b = [0, 300], [0, 12]

    def valid():
        _same(_gpu(xyz, boxes)[:3], want)

    valid()
    rc, _ = _raw(xyz, boxes, off_p, off_b)
    assert rc == hip.SG_OK
    for kw in (dict(null=("xyz",)), dict(null=("box",)), dict(null=("count",)), dict(null=("first",)), dict(null=("inner",)), dict(null=("ws",)),
               dict(null=("off_p",)), dict(null=("off_b",)), dict(stride=2), dict(n=-1), dict(k=-1), dict(margin=-1e-300), dict(margin=float("nan")),
               dict(margin=float("inf")), dict(short_ws=1)):
        rc, msg = _raw(xyz, boxes, off_p, off_b, **kw)
        assert rc == hip.SG_EINVAL and "sg_points_in_boxes" in msg, (kw, rc, msg)
    valid()
    for op, ob, text in (([1, 300], [0, 12], "start at 0"), ([0, 300], [2, 12], "start at 0"), ([0, 200, 100, 300], [0, 4, 8, 12], "ascend"),
                         ([0, 100, 300], [0, 13, 12], "ascend"), ([0, 299], [0, 12], "end at"), ([0, 301], [0, 12], "end at"), ([0, 300], [0, 11], "end at"),
                         ([0, 300], [0, 13], "end at"), ([0, 100, 300], [0, -1, 12], "ascend")):
        rc, msg = _raw(xyz, boxes, op, ob)
        assert rc == hip.SG_EINVAL and "sg_points_in_boxes" in msg and text in msg, msg
    valid()
    # through the flag word
    for column, value, text in ((0, np.nan, "not finite"), (2, np.inf, "not finite"), (5, -np.inf, "not finite"), (10, np.nan, "not finite"),
                                (3, -0.5, "negative size"), (5, -1e-300, "negative size"), (6, 1.1, "not orthonormal"), (9, 2e-3, "not orthonormal")):
        bad = boxes.copy()
        bad[4] = R.row(1, 1, 1, 1, 1, 1)
        bad[4, column] = value                                               # column 9 of the identity: r_0.r_1 = 2e-3
        with pytest.raises(ValueError, match=text) as e:
            boxlabels.points_in_boxes(xyz, bad, device=DEV)
        assert "sg_points_in_boxes" in str(e.value)
        valid()
    near = boxes.copy()
    near[4] = R.row(1, 1, 1, 1, 1, 1)
    near[4, 9] = 9e-7                                                        # inside the tolerance
    boxlabels.points_in_boxes(xyz, near, device=DEV)
    for row, column, value in ((7, 0, np.nan), (299, 2, np.inf), (0, 1, -np.inf)):
        bad = xyz.copy()
        bad[row, column] = value
        with pytest.raises(ValueError, match="coordinate that is not finite") as e:
            boxlabels.points_in_boxes(bad, boxes, device=DEV)
        assert "sg_points_in_boxes" in str(e.value)
        valid()
    bad = xyz.copy()
    bad[7] = np.nan
    r = boxlabels.points_in_boxes(bad, np.zeros((0, 15)), device=DEV)         # no boxes: 0 / -1 / -1 whatever the point holds
    assert not r.count.any().item() and (r.first == -1).all().item() and (r.inner == -1).all().item() and r.count.shape == (300,)
    r = boxlabels.points_in_boxes(np.zeros((0, 3), np.float32), boxes, device=DEV, held=True)
    assert r.count.shape == (0,) and r.held.cpu().tolist() == [0] * 12
    flat = boxes.copy()
    flat[4, 3:6] = 0.0                                                       # a zero size is valid
    _same(_gpu(xyz, flat), R.points_in_boxes(xyz, flat))
    # the limits: refused before anything is read
    for n, k, scenes in (((1 << 24) + 1, 12, 1), (300, (1 << 20) + 1, 1), (300, 12, (1 << 16) + 1)):
        rc, msg = _raw(xyz, boxes, [0] * scenes + [300], [0] * scenes + [12], n=n, k=k)
        assert rc == hip.SG_EUNSUP and "sg_points_in_boxes" in msg and "2^24" in msg, msg
    valid()


# ---- the loop closed with `boxes` -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,margin", (("aabb", 0.0), ("yaw", 1e-9), ("pca", 1e-9)))
def test_every_labelled_point_is_in_its_own_box(kind, margin):
    """label_boxes, then the points in label_index order with the label offsets as the SCENE offsets and one box a scene: every point is in
    its label's box.  aabb at margin 0: lo + hi, its half, hi - lo and x - c are exact for float32 inputs of like magnitude."""
    from seggroup_amd import boxes, boxlabels
    rng = np.random.RandomState(12)
    n, l = 3000, 70
    centres = rng.rand(l, 3) * 4.0
    labels = rng.randint(-1, l, n).astype(np.int32)                          # -1: not labelled
    spread = rng.normal(size=(n, 3)) * np.array([0.4, 0.15, 0.05])
    turn = np.stack([R.yaw_frame(a) for a in rng.rand(l) * np.pi])
    xyz = (centres[labels] + np.einsum("na,nab->nb", spread, turn[labels])).astype(np.float32)
    found = boxes.label_boxes(xyz, labels, kind=kind, device=DEV)
    index = boxes.label_index(labels, device=DEV)
    order, start = index.order.cpu().numpy(), index.start.cpu().numpy()
    k = found.values.shape[0]
    assert k == np.unique(labels[labels >= 0]).shape[0] and start.shape[0] == k + 1 and k > 60
    rows = boxlabels.box_frames(found)
    got = _gpu(xyz[order], rows, margin, start, np.arange(k + 1))
    _same(got, R.points_in_boxes(xyz[order], rows, margin, start, np.arange(k + 1)))
    assert (got[0] == 1).all() and not got[1].any() and not got[2].any() and np.array_equal(got[3], np.diff(start))


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def _run(args, tail):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "seggroup_amd.boxlabels"] + args, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and tail in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def _txt(path):
    with open(path, "rb") as f:
        return np.array(f.read().split(), dtype=np.int64)


def test_command_on_a_lattice_scene(tmp_path):
    """Four lattice cuboids of 585 points (13 x 9 x 5 on a 0.25 lattice filling 3 x 2 x 1; every box below is exact): A at the origin,
    B at +6 in x, C at +6 in y and D at +2.5 in x, so the boxes of A and D share x in [2.5, 3]: the 135 points of A with x >= 2.5 and
    the 135 points of D with x <= 3 lie in both.  Instances 1..4 = A, B, C, D with classes chair (5), table (7), chair, sofa (6); the
    aabb boxes come in that order and all have volume (3*2)*1, so `inner` of the shared points is A, the lower index.  Segments:
      0  A without the shared part, 450 vertices        1  A's shared part, 135        2  D's shared part, 135        3  the rest of D, 450
      4  B with x' <= 2.5, 495 vertices                 5  STRADDLES: B's last two lattice planes (90) and C's first (45)
      6  the rest of C, 540
    --overlap skip, purity 1: segments 0, 3, 4, 6 take A, D, B, C; 1 and 2 hold "several"; 5 is 90 of 135 for B: not pure.
      labelled 450 + 450 + 495 + 540 = 1935, all of them right (agree 1935); several 270; every box has a segment
      per box inside / owned / segments / vertices:  A 720 / 450 / 1 / 450   B 585 / 585 / 1 / 495   C 585 / 585 / 1 / 540   D 720 / 450 / 1 / 450
    --overlap inner: the 270 shared vertices vote for A, so segments 1 and 2 take A too -- and D's 135 get the WRONG instance:
      labelled 2205, agree 2070;  A 720 / 720 / 3 / 720, D 720 / 450 / 1 / 450, B and C as before."""
    import torch
    from seggroup_amd import boxes, boxlabels, labels, pseudo_labels
    scene = "scene0011_00"
    cub = BR.lattice_cuboid()
    shifts = np.float32([[0, 0, 0], [6, 0, 0], [0, 6, 0], [2.5, 0, 0]])
    x = np.tile(cub[:, 0], 4)                                                # the coordinate within the cuboid
    xyz = np.concatenate([cub + s for s in shifts]).astype(np.float32)
    ins = np.repeat([1, 2, 3, 4], 585)
    seg = np.select([(ins == 1) & (x < 2.5), ins == 1, (ins == 4) & (x <= 0.5), ins == 4, (ins == 2) & (x <= 2.5), (ins == 2) | ((ins == 3) & (x == 0))],
                    [0, 1, 2, 3, 4, 5], 6)
    assert np.bincount(seg).tolist() == [450, 135, 135, 450, 495, 135, 540]
    perm = np.random.RandomState(4).permutation(xyz.shape[0])
    xyz, ins, seg = np.ascontiguousarray(xyz[perm]), ins[perm], seg[perm]
    sem = np.array([0, 5, 7, 5, 6])[ins]
    root = str(tmp_path)
    scans_dir = os.path.join(root, "scans")
    os.makedirs(os.path.join(scans_dir, scene))
    P.write_vertex_only_ply(os.path.join(scans_dir, scene, scene + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))
    with open(os.path.join(scans_dir, scene, scene + "_vh_clean_2.0.010000.segs.json"), "w") as f:
        json.dump({"params": {}, "sceneId": scene, "segIndices": [int(s) for s in seg]}, f)
    raw = os.path.join(root, "label", "real", "raw", scene)
    labels._write_txt(os.path.join(raw, scene + ".ins.txt"), ins)
    labels._write_txt(os.path.join(raw, scene + ".sem.txt"), sem)
    mapper = torch.from_numpy(np.random.RandomState(5).randint(0, xyz.shape[0], 500))
    os.makedirs(os.path.join(root, "data", "resampled", scene))
    torch.save(mapper, os.path.join(root, "data", "resampled", scene, scene + ".map.pth"))

    def expected(taking):
        keep = np.isin(seg, taking)
        return np.where(keep, np.where(np.isin(seg, (1, 2)), 1, ins), -1), np.where(keep, np.where(np.isin(seg, (1, 2)), 5, sem), -1)

    def check(style, want_ins, want_sem, per_box, labelled, agree, from_real=True):
        out = os.path.join(root, "label", "seg", style, "raw", scene)
        assert np.array_equal(_txt(os.path.join(out, scene + ".ins.txt")), want_ins) and np.array_equal(_txt(os.path.join(out, scene + ".sem.txt")), want_sem)
        doc = json.load(open(os.path.join(root, "label", "seg", style, boxlabels.REPORT_NAME)))
        e = doc["scenes"][scene]
        assert [[b[k] for k in ("inside", "owned", "segments", "vertices")] for b in e["boxes"]] == per_box
        assert [(b["id"], b["sem"]) for b in e["boxes"]] == [(1, 5), (2, 7), (3, 5), (4, 6)]
        assert (e["labelled"], e["several"], e["boxes_without_segment"], e["V"], e["K"], e["segments"]) == (labelled, 270, 0, 2340, 4, 7)
        assert e.get("agree") == (agree if from_real else None) and e["resampled"] == "written"
        got = torch.load(os.path.join(root, "label", "seg", style, "resampled", scene, scene + ".label.pth"))
        shifted = np.stack([np.where(want_ins >= 0, want_sem - 1, want_sem), np.where(want_ins >= 0, want_ins - 1, want_ins)], 1)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), shifted[mapper.numpy()])
        with np.load(os.path.join(out, scene + boxlabels.NPZ_SUFFIX)) as z:
            assert (z["count"] > 1).sum() == 270 and z["seg_ids"].tolist() == list(range(7)) and z["seg_size"].tolist() == np.bincount(seg).tolist()
            assert np.array_equal(z["first"][z["count"] == 1], ins[z["count"] == 1] - 1) and not z["inner"][z["count"] > 1].any()
        return doc

    base = ["--scans", scans_dir, "--root", root, "--workers", "1"]
    skip = expected((0, 3, 4, 6))
    skip_boxes = [[720, 450, 1, 450], [585, 585, 1, 495], [585, 585, 1, 540], [720, 450, 1, 450]]
    text = _run(base + ["--from-real"], "1 written, 0 skipped")              # the one child process: the command as a user starts it
    assert "1935 labelled in 4 of 7 segments" in text
    doc = check("box", *skip, skip_boxes, 1935, 1935)
    assert doc["parameters"] == dict(from_real=True, kind="aabb", angles=0, min_points=1, margin=0.0, purity=1.0, overlap="skip", style_name="box")
    assert (skip[0] >= 0).sum() == 1935 and np.array_equal(skip[0][skip[0] >= 0], ins[skip[0] >= 0])
    report, skipped = boxlabels.boxlabels_scans(scans_dir, root, workers=1, device=DEV, from_real=True)          # there already: not overwritten
    assert report == {} and skipped == [scene]
    inner = expected((0, 1, 2, 3, 4, 6))
    boxlabels.boxlabels_scans(scans_dir, root, workers=1, device=DEV, from_real=True, overlap="inner", style_name="box_inner", kind="yaw", angles=2)
    check("box_inner", *inner, [[720, 720, 3, 720]] + skip_boxes[1:], 2205, 2070)
    assert (inner[0] >= 0).sum() == 2205 and ((inner[0] >= 0) & (inner[0] == ins)).sum() == 2070
    # purity 0.6: the straddling segment is 90 of 135 for B, so C's 45 vertices in it get B's label
    boxlabels.boxlabels_scans(scans_dir, root, workers=1, device=DEV, from_real=True, purity=0.6, style_name="box_p")
    loose = (np.where(seg == 5, 2, skip[0]), np.where(seg == 5, 7, skip[1]))
    check("box_p", *loose, [skip_boxes[0], [585, 585, 2, 630]] + skip_boxes[2:], 2070, 2025)
    # --boxes over the files `boxes` wrote for the real instances as an experiment: the same label files, on either suffix
    tables = np.zeros((pseudo_labels.INS_NVEC, 4), np.int32)
    tables[12], tables[13] = [1, 2, 3, 4], [5, 7, 5, 6]
    d = os.path.join(root, "results", "truth", scene, "epoch_last")
    os.makedirs(d)
    pseudo_labels.write(d, tables, (ins - 1).astype(np.int32))
    box_dir = os.path.join(root, "boxfiles")
    rep, _ = boxes.boxes_scans(scans_dir, box_dir, workers=1, device=DEV, exp="truth", stage="epoch_last", root=root, min_points=1, kind="aabb",
                               detector_files=True)
    assert rep[scene]["kept"] == 4
    boxlabels.boxlabels_scans(scans_dir, root, workers=1, device=DEV, boxes=box_dir, style_name="box_det", suffix="_bbox.npy")
    check("box_det", *skip, skip_boxes, 1935, None, from_real=False)
    boxlabels.boxlabels_scans(scans_dir, root, workers=1, device=DEV, boxes=box_dir, style_name="box_files")
    check("box_files", *skip, skip_boxes, 1935, None, from_real=False)
