"""sg_lift and sg_lift_vote on the GPU (seggroup_amd/lift.py) against tests/lift_ref.py: label, votes, total, seen, tied, the raw
counts and the seven stats EQUAL to the restatement -- the rule is integers over a fixed sequence of correctly rounded double operations, so
no tolerance appears anywhere --, accumulation over calls, the flag, the refusals, the scan as its own occluder, and the command on a
two-scene tree and on a ScanNet-shaped one."""
import json
import os

import numpy as np
import pytest

import lift_ref as L
import render_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (67, 45)                          # no multiple of a wave
TOL = 0.06                               # lift_ref.soup_images: the planted depths lie within 0.1 of the vertices', so both sides of it occur


def _tables(xyz, cams, classes, depth, tol, C, ortho, near=R.SOUP_NEAR, **kw):
    """lift.fuse -> (counts int64 [V,C], seen int64 [V], the seven stats)"""
    from seggroup_amd import lift as M
    d_counts, d_seen = M.fuse(xyz, cams, classes, C, depth, tol=tol, ortho=ortho, near=near, device=DEV, **kw)
    return d_counts.cpu().numpy().astype(np.int64), d_seen.cpu().numpy().astype(np.int64), M.last_stats()


def _vote(counts):
    """lift.vote on a table -> four int32 arrays"""
    import torch
    from seggroup_amd import lift as M
    out = M.vote(torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(DEV))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check(xyz, cams, classes, depth, tol, C, ortho, want=None, what="", **kw):
    """one fuse and one vote against the restatement -> the restatement's (counts, seen, stats)"""
    if want is None:
        want = L.accumulate(np.asarray(xyz)[:, :3], cams, classes, depth, tol, C, ortho, R.SOUP_NEAR, kw.get("counts"), kw.get("seen"))[:3]
    counts, seen, stats = _tables(xyz, cams, classes, depth, tol, C, ortho, **kw)
    print(what, stats)
    assert np.array_equal(counts, want[0]), (what, "counts", int((counts != want[0]).sum()))
    assert np.array_equal(seen, want[1]), (what, "seen", int((seen != want[1]).sum()))
    assert stats == want[2], (what, stats, want[2])
    for name, a, b in zip(("winner", "votes", "total", "tied"), _vote(counts), L.vote(want[0])):
        assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (what, name, int((a != b).sum()))
    return want


def _three(cam):
    cams = np.stack([cam, cam, cam])
    cams[1, 14] += 11.25                                                         # cx: the image shifted by a fraction of the pixel grid
    cams[2, 3], cams[2, 11] = 0.7, 0.5                                           # the camera moved sideways and back
    return cams


@pytest.fixture(scope="module")
def soup():
    """the soup's points, images and restatements, once: {(projection, C): (cams, ortho, labels, depth, (counts, seen, stats))}"""
    xyz = L.soup_points()
    known = {}
    for name, cam, ortho in zip(("perspective", "orthographic"), R.soup_cameras(SIZE), (False, True)):
        for C in (5, 70):
            cams = _three(cam)
            labels, depth, _ = L.soup_images(xyz, cams, SIZE, C, ortho, seed=C)
            counts, seen, stats, bad = L.accumulate(xyz, cams, labels, depth, TOL, C, ortho, R.SOUP_NEAR)
            assert bad == 0
            known[name, C] = (cams, ortho, labels, depth, (counts, seen, stats))
    return xyz, known


@pytest.mark.parametrize("C", (5, 70))
@pytest.mark.parametrize("projection", ("perspective", "orthographic"))
def test_a_soup_of_3000_points_in_three_views(soup, projection, C):
    xyz, known = soup
    cams, ortho, labels, depth, want = known[projection, C]
    assert xyz.shape[0] == 3000 and all(want[2][k] > 0 for k in L.STAT_NAMES), want[2]       # every kind of pair occurs
    assert sum(want[2].values()) == 3 * 3000 and (want[0].sum(1) > 1).any()
    _check(xyz, cams, labels, depth, TOL, C, ortho, want=want, what=(projection, C))
    wide = np.concatenate([xyz, np.full((xyz.shape[0], 3), np.nan, np.float32)], 1)          # rows of 6 floats: only the first three are read
    _check(wide, cams, labels, depth, TOL, C, ortho, want=want, what=(projection, C, "stride 6"))


def test_lift_returns_labels_not_classes(soup):
    from seggroup_amd import lift as M
    xyz, known = soup
    cams, ortho, labels, depth, _ = known["perspective", 5]
    sparse = np.where(labels >= 0, np.array([3, 7, 40, 41, 65535])[np.maximum(labels, 0)], -9)       # labels with gaps, negatives of another value
    for kw in (dict(), dict(min_votes=2), dict(min_share=0.6)):
        got = M.lift(xyz, cams, sparse, depth, tol=TOL, ortho=ortho, near=R.SOUP_NEAR, device=DEV, **kw)
        stats = M.last_stats()
        want, _, want_stats = L.lift(xyz, cams, sparse, depth, TOL, ortho, R.SOUP_NEAR, **kw)
        for name, a, b in zip(want._fields, got, want):
            assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (kw, name)
        assert stats == want_stats and set(np.unique(got.label)) <= {-1, 3, 7, 40, 41, 65535}
    assert (got.tied > 0).any() and (got.label >= 0).sum() > 100


@pytest.mark.parametrize("C", (1, 5, 64, 65, 70, 4096))
def test_the_vote_on_random_tables(C):
    rng = np.random.RandomState(C)
    V = 1000 if C < 4096 else 130
    counts = rng.randint(0, 4, (V, C)).astype(np.int64)                          # few values: ties everywhere
    counts[rng.uniform(0, 1, (V, C)) < 0.5] = 0
    counts[::7] = 0                                                              # rows without a vote
    counts[1::7, C - 1] = 9                                                      # the last class wins
    counts[2::7, 0] = counts[2::7, C - 1] = 11                                   # the first and the last class tie
    counts[3::7] = rng.randint(0, 1 << 30, (counts[3::7].shape[0], 1)) // C      # large counts, the whole row equal
    for name, a, b in zip(("winner", "votes", "total", "tied"), _vote(counts), L.vote(counts)):
        assert np.array_equal(a, b), (C, name, int((a != b).sum()))


@pytest.mark.parametrize("V, C", ((1, 5), (3000, 1), (257, 5), (256, 3)))
def test_edge_shapes_of_the_table(soup, V, C):
    xyz = soup[0]
    pick = xyz[1500:1500 + V] if V < 3000 else xyz
    persp, _ = R.soup_cameras(SIZE)
    cams = _three(persp)
    labels, depth, _ = L.soup_images(pick, cams, SIZE, C, False, seed=V)
    want = _check(pick, cams, labels, depth, TOL, C, False, what=("V, C", V, C))
    assert want[2]["labelled"] + want[2]["visible"] > 0 or V == 1


@pytest.mark.parametrize("size", ((1, 1), (1, 4096), (4096, 1)))
def test_images_of_one_pixel_and_of_one_column(soup, size):
    rng = np.random.RandomState(12)
    middle = np.stack([rng.uniform(-0.004, 0.004, 50), rng.uniform(-0.004, 0.004, 50), rng.uniform(1.0, 3.0, 50)], 1).astype(np.float32)
    xyz = np.concatenate([soup[0], middle])                                      # 50 points on the image's middle pixel, whatever its size
    for cam, ortho in zip(R.soup_cameras(size), (False, True)):
        labels, depth, _ = L.soup_images(xyz, cam[None], size, 5, ortho, seed=3)
        want = _check(xyz, cam[None], labels, depth, TOL, 5, ortho, what=(size, ortho))
        assert want[2]["outside"] > 0 and want[2]["labelled"] + want[2]["occluded"] > 0


def test_counts_and_seen_are_added_to(soup):
    xyz, known = soup
    cams, ortho, labels, depth, clean = known["perspective", 5]
    rng = np.random.RandomState(2)
    pre_counts, pre_seen = rng.randint(0, 1000, clean[0].shape), rng.randint(0, 1000, clean[1].shape)
    want = _check(xyz, cams, labels, depth, TOL, 5, ortho, counts=pre_counts, seen=pre_seen, what="pre-filled")
    assert np.array_equal(want[0], clean[0] + pre_counts) and np.array_equal(want[1], clean[1] + pre_seen) and want[2] == clean[2]


def test_seventy_views_are_two_chunks_and_two_explicit_calls():
    import torch
    from seggroup_amd import lift as M
    rng = np.random.RandomState(6)
    size, C, B = (16, 12), 4, 70
    xyz = L.soup_points(500, 5)
    cams = np.tile(R.camera_row(np.eye(4), 4.0, 4.0, 8.0, 6.0), (B, 1))          # wide enough for most of the soup
    cams[:, 14] += rng.uniform(-3.0, 3.0, B)
    cams[:, 3] = rng.uniform(-0.5, 0.5, B)
    labels, depth, _ = L.soup_images(xyz, cams, size, C, False, seed=9)
    labels = np.where(labels >= 0, 10 * labels + 3, -1).astype(np.int32)         # labels 3, 13, 23, 33: the classes 0..3
    assert M.view_chunks(B, *size) == [(0, 64), (64, 70)]
    got = M.lift(xyz, cams, labels, depth, tol=TOL, near=R.SOUP_NEAR, device=DEV)
    stats = M.last_stats()
    want, want_counts, want_stats = L.lift(xyz, cams, labels, depth, TOL, False, R.SOUP_NEAR)
    for name, a, b in zip(want._fields, got, want):
        assert np.array_equal(a, b), name
    assert stats == want_stats and sum(stats.values()) == B * 500 and stats["labelled"] > 500
    classes = L.classes(labels)[0].astype(np.int32)
    d_xyz = torch.from_numpy(xyz).to(DEV)
    d_counts, d_seen = torch.zeros((500, C), dtype=torch.int32, device=DEV), torch.zeros(500, dtype=torch.int32, device=DEV)
    total = dict.fromkeys(L.STAT_NAMES, 0)
    for a, b in ((0, 64), (64, 70)):
        one = M.accumulate(d_xyz, np.ascontiguousarray(cams[a:b]), torch.from_numpy(classes[a:b]).to(DEV), torch.from_numpy(depth[a:b]).to(DEV), TOL,
                           d_counts, d_seen, False, R.SOUP_NEAR)
        assert one == L.accumulate(xyz, cams[a:b], classes[a:b], depth[a:b], TOL, C, False, R.SOUP_NEAR)[2]
        total = {k: total[k] + one[k] for k in total}
    assert np.array_equal(d_counts.cpu().numpy(), want_counts) and np.array_equal(d_seen.cpu().numpy(), want.seen) and total == want_stats
    chunked = _tables(xyz, cams, classes, depth, TOL, C, False)
    assert np.array_equal(chunked[0], want_counts) and np.array_equal(chunked[1], want.seen) and chunked[2] == want_stats


def test_the_same_bytes_twice_and_on_a_second_stream(soup):
    import torch
    from seggroup_amd import lift as M
    xyz, known = soup
    cams, ortho, labels, depth, want = known["perspective", 70]
    runs = [M.fuse(xyz, cams, labels, 70, depth, tol=TOL, near=R.SOUP_NEAR, device=DEV, stream=s) for s in (None, None, torch.cuda.Stream(device=DEV))]
    torch.cuda.synchronize()
    first = [t.cpu().numpy().tobytes() for t in runs[0]]
    for other in runs[1:]:
        assert [t.cpu().numpy().tobytes() for t in other] == first
    assert np.array_equal(runs[0][0].cpu().numpy(), want[0])
    a = M.lift(xyz, cams, labels, depth, tol=TOL, near=R.SOUP_NEAR, device=DEV)
    b = M.lift(xyz, cams, labels, depth, tol=TOL, near=R.SOUP_NEAR, device=DEV, stream=torch.cuda.Stream(device=DEV))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_label_of_C_raises_the_flag_and_the_other_pairs_are_counted(soup):
    import torch
    from seggroup_amd import lift as M
    xyz, known = soup
    cams, ortho, labels, depth, clean = known["orthographic", 5]
    kind, _ = L.classify(xyz, cams[1], labels[1], depth[1], TOL, 5, ortho, R.SOUP_NEAR)
    v = int(np.flatnonzero(kind == 6)[0])                                        # a labelled pair of view 1: its pixel's label becomes C
    X, Y, _, _ = R.project(xyz, cams[1], ortho, R.SOUP_NEAR)
    bad_labels = labels.copy()
    bad_labels[1, Y[v] >> 8, X[v] >> 8] = 5
    want_counts, want_seen, _, bad = L.accumulate(xyz, cams, bad_labels, depth, TOL, 5, ortho, R.SOUP_NEAR)
    assert bad >= 1 and want_counts.sum() == clean[0].sum() - bad
    with pytest.raises(ValueError, match="sg_lift: a visible pixel's label is outside the 5 classes"):
        M.fuse(xyz, cams, bad_labels, 5, depth, tol=TOL, ortho=ortho, near=R.SOUP_NEAR, device=DEV)
    assert M.call_stats() == dict.fromkeys(L.STAT_NAMES, 0)
    d_counts, d_seen = torch.zeros((3000, 5), dtype=torch.int32, device=DEV), torch.zeros(3000, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="sg_lift:"):
        M.accumulate(torch.from_numpy(xyz).to(DEV), cams, torch.from_numpy(bad_labels).to(DEV), torch.from_numpy(depth).to(DEV), TOL, d_counts, d_seen, ortho,
                     R.SOUP_NEAR)
    assert np.array_equal(d_counts.cpu().numpy(), want_counts) and np.array_equal(d_seen.cpu().numpy(), want_seen)
    _check(xyz, cams, labels, depth, TOL, 5, ortho, want=clean, what="after the refusal")      # the library is as it was


def test_refusals_name_the_entry():
    import ctypes as C

    import torch
    from seggroup_amd import hip
    lib = hip.lib()
    V, K, W, H = 100, 5, 8, 6
    xyz = torch.zeros((V, 3), dtype=torch.float32, device=DEV)
    label = torch.zeros((1, H, W), dtype=torch.int32, device=DEV)
    depth = torch.ones((1, H, W), dtype=torch.float32, device=DEV)
    counts = torch.zeros((V, K), dtype=torch.int32, device=DEV)
    seen = torch.zeros(V, dtype=torch.int32, device=DEV)
    need = lib.sg_lift_ws_bytes(V, 1)
    assert need > 0
    ws = torch.empty(max(need, lib.sg_lift_ws_bytes(V, 64)), dtype=torch.uint8, device=DEV)
    rows = np.ascontiguousarray(np.tile(R.pixel_camera(), (65, 1)))

    def call(xyz_p=xyz.data_ptr(), stride=3, n=V, B=1, cams=rows, near=0.05, w=W, h=H, label_p=label.data_ptr(), depth_p=depth.data_ptr(), tol=0.1, classes=K,
             counts_p=counts.data_ptr(), seen_p=seen.data_ptr(), ws_bytes=need):
        return lib.sg_lift(xyz_p, stride, n, B, cams.ctypes.data, 1, near, w, h, label_p, depth_p, tol, classes, counts_p, seen_p, ws.data_ptr(), ws_bytes, None)

    assert call() == hip.SG_OK
    nan_cam, zero_fy = rows.copy(), rows.copy()
    nan_cam[0, 5], zero_fy[0, 13] = np.nan, 0.0
    for kw, word in ((dict(xyz_p=None), "null"), (dict(label_p=None), "null"), (dict(depth_p=None), "null"), (dict(counts_p=None), "null"),
                     (dict(seen_p=None), "null"), (dict(stride=2), "rows of 2 floats"), (dict(classes=0), "0 classes"), (dict(n=0), "0 vertices"),
                     (dict(B=0), "0 views"), (dict(tol=-0.001), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"), (dict(near=0.0), "near"),
                     (dict(cams=nan_cam), "not finite"), (dict(cams=zero_fy), "fy = 0"), (dict(ws_bytes=need - 1), "workspace too small")):
        assert call(**kw) == hip.SG_EINVAL, kw
        msg = lib.sg_last_error().decode()
        assert msg.startswith("sg_lift:") and word in msg, (kw, msg)
    for kw, word in ((dict(B=65), "65 views"), (dict(classes=4097), "4097 classes"), (dict(w=4097), "4097"), (dict(h=4097), "4097"),
                     (dict(n=(1 << 19) + 1, classes=4096), "2^31"), (dict(n=(1 << 27) + 1), "vertices")):      # refused before anything is read
        assert call(**kw) == hip.SG_EUNSUP, kw
        msg = lib.sg_last_error().decode()
        assert msg.startswith("sg_lift:") and word in msg, (kw, msg)
    assert int(counts.sum()) == 0 and int(seen.sum()) == 0                       # the good call's vertices lie at depth 0, behind `near`: nothing was added
    assert lib.sg_lift_ws_bytes(V, 65) == 0 and lib.sg_lift_ws_bytes(0, 1) == 0 and lib.sg_lift_ws_bytes((1 << 27) + 1, 1) == 0
    assert lib.sg_lift_ws_bytes(1 << 27, 64) > 0
    h = (C.c_int64 * 7)()
    assert lib.sg_lift_stats(h, 6) == hip.SG_EINVAL and lib.sg_last_error().decode().startswith("sg_lift_stats:")
    assert lib.sg_lift_stats(h, 7) == 7
    out = [torch.empty(V, dtype=torch.int32, device=DEV) for _ in range(4)]
    ptrs = [t.data_ptr() for t in out]
    assert lib.sg_lift_vote(counts.data_ptr(), V, K, *ptrs, None) == hip.SG_OK
    for args, code in (((None, V, K, *ptrs), hip.SG_EINVAL), ((counts.data_ptr(), V, 0, *ptrs), hip.SG_EINVAL), ((counts.data_ptr(), 0, K, *ptrs), hip.SG_EINVAL),
                       ((counts.data_ptr(), V, K, ptrs[0], None, ptrs[2], ptrs[3]), hip.SG_EINVAL), ((counts.data_ptr(), V, 4097, *ptrs), hip.SG_EUNSUP),
                       ((counts.data_ptr(), (1 << 19) + 1, 4096, *ptrs), hip.SG_EUNSUP)):
        assert lib.sg_lift_vote(*args, None) == code, args
        assert lib.sg_last_error().decode().startswith("sg_lift_vote:")
    torch.cuda.synchronize()


# ---- the scan as its own occluder -------------------------------------------------------------------------------------------------------------------
SHEET_TOL = 0.02         # the sheet and its folded part lie 0.4 apart, the jitter is 0.002: anything between sees the near surface and not the far one


def test_a_folded_sheet_occludes_itself():
    from seggroup_amd import lift as M
    from seggroup_amd import render
    xyz, faces, hidden = R.folded_sheet()
    assert xyz.shape[0] == 20000 and hidden.sum() > 2000
    stripe = (np.floor(np.maximum(xyz[:, 0], 0.0) * 2.0) + 1).astype(np.int32)   # stripes of half a unit across the fold: 1..9
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    size = (320, 240)
    top = render.top_view(lo, hi, size).row()[None]
    below = np.stack([c.row() for c in render.orbit_views(lo, hi, size, 4, -50.0)])
    share = {}
    for name, cams, ortho in (("top", top, True), ("below", below, False)):
        img = R.render(xyz, faces, cams, size, ortho, 0.05, buckets=True)
        labels = np.where(img.vert >= 0, stripe[np.maximum(img.vert, 0)], -1).astype(np.int32)
        want, _, want_stats = L.lift(xyz, cams, labels, img.depth, SHEET_TOL, ortho, 0.05)
        # the conditions SHEET_TOL was chosen for, in the restatement alone
        if name == "top":
            assert (want.seen[hidden] == 0).all()                                # from above no vertex of the fold's hidden side is visible
            assert 2 * int((want.label >= 0).sum()) >= xyz.shape[0]              # at least half of the vertices get a label
        else:
            assert (want.seen[hidden] > 0).any()                                 # from below at least one is
        got = M.lift(xyz, cams, labels, None, faces, tol=SHEET_TOL, ortho=ortho, near=0.05, device=DEV)      # depth=None: sg_render's depth, on the device
        assert M.last_stats() == want_stats, (name, M.last_stats(), want_stats)
        for field, a, b in zip(want._fields, got, want):
            assert np.array_equal(a, b), (name, field, int((a != b).sum()))
        given = M.lift(xyz, cams, labels, img.depth, tol=SHEET_TOL, ortho=ortho, near=0.05, device=DEV)
        assert all(np.array_equal(a, b) for a, b in zip(given, want))
        on = got.label >= 0
        share[name] = (int(on.sum()), float((got.label[on] == stripe[on]).mean()))
    print("folded sheet: (labelled vertices, the share whose lifted label is their own stripe)", share)      # DESIGN.md 8z quotes it; not a gate


# ---- the command ------------------------------------------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    from seggroup_amd import render
    from seggroup_amd.prepare import write_ply
    rng = np.random.RandomState(8)
    scans_dir, frames_dir, plain_dir = tmp_path / "scans", tmp_path / "frames", tmp_path / "frames_no_depth"
    frames_dir.mkdir()
    plain_dir.mkdir()
    mesh_xyz, mesh_faces, _ = R.folded_sheet(40, 30, 2)
    cloud = np.stack([rng.uniform(0, 3, 5000), rng.uniform(0, 2, 5000), rng.uniform(0, 1, 5000)], 1).astype(np.float32)
    out = {}
    for name, xyz, faces in (("scene0000_00", mesh_xyz, mesh_faces), ("scene0001_00", cloud, np.zeros((0, 3), np.int32))):
        (scans_dir / name).mkdir(parents=True)
        write_ply(str(scans_dir / name / (name + "_vh_clean_2.ply")), xyz, rng.randint(0, 256, (xyz.shape[0], 3)).astype(np.uint8), faces)
        cams = render.orbit_views(xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64), (96, 64), 3, 40.0)
        T, K = np.stack([c.T for c in cams]), np.array([[c.fx, c.fy, c.cx, c.cy] for c in cams])
        img = render.render(xyz, faces if faces.shape[0] else None, cams, (96, 64), device=DEV)
        own = (np.floor(xyz[:, 0] * 2.0) * 5 + 2).astype(np.int32)               # labels with gaps: 2, 7, 12, ...
        label = np.where(img.vert >= 0, own[np.maximum(img.vert, 0)], -1).astype(np.int32)
        depth = img.depth.copy()
        depth[:, ::9, ::7] = 0.0                                                 # a sensor's holes
        np.savez(str(frames_dir / (name + ".frames.npz")), T=T, K=K, label=label, depth=depth)
        np.savez(str(plain_dir / (name + ".frames.npz")), T=T[:, :3], K=K, label=label)
        seg = (np.floor(np.maximum(xyz[:, 0], 0.0) * 4.0) * 10 + np.floor(np.maximum(xyz[:, 1], 0.0) * 4.0)).astype(np.int64)      # patches of a quarter unit
        with open(str(scans_dir / name / (name + "_vh_clean_2.0.010000.segs.json")), "w") as f:
            json.dump({"segIndices": seg.tolist()}, f)
        out[name] = (xyz, faces, M_rows(cams), label, depth, seg)
    return str(scans_dir), str(frames_dir), str(plain_dir), out


def M_rows(cams):
    return np.stack([c.row() for c in cams])


def _same_npz(path, want, extra=()):
    with np.load(path) as z:
        got = {k: z[k] for k in z.files}
    assert sorted(got) == sorted(want._fields + tuple(extra)), sorted(got)
    for name, b in zip(want._fields, want):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], b), (path, name)
    return got


def test_the_command_on_a_mesh_and_a_faceless_scan(tmp_path, capsys):
    from seggroup_amd import labels as labels_module
    from seggroup_amd import lift as M
    from seggroup_amd.geodesic import snap_to_segments
    scans_dir, frames_dir, plain_dir, scenes = _tree(tmp_path)
    out, root = str(tmp_path / "out"), str(tmp_path / "root")
    args = ["--scans", scans_dir, "--out", out, "--frames", frames_dir, "--tol", "0.03", "--min-votes", "2", "--snap", "--style-name", "lifted", "--root", root,
            "--as", "ins", "--workers", "2", "--device", DEV]
    assert M.main(args) == 0
    assert "2 written, 0 skipped" in capsys.readouterr().out
    report = json.load(open(os.path.join(out, "lift_report.json")))
    assert report["skipped"] == [] and sorted(report["scenes"]) == sorted(scenes) and report["parameters"]["tol"] == 0.03 and report["parameters"]["as"] == "ins"
    for name, (xyz, faces, rows, label, depth, seg) in scenes.items():
        want = M.lift(xyz, rows, label, depth, tol=0.03, min_votes=2, device=DEV)
        stats = M.last_stats()
        got = _same_npz(os.path.join(out, name + ".lift.npz"), want, ("label_snapped",))
        snapped, moved = snap_to_segments(seg, want.label, device=DEV)
        assert np.array_equal(got["label_snapped"], snapped)
        entry = report["scenes"][name]
        assert {k: entry[k] for k in L.STAT_NAMES} == stats and sum(stats.values()) == 3 * xyz.shape[0] and entry["moved"] == moved
        assert entry["views"] == 3 and entry["views_skipped"] == 0 and entry["vertices"] == xyz.shape[0] and entry["occluder"] == "depth images"
        assert entry["vertices_seen"] == int((want.seen > 0).sum()) > 0 and entry["vertices_labelled"] == int((want.label >= 0).sum()) > 100
        assert entry["vertices_tied"] == int((want.tied > 0).sum()) and "sem.txt is -1 throughout" in entry["style"] and entry["resampled"].startswith("not written")
        raw = os.path.join(root, "label", "seg", "lifted", "raw", name)
        assert np.array_equal(np.array(labels_module.load_labels(os.path.join(raw, name + ".ins.txt"))), snapped)
        assert (np.array(labels_module.load_labels(os.path.join(raw, name + ".sem.txt"))) == -1).all()
    assert M.main(args) == 0                                                      # every .npz is there: nothing is lifted again
    assert "0 written, 2 skipped" in capsys.readouterr().out
    plain = str(tmp_path / "plain")                                               # no depth in the file: the scan occludes itself
    assert M.main(["--scans", scans_dir, "--out", plain, "--frames", plain_dir, "--tol", "0.03", "--device", DEV]) == 0
    rep = json.load(open(os.path.join(plain, "lift_report.json")))
    for name, (xyz, faces, rows, label, depth, seg) in scenes.items():
        mesh = faces.shape[0] > 0
        want = M.lift(xyz, rows, label, None, faces if mesh else None, tol=0.03, device=DEV)
        stats = M.last_stats()
        _same_npz(os.path.join(plain, name + ".lift.npz"), want)
        assert rep["scenes"][name]["occluder"] == ("the scan's faces" if mesh else "the scan, as splats")
        assert {k: rep["scenes"][name][k] for k in L.STAT_NAMES} == stats and rep["scenes"][name]["vertices_labelled"] > 100


def test_the_command_on_a_scannet_shaped_tree(tmp_path, capsys):
    from seggroup_amd import labels as labels_module
    from seggroup_amd import lift as M
    from seggroup_amd.prepare import write_ply
    rng = np.random.RandomState(4)
    name = "scene0000_00"
    frames_root = tmp_path / "frames"
    scene_dir, _, _ = L.scannet_tree(frames_root, name)
    xyz = np.stack([rng.uniform(-0.6, 0.6, 800), rng.uniform(-0.5, 0.5, 800), rng.uniform(0.5, 3.0, 800)], 1).astype(np.float32)
    (tmp_path / "scans" / name).mkdir(parents=True)
    write_ply(str(tmp_path / "scans" / name / (name + "_vh_clean_2.ply")), xyz, np.zeros((800, 3), np.uint8), np.zeros((0, 3), np.int32))
    out, root = str(tmp_path / "out"), str(tmp_path / "root")
    assert M.main(["--scans", str(tmp_path / "scans"), "--out", out, "--scannet-frames", str(frames_root), "--image-kind", "instance-filt", "--every", "2",
                   "--tol", "0.5", "--style-name", "lifted2d", "--root", root, "--as", "sem", "--device", DEV]) == 0
    assert "1 written, 0 skipped" in capsys.readouterr().out
    fr = M.load_scannet_frames(scene_dir, "instance-filt", 2)
    assert fr.used == ["0", "11"] and fr.skipped == ["2"]
    want = M.lift(xyz, fr.rows, fr.label, fr.depth, tol=0.5, device=DEV)
    stats = M.last_stats()
    ref, _, ref_stats = L.lift(xyz, fr.rows, fr.label, fr.depth, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(want, ref)) and stats == ref_stats and stats["labelled"] > 50 and stats["nodepth"] >= 0
    _same_npz(os.path.join(out, name + ".lift.npz"), want)
    entry = json.load(open(os.path.join(out, "lift_report.json")))["scenes"][name]
    assert entry["views"] == 2 and entry["views_skipped"] == 1 and {k: entry[k] for k in L.STAT_NAMES} == stats and entry["image"] == [8, 6]
    raw = os.path.join(root, "label", "seg", "lifted2d", "raw", name)
    assert np.array_equal(np.array(labels_module.load_labels(os.path.join(raw, name + ".sem.txt"))), want.label)
    assert (np.array(labels_module.load_labels(os.path.join(raw, name + ".ins.txt"))) == -1).all()
