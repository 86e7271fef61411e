"""The restatement of sg_render's rule (tests/render_ref.py) on cases worked out by hand, and the host side of seggroup_amd/render.py: the
view helpers, the PNG writer, the contact sheet and the command's refusals.  No GPU: nothing here makes a device call."""
import os

import numpy as np
import pytest

import render_ref as R
from seggroup_amd import render as M

CAM = R.pixel_camera()                  # orthographic: world x, y are pixels, depth is world z
SIZE = (8, 6)
# a right triangle with its corners on the centres of pixels (0,0), (4,0), (0,4)
TRI = np.array([[0.5, 0.5, 2.0], [4.5, 0.5, 2.0], [0.5, 4.5, 2.0]], np.float32)
F0 = np.array([[0, 1, 2]], np.int32)


def _draw(xyz, faces, size=SIZE, cam=CAM, ortho=True, near=0.05, **kw):
    return R.render(np.asarray(xyz, np.float32), None if faces is None else np.asarray(faces, np.int32), cam, size, ortho, near, **kw)


def _pixels(img, b=0):
    py, px = np.nonzero(img.prim[b] >= 0)
    return set(zip(px.tolist(), py.tolist()))


def _fixed(xyz):
    return [(int(np.floor(float(x) * 256.0 + 0.5)), int(np.floor(float(y) * 256.0 + 0.5))) for x, y, _ in np.asarray(xyz, np.float32)]


def test_a_triangle_on_pixel_centres_covers_its_edges_too():
    img = _draw(TRI, F0)
    want = {(px, py) for px in range(5) for py in range(5) if px + py <= 4}          # the hypotenuse's five centres included
    assert _pixels(img) == want == R.covered_exact(_fixed(TRI), *SIZE)
    assert img.stats == dict(kept=1, behind=0, far=0, degenerate=0, large=0, covered=15)
    assert (img.depth[0][img.prim[0] >= 0] == np.float32(2.0)).all() and np.isinf(img.depth[0][img.prim[0] < 0]).all()
    assert (img.vert[0][img.prim[0] < 0] == -1).all()


def test_a_corner_moved_by_one_subpixel_step_loses_the_column():
    """the vertical edge one 1/256 pixel to the right of the centres of column 0: the column is out, the hypotenuse's centres stay in"""
    xyz = TRI.copy()
    xyz[[0, 2], 0] += 1.0 / 256.0
    want = {(px, py) for px in range(1, 5) for py in range(5) if px + py <= 4}
    assert len(want) == 10
    assert _pixels(_draw(xyz, F0)) == want == R.covered_exact(_fixed(xyz), *SIZE)


def test_random_subpixel_triangles_agree_with_the_exact_rationals():
    rng = np.random.RandomState(5)
    for _ in range(40):
        xyz = np.concatenate([rng.randint(-256, 9 * 256, (3, 2)) / 256.0, np.full((3, 1), 1.0)], 1).astype(np.float32)
        assert _pixels(_draw(xyz, F0)) == R.covered_exact(_fixed(xyz), *SIZE)


def _two(z0, z1):
    """two triangles that share the hypotenuse of TRI, with corners of their own: depths z0 and z1"""
    other = np.array([[4.5, 0.5, z1], [4.5, 4.5, z1], [0.5, 4.5, z1]], np.float32)
    first = TRI.copy()
    first[:, 2] = z0
    return np.concatenate([first, other]), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def test_a_centre_on_a_shared_edge_goes_to_the_nearer_then_to_the_lower_index():
    edge = [(4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
    for z0, z1, winner in ((2.0, 1.0, 1), (1.0, 2.0, 0), (1.5, 1.5, 0)):
        img = _draw(*_two(z0, z1))
        assert [int(img.prim[0, py, px]) for px, py in edge] == [winner] * 5, (z0, z1)
        assert all(img.depth[0, py, px] == np.float32(min(z0, z1)) for px, py in edge)
        assert img.prim[0, 1, 1] == 0 and img.prim[0, 3, 3] == 1                     # off the edge each keeps its own


def test_both_orientations_give_the_same_image():
    xyz, faces = R.pixel_lattice()
    a, b = _draw(xyz, faces, (33, 33)), _draw(xyz, faces[:, [0, 2, 1]], (33, 33))
    assert np.array_equal(a.prim, b.prim) and np.array_equal(a.depth.view(np.uint32), b.depth.view(np.uint32))
    assert a.stats == b.stats and np.array_equal(a.vert >= 0, b.vert >= 0)
    # `vert` is the same vertex wherever the winner's three w_i are distinct (where two tie, the lower corner POSITION wins, and the positions swapped)
    X, Y, _, _ = R.project(xyz, CAM, True, 0.05)
    py, px = np.nonzero(a.prim[0] >= 0)
    f = faces[a.prim[0][py, px]].astype(np.int64)
    w0, w1, w2, _ = R._edges([X[f[:, i]] for i in range(3)], [Y[f[:, i]] for i in range(3)], 256 * px.astype(np.int64) + 128, 256 * py.astype(np.int64) + 128)
    distinct = (w0 != w1) & (w1 != w2) & (w0 != w2)
    assert 100 < distinct.sum() < distinct.size
    assert np.array_equal(a.vert[0][py, px][distinct], b.vert[0][py, px][distinct])
    assert (a.vert[0][py, px][distinct] == f[np.arange(f.shape[0]), np.argmax(np.stack([w0, w1, w2], 1), 1)][distinct]).all()


def test_a_triangle_of_no_area_is_degenerate():
    line = np.array([[0.5, 0.5, 1.0], [2.5, 2.5, 1.0], [4.5, 4.5, 1.0]], np.float32)
    for faces in (F0, np.array([[0, 1, 0]], np.int32)):
        img = _draw(line, faces)
        assert img.stats == dict(kept=0, behind=0, far=0, degenerate=1, large=0, covered=0) and (img.prim == -1).all()


def test_a_vertex_at_near_drops_the_face_as_behind():
    xyz = TRI.copy()
    xyz[1, 2] = 0.5
    assert _draw(xyz, F0, near=0.5).stats == dict(kept=0, behind=1, far=0, degenerate=0, large=0, covered=0)
    assert _draw(xyz, F0, near=0.49).stats["kept"] == 1
    xyz[2, 0] = 20000.0                                                              # behind AND far: counted as behind
    assert _draw(xyz, F0, near=0.5).stats["behind"] == 1
    xyz[1, 2] = np.nan
    assert _draw(xyz, F0).stats["behind"] == 1


def test_the_guard_band_is_16384_pixels_inclusive():
    xyz = TRI.copy()
    xyz[1, 0] = 16385.0
    assert _draw(xyz, F0).stats == dict(kept=0, behind=0, far=1, degenerate=0, large=0, covered=0)
    xyz[1, 0] = 16384.0
    img = _draw(xyz, F0)
    assert img.stats["far"] == 0 and img.stats["kept"] == 1 and img.stats["covered"] > 0
    xyz[1, 0] = -16384.0
    assert _draw(xyz, F0).stats["far"] == 0
    xyz[1, 0] = -16384.5
    assert _draw(xyz, F0).stats["far"] == 1


def test_perspective_depth_is_the_harmonic_interpolation():
    """screen corners (0.5, 0.5), (8.5, 0.5), (0.5, 8.5) at depths 1, 4, 4: the centre of pixel (4, 0) is the screen midpoint of the first edge"""
    xyz = np.array([[0.5, 0.5, 1.0], [34.0, 2.0, 4.0], [2.0, 34.0, 4.0]], np.float32)
    cam = R.camera_row(np.eye(4), 1.0, 1.0, 0.0, 0.0)
    img = _draw(xyz, F0, (10, 10), cam, ortho=False)
    assert img.prim[0, 0, 4] == 0
    assert img.depth[0, 0, 4] == np.float32(1.0 / (0.5 / 1.0 + 0.5 / 4.0)) == np.float32(1.6)
    assert img.depth[0, 0, 4] != np.float32(2.5)                                     # the linear one
    assert img.depth[0, 0, 0] == np.float32(1.0)


def test_orthographic_and_perspective_agree_on_a_fronto_parallel_triangle():
    xyz = TRI.copy()
    xyz[:, 2] = 2.0
    o = _draw(xyz, F0)
    p = _draw(xyz, F0, cam=R.camera_row(np.eye(4), 2.0, 2.0, 0.0, 0.0), ortho=False)
    for a, b in zip(o[:4], p[:4]):
        assert np.array_equal(a, b)
    assert o.stats == p.stats


def test_splats_at_a_corner_are_clipped():
    pts = np.array([[0.5, 0.5, 1.0]], np.float32)
    for side, want in ((1, 1), (3, 4), (15, 48)):
        img = _draw(pts, None, point_size=side)
        assert img.stats["covered"] == want == int(img.hits[0]) and img.stats["kept"] == 1, side     # 15: 8 columns x 6 rows of the 8 x 6 image
        assert (img.prim[0][:min(side // 2 + 1, 6), :side // 2 + 1] == 0).all()
    outside = np.array([[-0.5, 2.5, 1.0]], np.float32)                               # centred on pixel (-1, 2): arithmetic shift
    assert _pixels(_draw(outside, None, point_size=1)) == set()
    assert _pixels(_draw(outside, None, point_size=3)) == {(0, 1), (0, 2), (0, 3)}
    two = np.array([[2.5, 2.5, 1.0], [2.5, 2.5, 1.0], [2.5, 2.5, 0.5]], np.float32)   # coincident: the lower index; nearer: the depth
    assert _draw(two[:2], None, point_size=3).prim[0, 2, 2] == 0 and _draw(two, None, point_size=3).prim[0, 2, 2] == 2


def test_hits_sum_to_the_covered_pixels():
    xyz, faces = R.soup(300, 1)
    persp, ortho = R.soup_cameras()
    for cam, o in ((persp, False), (ortho, True)):
        img = _draw(xyz, faces, (67, 45), np.stack([cam, cam]), o, R.SOUP_NEAR)
        assert int(img.hits.sum()) == img.stats["covered"] == int((img.vert >= 0).sum()) == int((img.prim >= 0).sum()) > 0


def test_vert_ties_go_to_the_lower_corner_position():
    xyz = np.zeros((6, 3), np.float32)
    xyz[[5, 3, 4]] = TRI                                                             # corners 0, 1, 2 are the vertices 5, 3, 4
    img = _draw(xyz, np.array([[5, 3, 4]], np.int32))
    assert img.vert[0, 0, 2] == 5                                                    # the middle of the edge 0-1: w_0 == w_1 > w_2 = 0
    assert img.vert[0, 2, 2] == 3                                                    # the middle of the hypotenuse: w_1 == w_2 > w_0 = 0
    assert img.vert[0, 0, 0] == 5 and img.vert[0, 0, 4] == 3 and img.vert[0, 4, 0] == 4


def test_the_soup_holds_every_kind_and_the_buckets_equal_the_loop():
    xyz, faces = R.soup()
    for cam, o in zip(R.soup_cameras(), (False, True)):
        a = _draw(xyz, faces, (67, 45), cam, o, R.SOUP_NEAR)
        b = _draw(xyz, faces, (67, 45), cam, o, R.SOUP_NEAR, buckets=True)
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        assert a.stats == b.stats
        s = a.stats
        assert s["behind"] > 10 and s["far"] > 10 and s["degenerate"] > 5 and s["large"] > 5 and s["kept"] > 1000, s
        assert 0.3 * 67 * 45 < s["covered"] <= 67 * 45


# ---- the view helpers ---------------------------------------------------------------------------------------------------------------------------
LO, HI = np.array([-1.0, 2.0, 0.5]), np.array([3.0, 4.5, 2.5])


def _corner_pixels(cam, ortho):
    c = M._corners(LO, HI) @ cam.T[:, :3].T + cam.T[:, 3]
    a = c[:, :2] if ortho else c[:, :2] / c[:, 2:3]
    return a * [cam.fx, cam.fy] + [cam.cx, cam.cy], c[:, 2]


def test_look_at_is_a_rotation_that_looks_along_z():
    T = M.look_at([1.0, -2.0, 3.0], [0.0, 0.5, 1.0])
    Rm = T[:, :3]
    assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(Rm), 1.0)
    c = Rm @ np.array([0.0, 0.5, 1.0]) + T[:, 3]
    assert np.allclose(c[:2], 0.0, atol=1e-12) and c[2] > 0                          # the target on the axis, in front
    up = Rm @ np.array([1.0, -2.0, 4.0]) + T[:, 3]                                   # a point above the eye is up the image: y negative
    assert up[1] < 0
    with pytest.raises(ValueError, match="look_at"):
        M.look_at([0, 0, 0], [0, 0, 1])
    with pytest.raises(ValueError, match="look_at"):
        M.look_at([0, 0, 0], [0, 0, 0])


def test_top_view_and_orbit_views_hold_the_box():
    size = (320, 240)
    cam = M.top_view(LO, HI, size)
    uv, z = _corner_pixels(cam, True)
    assert (uv >= 0).all() and (uv[:, 0] <= 320).all() and (uv[:, 1] <= 240).all() and (z > 0.05).all()
    assert np.isclose(uv[:, 0].min(), 16.0) or np.isclose(uv[:, 1].min(), 12.0)      # fitted: one axis reaches the margin
    assert np.allclose(cam.T[:, :3], [[1, 0, 0], [0, -1, 0], [0, 0, -1]])            # x right, world y up the image, looking down
    for el in (30.0, -40.0, 0.0, 89.0):
        views = M.orbit_views(LO, HI, size, 5, el)
        assert len(views) == 5
        for v in views:
            uv, z = _corner_pixels(v, False)
            assert (uv >= -1e-9).all() and (uv[:, 0] <= 320 + 1e-9).all() and (uv[:, 1] <= 240 + 1e-9).all() and (z > 0.05).all()
            eye = -v.T[:, :3].T @ v.T[:, 3]
            assert np.isclose(np.sign(eye[2] - 1.5), np.sign(el)) or el == 0.0
    for v in M.orbit_views(LO, HI, size, 2, 20.0, ortho=True):
        uv, _ = _corner_pixels(v, True)
        assert (uv >= -1e-9).all() and (uv[:, 0] <= 320 + 1e-9).all() and (uv[:, 1] <= 240 + 1e-9).all()
    one = M.orbit_views(LO, LO, size, 1)[0]                                          # a box of one point
    assert np.isfinite(one.row()).all() and one.fx > 0
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="orbit"):
            M.orbit_views(LO, HI, size, bad)
    with pytest.raises(ValueError, match="elevation"):
        M.orbit_views(LO, HI, size, 2, 90.0)


def test_from_pose_inverts_the_pose():
    rng = np.random.RandomState(0)
    q, _ = np.linalg.qr(rng.randn(3, 3))
    q *= np.sign(np.linalg.det(q))
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = q, [1.0, -2.0, 0.5]
    K = np.array([[577.87, 0, 319.5, 0], [0, 577.87, 239.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    cam = M.from_pose(P, K)
    T4 = np.concatenate([cam.T, [[0, 0, 0, 1]]])
    assert np.allclose(T4 @ P, np.eye(4), atol=1e-12) and np.allclose(P @ T4, np.eye(4), atol=1e-12)
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (577.87, 577.87, 320.0, 240.0)        # K's centres on whole numbers, ours on halves
    assert M.from_pose(P, K[:3, :3]) [1:] == cam[1:] and M.from_pose(P, [577.87, 577.87, 319.5, 239.5])[1:] == cam[1:]
    assert M.camera_rows(cam).shape == (1, 16) and np.array_equal(M.camera_rows(cam)[0], R.camera_row(cam.T, *cam[1:]))
    with pytest.raises(ValueError, match="from_pose"):
        M.from_pose(np.eye(3), K)


def test_camera_rows_refuses_what_the_library_would():
    good = R.pixel_camera()
    assert M.camera_rows(good[None]).shape == (1, 16)
    for bad, word in ((np.r_[good[:12], 0.0, 1.0, 0.0, 0.0][None], "fx or fy"), (np.r_[np.nan, good[1:]][None], "not finite"),
                      (np.zeros((65, 16)) + 1.0, "65 views"), (np.zeros((1, 12)), "16"), ([], "cameras=")):
        with pytest.raises(ValueError, match=word):
            M.camera_rows(bad)


# ---- images ---------------------------------------------------------------------------------------------------------------------------------------
def test_write_png_round_trips_both_formats(tmp_path):
    rng = np.random.RandomState(1)
    rgb = rng.randint(0, 256, (13, 31, 3)).astype(np.uint8)
    grey = rng.randint(0, 65536, (7, 5)).astype(np.uint16)
    grey[0, :2] = [0, 65535]
    for name, img in (("rgb.png", rgb), ("grey.png", grey), ("one.png", rgb[:1, :1]), ("flat.png", np.zeros((64, 64, 3), np.uint8))):
        path = str(tmp_path / name)
        M.write_png(path, img)
        back = R.read_png(path)
        assert back.dtype == img.dtype and np.array_equal(back, img), name
        assert not os.path.exists(path + ".tmp")
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(path)).astype(img.dtype), img), name
    for bad in (rgb.astype(np.float32), rgb[:, :, :2], grey.astype(np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="write_png"):
            M.write_png(str(tmp_path / "bad.png"), bad)


def test_depth_in_millimetres():
    d = np.array([[0.0, 1.2344, 1.2346, 65.5351, 70.0, np.inf]], np.float32)
    assert M.depth_mm(d).tolist() == [[0, 1234, 1235, 65535, 65535, 0]] and M.depth_mm(d).dtype == np.uint16


def test_contact_sheet_shapes():
    tiles = [np.full((4, 6, 3), k, np.uint8) for k in range(5)]
    s = M.contact_sheet(tiles, 2)
    assert s.shape == (12, 12, 3) and s.dtype == np.uint8
    assert (s[4:8, 6:12] == 3).all() and (s[8:12, 0:6] == 4).all() and (s[8:12, 6:12] == 255).all()
    assert M.contact_sheet(tiles, 5).shape == (4, 30, 3) and M.contact_sheet(tiles, 9).shape == (4, 54, 3) and M.contact_sheet(tiles[:1], 1).shape == (4, 6, 3)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="--sheet"):
            M.contact_sheet(tiles, bad)
    with pytest.raises(ValueError, match="contact_sheet"):
        M.contact_sheet(tiles + [np.zeros((4, 5, 3), np.uint8)], 2)


# ---- the command's refusals: all before the device is asked for ----------------------------------------------------------------------------------
BASE = ["--scans", "nowhere", "--out", "nowhere"]
REFUSALS = [
    ([], "exactly one source of colours"),
    (["--rgb", "-n", "exp"], "exactly one source of colours"),
    (["--rgb", "--labels-from", "d", "--suffix", ".npy", "--label-type", "instance"], "exactly one source of colours"),
    (["--rgb", "--stage", "epoch_last"], "--stage, --layer and --root belong"),
    (["--rgb", "--label-type", "instance"], "--suffix, --key and --label-type belong"),
    (["-n", "exp", "--layer", "final.foo"], "--layer names an exported vector"),
    (["--labels-from", "d", "--label-type", "instance"], "--labels-from needs --suffix"),
    (["--labels-from", "d", "--suffix", ".npz", "--label-type", "instance"], "--key names the array"),
    (["--labels-from", "d", "--suffix", ".npy", "--key", "k", "--label-type", "instance"], "--key names the array"),
    (["--labels-from", "d", "--suffix", ".npy"], "--label-type is needed"),
    (["--labels-from", "d", "--suffix", ".npy", "--label-type", "colour"], "--label-type is needed"),
    (["--rgb", "--views", "orbit:0"], "--views orbit:N"),
    (["--rgb", "--views", "orbit:65"], "--views orbit:N"),
    (["--rgb", "--views", "orbit:x"], "--views orbit:N"),
    (["--rgb", "--views", "side"], "--views is top, orbit:N or poses:FILE.npz"),
    (["--rgb", "--size", "0", "480"], "--size"),
    (["--rgb", "--size", "4097", "480"], "--size"),
    (["--rgb", "--size", "640", "4097"], "--size"),
    (["--rgb", "--views", "orbit:64", "--size", "2048", "1024"], "--size.*2\\^26"),
    (["--rgb", "--point-size", "4"], "--point-size"),
    (["--rgb", "--point-size", "17"], "--point-size"),
    (["--rgb", "--point-size", "-1"], "--point-size"),
    (["--rgb", "--sheet", "0"], "--sheet"),
    (["--rgb", "--near", "0"], "--near"),
    (["--rgb", "--near", "inf"], "--near"),
    (["--rgb", "--views", "orbit:2", "--elevation", "90"], "--elevation"),
    (["--rgb", "--workers", "0"], "--workers"),
]


@pytest.mark.parametrize("args, message", REFUSALS, ids=[" ".join(a) or "nothing" for a, _ in REFUSALS])
def test_the_command_refuses_before_any_device_work(args, message, capsys, monkeypatch):
    from seggroup_amd import hip

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the refusal")

    monkeypatch.setattr(hip, "require_device", no_device)
    monkeypatch.setattr(hip, "lib", no_device)
    with pytest.raises(SystemExit) as e:
        M.main(BASE + args)
    assert e.value.code == 2
    import re
    assert re.search(message, capsys.readouterr().err), args


def test_pose_files_are_checked_on_the_host(tmp_path):
    good = str(tmp_path / "poses.npz")
    T = np.tile(np.eye(4)[None], (3, 1, 1))
    np.savez(good, T=T, K=np.tile([500.0, 500.0, 320.0, 240.0], (3, 1)))
    p = M.check_command(rgb=True, views="poses:" + good)
    assert p["views"] == 3 and p["view_names"] == ["pose0", "pose1", "pose2"] and len(p["cameras"]) == 3 and not p["ortho"]
    np.savez(good, T=T[:, :3], K=np.tile([500.0, 500.0, 320.0, 240.0], (3, 1)))
    assert M.check_command(rgb=True, views="poses:" + good, ortho=True)["ortho"]
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, T=T, K=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="--views poses:"):
        M.check_command(rgb=True, views="poses:" + bad)
    np.savez(bad, T=T)
    with pytest.raises(ValueError, match="needs the arrays T and K"):
        M.check_command(rgb=True, views="poses:" + bad)
    top = M.check_command(rgb=True)
    assert top["ortho"] and top["view_names"] == ["top"] and top["vectors"] == ["rgb"] and top["size"] == (640, 480)
    exp = M.check_command(exp="e", layers=["final.ins", "layer_2.seg"], views="orbit:4")
    assert exp["vectors"] == ["final.ins", "layer_2.seg"] and exp["view_names"] == ["orbit0", "orbit1", "orbit2", "orbit3"] and not exp["ortho"]
    assert M.check_command(exp="e")["vectors"] == ["final.ins"] and M.check_command(exp="e")["stage"] == "epoch_last"
