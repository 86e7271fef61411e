"""sg_render on the GPU (seggroup_amd/render.py) against tests/render_ref.py: prim, the bits of depth, vert, hits and the six
counts EQUAL to the restatement -- the rule is exact and order-free, so no tolerance appears anywhere --, the refusals, sg_render_colour
against visualize's palette, and the command on a two-scene tree."""
import json
import os

import numpy as np
import pytest

import render_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (67, 45)                          # no multiple of a wave, of the 16 x 16 tile or of the small-primitive threshold


def _same(got, want, what=""):
    for name, a, b in (("prim", got.prim, want.prim), ("depth", got.depth.view(np.uint32), want.depth.view(np.uint32)), ("vert", got.vert, want.vert),
                       ("hits", got.hits, want.hits)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.argwhere(a != b)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:6].tolist(), a[tuple(bad[:6].T)].tolist(), b[tuple(bad[:6].T)].tolist())


def _check(xyz, faces, cams, size, ortho=False, near=R.SOUP_NEAR, point_size=3, want=None, what="", stream=None):
    """one call against the restatement, the six counts included -> (result, stats)"""
    from seggroup_amd import render as M
    got = M.render(xyz, faces, cams, size, ortho, near, point_size, device=DEV, stream=stream)
    stats = M.last_stats()
    if want is None:
        want = R.render(xyz, faces, cams, size, ortho, near, point_size, buckets=True)
    _same(got, want, what)
    assert stats == want.stats, (what, stats, want.stats)
    print(what, stats)
    return got, stats


@pytest.fixture(scope="module")
def soup():
    """the soup and its restatements, once: {"perspective" | "orthographic": (camera row, ortho, Image)}"""
    xyz, faces = R.soup()
    known = {name: (cam, o, R.render(xyz, faces, cam, SIZE, o, R.SOUP_NEAR, buckets=True)) for name, cam, o in
             zip(("perspective", "orthographic"), R.soup_cameras(SIZE), (False, True))}
    return xyz, faces, known


@pytest.mark.parametrize("projection", ("perspective", "orthographic"))
def test_a_soup_of_1500_triangles_of_every_kind(soup, projection):
    xyz, faces, known = soup
    cam, ortho, want = known[projection]
    s = want.stats
    assert s["behind"] > 10 and s["far"] > 10 and s["degenerate"] > 5 and s["large"] > 5 and s["covered"] > 1000      # both paths and every count
    _check(xyz, faces, cam, SIZE, ortho, want=want, what=projection)
    wide = np.concatenate([xyz, np.full((xyz.shape[0], 3), np.nan, np.float32)], 1)      # rows of 6 floats: only the first three are read
    _check(wide, faces, cam, SIZE, ortho, want=want, what=projection + ", stride 6")


def test_the_same_bytes_twice_and_on_a_second_stream(soup):
    import torch
    from seggroup_amd import render as M
    xyz, faces, known = soup
    cam, ortho, want = known["perspective"]
    first = M.render(xyz, faces, cam, SIZE, ortho, R.SOUP_NEAR, device=DEV)
    again = M.render(xyz, faces, cam, SIZE, ortho, R.SOUP_NEAR, device=DEV)
    other = M.render(xyz, faces, cam, SIZE, ortho, R.SOUP_NEAR, device=DEV, stream=torch.cuda.Stream(device=DEV))
    for a in (again, other):
        for x, y in zip(first, a):
            assert x.tobytes() == y.tobytes()
    _same(first, want)


def test_three_views_in_one_call_are_three_calls(soup):
    from seggroup_amd import render as M
    xyz, faces, known = soup
    cam = known["perspective"][0]
    cams = np.stack([cam, cam, cam])
    cams[1, 14] += 11.25                                                         # cx: the image shifted by a fraction of a pixel grid
    cams[2, 3], cams[2, 11] = 0.7, 0.5                                           # the camera moved sideways and back
    all3 = M.render(xyz, faces, cams, SIZE, False, R.SOUP_NEAR, device=DEV)
    stats3 = M.last_stats()
    hits, total = np.zeros_like(all3.hits), dict.fromkeys(stats3, 0)
    for b in range(3):
        one, s = _check(xyz, faces, cams[b], SIZE, what="view %d" % b)
        for name in ("prim", "depth", "vert"):
            assert getattr(one, name)[0].tobytes() == getattr(all3, name)[b].tobytes(), (b, name)
        hits += one.hits
        total = {k: total[k] + s[k] for k in total}
    assert np.array_equal(all3.hits, hits) and stats3 == total


def test_centres_on_edges_and_on_corners_shared_by_six():
    xyz, faces = R.pixel_lattice()
    assert faces.shape[0] == 200
    img, stats = _check(xyz, faces, R.pixel_camera(), (33, 33), ortho=True, what="lattice")
    assert stats["covered"] == 31 * 31 and stats["kept"] == 200                  # the centres 0.5 .. 30.5, the lattice's rim included
    _check(xyz, faces[::-1].copy(), R.pixel_camera(), (33, 33), ortho=True, what="lattice, faces reversed")
    _check(xyz, faces[:, [0, 2, 1]].copy(), R.pixel_camera(), SIZE, ortho=True, what="lattice, clockwise")


def test_two_coincident_copies_the_lower_face_index_wins():
    xyz, faces = R.pixel_lattice()
    F = faces.shape[0]
    once, _ = _check(xyz, faces, R.pixel_camera(), (33, 33), ortho=True, what="once")
    twice, stats = _check(xyz, np.concatenate([faces, faces]), R.pixel_camera(), (33, 33), ortho=True, what="twice")
    assert twice.prim.max() < F and stats["kept"] == 2 * F
    for a, b in zip(once, twice):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size", ((1, 1), (1, 4096), (4096, 1)))
def test_images_of_one_pixel_and_of_one_column(size):
    xyz, faces = R.soup(400, 7)
    persp, ortho = R.soup_cameras(size)
    _, s = _check(xyz, faces, persp, size, what=("perspective", size))
    _check(xyz, faces, ortho, size, ortho=True, what=("orthographic", size))
    assert s["covered"] >= 1 and (max(size) == 1 or s["large"] > 0)


def test_splats_of_every_size_some_coincident():
    rng = np.random.RandomState(11)
    xyz = np.stack([rng.uniform(-1.2, 1.2, 3000), rng.uniform(-0.9, 0.9, 3000), rng.uniform(0.02, 3.0, 3000)], 1).astype(np.float32)
    xyz[1000:1200] = xyz[:200]                                                   # coincident: the lower index wins
    xyz[1200:1300, :2] = xyz[200:300, :2]                                        # the same pixel, another depth
    xyz[2990:] = [[5000.0, 0.0, 1.0]] * 5 + [[0.0, 0.0, np.inf]] * 5             # beyond the guard band; not finite
    persp, ortho = R.soup_cameras(SIZE)
    for side in (1, 3, 15):
        got, stats = _check(xyz, None, persp, SIZE, point_size=side, what=("splats", side))
        assert stats["far"] >= 5 and stats["behind"] >= 5 and stats["large"] == 0 and stats["degenerate"] == 0
        assert not np.isin(got.prim, np.arange(1000, 1200)).any() and np.array_equal(got.prim, got.vert)
    _check(xyz, np.zeros((0, 3), np.int32), ortho, SIZE, ortho=True, point_size=3, what="splats, orthographic, faces of no rows")
    none = np.array([[0.0, 0.0, -1.0], [9000.0, 0.0, 1.0]], np.float32)          # no point in view: SG_OK and an empty image
    got, stats = _check(none, None, persp, SIZE, what="nothing in view")
    assert (got.prim == -1).all() and np.isinf(got.depth).all() and (got.hits == 0).all() and stats["covered"] == 0


def test_refusals_name_the_entry():
    import ctypes as C

    import torch
    from seggroup_amd import hip
    from seggroup_amd import render as M
    xyz, faces = R.pixel_lattice()
    V = xyz.shape[0]
    cam = R.pixel_camera()
    for bad in (V, -1):
        f = faces.copy()
        f[17, 1] = bad
        with pytest.raises(ValueError, match="sg_render: a face names a vertex outside 0..%d" % (V - 1)):
            M.render(xyz, f, cam, (33, 33), True, device=DEV)
    _check(xyz, faces, cam, (33, 33), ortho=True, what="after the refusals")    # the library is as it was
    lib = hip.lib()
    d_xyz, d_f = torch.from_numpy(xyz).to(DEV), torch.from_numpy(faces).to(DEV)
    out = torch.empty(33 * 33, dtype=torch.int32, device=DEV)
    need = lib.sg_render_ws_bytes(V, 200, 1, 33, 33)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rows = np.ascontiguousarray(cam[None])

    def call(xyz_p=d_xyz.data_ptr(), stride=3, faces_p=d_f.data_ptr(), F=200, point=3, B=1, cams=rows, near=0.05, W=33, H=33, prim=out.data_ptr(),
             ws_bytes=need):
        return lib.sg_render(xyz_p, stride, V, faces_p, F, point, B, cams.ctypes.data, 1, near, W, H, prim, None, None, None, ws.data_ptr(), ws_bytes, None)

    assert call() == hip.SG_OK
    nan_cam, zero_fx = rows.copy(), rows.copy()
    nan_cam[0, 5], zero_fx[0, 12] = np.nan, 0.0
    for kw, word in ((dict(xyz_p=None), "null"), (dict(prim=None), "null"), (dict(stride=2), "rows of 2 floats"), (dict(faces_p=None), "splats NULL with F == 0"),
                     (dict(F=0), "splats NULL with F == 0"), (dict(faces_p=None, F=0, point=4), "point_size 4"), (dict(faces_p=None, F=0, point=17), "point_size 17"),
                     (dict(near=0.0), "near"), (dict(near=float("nan")), "near"), (dict(near=float("inf")), "near"), (dict(cams=nan_cam), "not finite"),
                     (dict(cams=zero_fx), "fx = 0"), (dict(ws_bytes=need - 1), "workspace too small")):
        assert call(**kw) == hip.SG_EINVAL, kw
        msg = lib.sg_last_error().decode()
        assert msg.startswith("sg_render:") and word in msg, (kw, msg)
    for kw in (dict(W=4097), dict(H=4097), dict(B=65), dict(F=(1 << 26) + 1)):
        assert call(**kw) == hip.SG_EUNSUP, kw
        assert lib.sg_last_error().decode().startswith("sg_render:")
    assert lib.sg_render_ws_bytes(V, 200, 64, 2048, 1024) == 0 and lib.sg_render_ws_bytes(V, 200, 1, 4096, 4096) > 0       # B*H*W <= 2^26
    assert lib.sg_render_ws_bytes(0, 0, 1, 8, 8) == 0 and lib.sg_render_ws_bytes(V, 0, 1, 8, 8) > 0
    h = (C.c_int64 * 6)()
    assert lib.sg_render_stats(h, 5) == hip.SG_EINVAL and lib.sg_last_error().decode().startswith("sg_render_stats:")
    assert lib.sg_render_set_tuning(33) == hip.SG_EINVAL and lib.sg_last_error().decode().startswith("sg_render_set_tuning:")
    bg = np.zeros(3, np.uint8)
    assert lib.sg_render_colour(out.data_ptr(), 4, None, None, V, bg.ctypes.data, out.data_ptr(), None) == hip.SG_EINVAL
    assert lib.sg_last_error().decode().startswith("sg_render_colour:")


def test_the_threshold_changes_the_count_of_large_primitives_only(soup):
    from seggroup_amd import hip
    from seggroup_amd import render as M
    xyz, faces, known = soup
    cam, ortho, want = known["perspective"]
    lib = hip.lib()
    try:
        for small in (1, 16, 32):
            hip.check(lib.sg_render_set_tuning(small))
            got = M.render(xyz, faces, cam, SIZE, ortho, R.SOUP_NEAR, device=DEV)
            stats = M.last_stats()
            _same(got, want, small)
            assert {k: v for k, v in stats.items() if k != "large"} == {k: v for k, v in want.stats.items() if k != "large"}
            assert (stats["large"] > want.stats["large"]) == (small < R.SMALL) and (stats["large"] < want.stats["large"]) == (small > R.SMALL)
    finally:
        hip.check(lib.sg_render_set_tuning(0))
    _check(xyz, faces, cam, SIZE, ortho, want=want, what="the build's threshold again")


def test_colours_are_the_palette_of_visualize():
    import torch
    from seggroup_amd import render as M
    from seggroup_amd import visualize
    rng = np.random.RandomState(3)
    V = 500
    vert = rng.randint(-1, V, (2, 9, 13)).astype(np.int32)
    vert[0, 0, :3] = [-1, 0, V - 1]
    palette = np.asarray(visualize.colors, np.uint8)
    labels = {"instance": rng.randint(-1, 30, V), "semantic": rng.randint(0, 41, V), "segment": rng.randint(0, 5000, V)}
    sem = rng.randint(0, 5, V).astype(np.int32)
    for kind, lab in labels.items():
        for second in (None, sem) if kind == "instance" else (None,):
            for bg in ((255, 255, 255), (1, 2, 3)):
                cidx = visualize.colour_vector(lab.astype(np.int32), kind, second=second, device=DEV).cpu().numpy()
                want = np.where((vert >= 0)[..., None], palette[cidx][np.maximum(vert, 0)], np.asarray(bg, np.uint8))
                got = M.colour(vert, labels=lab.astype(np.int32), label_type=kind, second=second, background=bg, device=DEV)
                assert got.dtype == np.uint8 and got.shape == (2, 9, 13, 3) and np.array_equal(got, want), (kind, bg)
    rgb = rng.randint(0, 256, (V, 3)).astype(np.uint8)
    got = M.colour(vert, rgb=rgb, background=(9, 8, 7), device=DEV, stream=torch.cuda.Stream(device=DEV))
    assert np.array_equal(got, np.where((vert >= 0)[..., None], rgb[np.maximum(vert, 0)], np.asarray((9, 8, 7), np.uint8)))
    assert M.colour(vert[:0], rgb=rgb, device=DEV).shape == (0, 9, 13, 3)
    for kw, word in ((dict(), "exactly one"), (dict(labels=sem, rgb=rgb), "exactly one"), (dict(labels=sem, label_type="colour"), "label_type"),
                     (dict(rgb=rgb.astype(np.int32)), "uint8"), (dict(rgb=rgb, background=(0, 0, 256)), "background")):
        with pytest.raises(ValueError, match=word):
            M.colour(vert, device=DEV, **kw)


@pytest.fixture(scope="module")
def sheet():
    from seggroup_amd import render as M
    xyz, faces, hidden = R.folded_sheet()
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    size = (320, 240)
    top = M.top_view(lo, hi, size)
    orbit = M.orbit_views(lo, hi, size, 4, -50.0)
    return (xyz, faces, hidden, size, top, orbit, R.render(xyz, faces, top.row(), size, True, 0.05, buckets=True),
            R.render(xyz, faces, np.stack([c.row() for c in orbit]), size, False, 0.05, buckets=True))


def test_a_folded_sheet_of_20000_vertices_from_above_and_from_below(sheet):
    xyz, faces, hidden, size, top, orbit, want_top, want_orbit = sheet
    assert xyz.shape[0] == 20000 and hidden.sum() > 2000
    above, s = _check(xyz, faces, top, size, ortho=True, near=0.05, want=want_top, what="top")
    assert s["kept"] == faces.shape[0] and s["covered"] > 0.95 * 288 * 144      # the 4 x 2 sheet at 72 pixels a unit
    below, _ = _check(xyz, faces, orbit, size, near=0.05, want=want_orbit, what="orbit from below")
    assert (above.hits[hidden] == 0).all()                                       # the folded part lies under the sheet: no pixel of the top view sees it
    assert (below.hits[hidden] > 0).all()                                        # from below the folded part is the nearest surface: every vertex of it is seen


# ---- the command ------------------------------------------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    from seggroup_amd.prepare import write_ply
    rng = np.random.RandomState(8)
    scans_dir, lab_dir = tmp_path / "scans", tmp_path / "labels"
    lab_dir.mkdir()
    mesh_xyz, mesh_faces, _ = R.folded_sheet(40, 30, 2)
    cloud = np.stack([rng.uniform(0, 3, 5000), rng.uniform(0, 2, 5000), rng.uniform(0, 1, 5000)], 1).astype(np.float32)
    out = {}
    for name, xyz, faces in (("scene0000_00", mesh_xyz, mesh_faces), ("scene0001_00", cloud, np.zeros((0, 3), np.int32))):
        (scans_dir / name).mkdir(parents=True)
        rgb = rng.randint(0, 256, (xyz.shape[0], 3)).astype(np.uint8)
        write_ply(str(scans_dir / name / (name + "_vh_clean_2.ply")), xyz, rgb, faces)
        labels = (np.floor(xyz[:, 0] * 2.0) + 1).astype(np.int32)
        labels[::17] = -1
        np.save(str(lab_dir / (name + ".ins.npy")), labels)
        out[name] = (xyz, faces, rgb, labels)
    return str(scans_dir), str(lab_dir), out


def test_the_command_on_a_mesh_and_a_faceless_scan(tmp_path, capsys):
    from seggroup_amd import render as M
    scans_dir, lab_dir, scenes = _tree(tmp_path)
    out = str(tmp_path / "out")
    args = ["--scans", scans_dir, "--out", out, "--labels-from", lab_dir, "--suffix", ".ins.npy", "--label-type", "instance", "--views", "orbit:2",
            "--size", "96", "64", "--sheet", "2", "--npz", "--depth", "--workers", "2", "--device", DEV]
    assert M.main(args) == 0
    assert "2 written, 0 skipped" in capsys.readouterr().out
    report = json.load(open(os.path.join(out, "render_report.json")))
    assert report["skipped"] == [] and report["parameters"]["view_names"] == ["orbit0", "orbit1"] and sorted(report["scenes"]) == sorted(scenes)
    for name, (xyz, faces, _, labels) in scenes.items():
        entry = report["scenes"][name]
        with np.load(os.path.join(out, name + ".render.npz")) as z:
            got = {k: z[k] for k in z.files}
        assert sorted(got) == ["cameras", "depth", "hits", "label.labels", "prim", "vert"]
        assert got["cameras"].shape == (2, 16) and got["prim"].shape == (2, 64, 96)
        splats = faces.shape[0] == 0
        want = R.render(xyz, None if splats else faces, got["cameras"], (96, 64), False, 0.05, 3, buckets=True)
        _same(M.Render(got["prim"], got["depth"], got["vert"], got["hits"]), want, name)
        assert {k: entry[k] for k in R.STAT_NAMES} == want.stats and entry["splats"] == splats and entry["vertices"] == xyz.shape[0]
        assert entry["vertices_seen"] == int((want.hits > 0).sum()) > 0 and entry["faces"] == faces.shape[0]
        assert np.array_equal(got["label.labels"], np.where(want.vert >= 0, labels[np.maximum(want.vert, 0)], -1))
        coloured = M.colour(want.vert, labels=labels, label_type="instance", device=DEV)
        tiles = []
        for b, view in enumerate(("orbit0", "orbit1")):
            assert entry["views"][view] == dict(covered=int((want.prim[b] >= 0).sum()), vertices_seen=int(np.unique(want.vert[b][want.vert[b] >= 0]).shape[0]))
            assert entry["views"][view]["covered"] > 200
            png = R.read_png(os.path.join(out, "%s.%s.labels.png" % (name, view)))
            assert np.array_equal(png, coloured[b])
            assert (png[want.vert[b] < 0] == 255).all() and len(np.unique(png.reshape(-1, 3), axis=0)) > 3
            assert np.array_equal(R.read_png(os.path.join(out, "%s.%s.depth.png" % (name, view))), M.depth_mm(want.depth[b]))
            tiles.append(png)
        assert np.array_equal(R.read_png(os.path.join(out, name + ".sheet.png")), np.concatenate(tiles, 1))
    assert M.main(args) == 0                                                      # every first image is there: nothing is drawn again
    assert "0 written, 2 skipped" in capsys.readouterr().out
    rgb_out = str(tmp_path / "rgb")
    assert M.main(["--scans", scans_dir, "--out", rgb_out, "--rgb", "--pointcloud", "--point-size", "5", "--size", "80", "60", "--npz", "--device", DEV]) == 0
    rep = json.load(open(os.path.join(rgb_out, "render_report.json")))
    for name, (xyz, faces, rgb, _) in scenes.items():
        assert rep["scenes"][name]["splats"] and rep["scenes"][name]["faces"] == 0 and list(rep["scenes"][name]["views"]) == ["top"]
        with np.load(os.path.join(rgb_out, name + ".render.npz")) as z:
            cams, vert = z["cameras"], z["vert"]
        want = R.render(xyz, None, cams, (80, 60), True, 0.05, 5)                 # the top view is orthographic
        assert np.array_equal(vert, want.vert) and rep["scenes"][name]["covered"] == want.stats["covered"] > 1000
        png = R.read_png(os.path.join(rgb_out, name + ".top.rgb.png"))
        assert np.array_equal(png, np.where((vert[0] >= 0)[..., None], rgb[np.maximum(vert[0], 0)], np.uint8(255)))
