"""Scans and their labels as images on the GPU: what a label vector looks like from a camera, and which vertex every pixel
sees.  `visualize` colours a copy of the scan's PLY, which a headless machine cannot look at; this writes PNGs.

    img = render(xyz, faces, cameras=top_view(lo, hi, size), size=size, ortho=True)   -- sg_render: Render(prim, depth, vert [B,H,W], hits [V])
    rgb = colour(img.vert, labels=ins, label_type="instance")                          -- sg_render_colour: uint8 [B,H,W,3], visualize's palette
    write_png(path, rgb[0]); write_png(path, depth_mm(img.depth[0]))

THE RULE (include/seggroup_hip.h; tests/render_ref.py restates it): a z-buffer over fixed-point screen coordinates (1/256 pixel), int64 edge
functions, a pixel centre on an edge is inside, nothing is clipped or blended -- a primitive with a vertex behind `near` or beyond the
guard band of 16384 pixels is dropped whole --, and a pixel keeps the least (float depth, primitive index).  `vert` is the winning face's
corner with the largest edge function, `hits[v]` the pixels of all views whose `vert` is v.  Exact and order-free: equality with the
restatement is the gate, and the same bytes come back on every run.  A scan without faces (faces=None) is drawn as square splats of side
`point_size`.  The camera looks along +z with x to the right and y DOWN; the centre of pixel (px, py) is (px + 0.5, py + 0.5).

Views are host NumPy (the kernel sees 16 doubles a view): Camera(T, fx, fy, cx, cy), look_at, top_view (orthographic: pass ortho=True),
orbit_views, from_pose (ScanNet's camera-to-world pose and intrinsics).

    python -m seggroup_amd.render --scans DIR --out DIR
        ( -n EXP --stage S [--layer final.ins ...] [--root .] | --labels-from DIR --suffix SFX [--key NAME] --label-type T | --rgb )
        [--views top | orbit:N | poses:FILE.npz] [--size W H] [--ortho] [--elevation DEG] [--near D] [--point-size P] [--pointcloud]
        [--depth] [--npz] [--sheet COLS] [--shuffle] [--scenes FILE --workers W --device D --force]
    Per scene ONE sg_render call draws all views; a scan with faces is a mesh, a face-less one (or any with --pointcloud) splats.  Written:
    OUT/<scene>.<view>.<vector>.png (views `top`, `orbit0`.., `pose0`..; vectors the --layer names, the --key (or `labels`), or `rgb`), with
    --depth OUT/<scene>.<view>.depth.png (16-bit grey, millimetres, 0 where empty), with --npz OUT/<scene>.render.npz (prim, vert, depth,
    hits, cameras and `label.<vector>` int32 images, -1 where empty), with --sheet OUT/<scene>.sheet.png (all views x vectors, COLS a row),
    and OUT/render_report.json: per scene the five counts of sg_render_stats and the covered pixels, SUMMED over the views (the one call
    a scene counts them so), and per view the covered pixels and the vertices seen.  `top` is orthographic; --ortho makes orbit and pose
    views orthographic too.  poses:FILE.npz holds `T` [B,3,4] or [B,4,4] world->camera and `K` [B,4] = fx fy cx cy, taken AS GIVEN in this
    module's convention (the centre of pixel (px, py) is (px + 0.5, py + 0.5)): intrinsics that put pixel centres on whole numbers
    (ScanNet's, OpenCV's) need 0.5 added to cx and cy first, which `from_pose` does -- save its Camera's T and fx fy cx cy.  A scene whose
    first image OUT holds already is skipped without --force.

Not here: clipping against the near plane, shading, lighting, anti-aliasing, textures, a top-left fill rule, lifting 2D labels back onto
vertices (that is seggroup_amd/lift.py), reading .sens files.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import random
import struct
import sys
import zlib
from typing import NamedTuple

import numpy as np

from . import hip, scans
from .device import cloud_box, device_cloud, device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_FACES = 1 << 26
MAX_VIEWS = 64
MAX_SIDE = 4096
MAX_PIXELS = 1 << 26
MAX_POINT_SIZE = 15
STAT_NAMES = ("kept", "behind", "far", "degenerate", "large", "covered")
REPORT_NAME = "render_report.json"
NPZ_SUFFIX = ".render.npz"
LABEL_TYPES = ("instance", "semantic", "segment")


class Camera(NamedTuple):
    """one view: T float64 [3,4] world->camera (the camera looks along +z, x right, y down), then the intrinsics in pixels"""
    T: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float

    def row(self) -> np.ndarray:
        return np.concatenate([np.asarray(self.T, np.float64)[:3, :4].reshape(12), [self.fx, self.fy, self.cx, self.cy]])


class Render(NamedTuple):
    """render's result: prim int32, depth float32, vert int32 [B,H,W] (-1 / +inf / -1 where empty), hits int32 [V]"""
    prim: np.ndarray
    depth: np.ndarray
    vert: np.ndarray
    hits: np.ndarray


# ---- views (host) -------------------------------------------------------------------------------------------------------------------------------
def _vec3(v, what: str) -> np.ndarray:
    v = np.asarray(v, np.float64)
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError("%s is 3 finite numbers, not %r" % (what, v.tolist() if v.ndim else v))
    return v


def look_at(eye, target, up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """-> T float64 [3,4] world->camera of a camera at `eye` that looks at `target`: rows right, down, forward"""
    eye, target, up = _vec3(eye, "eye"), _vec3(target, "target"), _vec3(up, "up")
    f = target - eye
    r = np.cross(f, up)
    if not np.linalg.norm(f) > 0.0 or not np.linalg.norm(r) > 1e-12 * np.linalg.norm(f) * np.linalg.norm(up):
        raise ValueError("look_at: eye and target coincide, or the view direction is along `up`")
    f, r = f / np.linalg.norm(f), r / np.linalg.norm(r)
    R = np.stack([r, np.cross(f, r), f])
    return np.concatenate([R, (-R @ eye)[:, None]], 1)


def _size(size):
    try:
        W, H = (int(s) for s in size)
        whole = all(float(s) == int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError("size (size=, --size) is W H, two whole numbers, not %r" % (size,)) from None
    if not whole or not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError("size (size=, --size) is W H with 1 <= W, H <= %d, not %r" % (MAX_SIDE, tuple(size)))
    return W, H


def _box(lo, hi):
    lo, hi = _vec3(lo, "lo"), _vec3(hi, "hi")
    if (hi < lo).any():
        raise ValueError("the box has hi below lo")
    return lo, hi, 0.5 * (lo + hi), max(float(np.linalg.norm(hi - lo)), 1e-6)


def _corners(lo, hi) -> np.ndarray:
    return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])


def _fit(T, corners, W, H, margin, ortho) -> Camera:
    """the largest fx = fy with the corners inside the image's inner (1 - 2 margin) part, the principal point at the image's centre"""
    c = corners @ T[:, :3].T + T[:, 3]
    a = c[:, :2] if ortho else c[:, :2] / c[:, 2:3]
    half = (0.5 - margin) * np.array([W, H], np.float64)
    reach = np.abs(a).max(0)
    f = float(min(half[k] / reach[k] for k in (0, 1) if reach[k] > 0.0) if (reach > 0.0).any() else min(W, H))
    return Camera(T, f, f, 0.5 * W, 0.5 * H)


def _margin(margin) -> float:
    if not 0.0 <= float(margin) < 0.5:
        raise ValueError("margin is a share of the image in [0, 0.5), not %r" % (margin,))
    return float(margin)


def top_view(lo, hi, size, margin=0.05) -> Camera:
    """ORTHOGRAPHIC (render(..., ortho=True)): looks down world z from above the box, x to the right and y up the image, fitted to the box"""
    W, H = _size(size)
    lo, hi, mid, diag = _box(lo, hi)
    eye = np.array([mid[0], mid[1], hi[2] + 1.0 + diag])
    return _fit(look_at(eye, [mid[0], mid[1], hi[2]], up=(0.0, 1.0, 0.0)), _corners(lo, hi), W, H, _margin(margin), True)


def orbit_views(lo, hi, size, n=4, elevation_deg=30.0, margin=0.05, ortho=False):
    """`n` views around the box's centre at 1.5 diagonals, `elevation_deg` above the horizon (negative: from below), each fitted so that the
    box's eight corners fall inside the image -> [Camera]"""
    W, H = _size(size)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_VIEWS:
        raise ValueError("orbit views (n=, --views orbit:N) are 1..%d, not %r" % (MAX_VIEWS, n))
    if not -89.0 <= float(elevation_deg) <= 89.0:
        raise ValueError("elevation (elevation_deg=, --elevation) is -89..89 degrees, not %r" % (elevation_deg,))
    lo, hi, mid, diag = _box(lo, hi)
    el = math.radians(float(elevation_deg))
    out = []
    for k in range(int(n)):
        az = 2.0 * math.pi * k / int(n)
        eye = mid + 1.5 * diag * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        out.append(_fit(look_at(eye, mid), _corners(lo, hi), W, H, _margin(margin), ortho))
    return out


def from_pose(pose_cam_to_world, K) -> Camera:
    """ScanNet's convention: a 4 x 4 camera-to-world pose (x right, y down, z forward) and the intrinsics K (3 x 3, 4 x 4, or fx fy cx cy).
    The rigid inverse is taken in double.  K's pixel centres sit on whole numbers, this module's on halves: cx and cy move by 0.5."""
    P = np.asarray(pose_cam_to_world, np.float64)
    if P.shape != (4, 4) or not np.isfinite(P).all():
        raise ValueError("from_pose: a pose is a finite 4 x 4 camera-to-world matrix, not %r" % (P.shape,))
    K = np.asarray(K, np.float64)
    if K.shape in ((3, 3), (4, 4)):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if K.shape != (4,) or not np.isfinite(K).all():
        raise ValueError("from_pose: K is 3 x 3, 4 x 4 or fx fy cx cy")
    R = P[:3, :3].T
    return Camera(np.concatenate([R, (-R @ P[:3, 3])[:, None]], 1), float(K[0]), float(K[1]), float(K[2]) + 0.5, float(K[3]) + 0.5)


def camera_rows(cameras) -> np.ndarray:
    """a Camera, a sequence of them, or [B,16] numbers -> float64 [B,16]; the library's refusals about cameras, made on the host"""
    if isinstance(cameras, Camera):
        cameras = [cameras]
    if cameras is None or len(cameras) == 0:
        raise ValueError("render: cameras= is a Camera, a list of them or [B,16] numbers")
    rows = np.stack([c.row() for c in cameras]) if all(isinstance(c, Camera) for c in cameras) else np.asarray(cameras, np.float64)
    if rows.shape == (16,):
        rows = rows[None]
    if rows.ndim != 2 or rows.shape[1] != 16:
        raise ValueError("render: cameras are [B,16] numbers (T row-major 3 x 4, fx fy cx cy), not %r" % (rows.shape,))
    if not 1 <= rows.shape[0] <= MAX_VIEWS:
        raise ValueError("render: %d views; a call takes 1..%d" % (rows.shape[0], MAX_VIEWS))
    if not np.isfinite(rows).all():
        raise ValueError("render: a camera number that is not finite")
    if (rows[:, 12:14] == 0.0).any():
        raise ValueError("render: a camera with fx or fy equal to 0")
    return np.ascontiguousarray(rows, np.float64)


# ---- the call -----------------------------------------------------------------------------------------------------------------------------------
def check_point_size(point_size) -> int:
    if isinstance(point_size, bool) or not isinstance(point_size, (int, np.integer)) or not 1 <= point_size <= MAX_POINT_SIZE or point_size % 2 == 0:
        raise ValueError("point size (point_size=, --point-size) is the side of a splat in pixels, odd and 1..%d, not %r" % (MAX_POINT_SIZE, point_size))
    return int(point_size)


def check_near(near) -> float:
    if isinstance(near, (bool, str)) or not isinstance(near, (int, float, np.integer, np.floating)) or not (math.isfinite(near) and near > 0.0):
        raise ValueError("near (near=, --near) is a finite distance > 0, not %r" % (near,))
    return float(near)


def check_image(size, views: int):
    W, H = _size(size)
    if views * W * H > MAX_PIXELS:
        raise ValueError("size (size=, --size): %d views of %d x %d pixels; a call takes at most 2^26 pixels in all" % (views, W, H))
    return W, H


def last_stats() -> dict:
    """sg_render_stats: the calling thread's last call, over all its views -> {kept, behind, far, degenerate, large, covered}"""
    h = (C.c_int64 * len(STAT_NAMES))()
    hip.check(hip.lib().sg_render_stats(h, len(STAT_NAMES)))
    return dict(zip(STAT_NAMES, (int(v) for v in h)))


def render(xyz, faces=None, cameras=None, size=(640, 480), ortho=False, near=0.05, point_size=3, device=None, stream=None) -> Render:
    """sg_render.  `xyz` [V, >= 3] (array or tensor; float32); `faces` [F,3] whole numbers, or None / no rows for splats of side `point_size`;
    `cameras` a Camera, a list of them or [B,16]; `size` (W, H).  -> Render of NumPy arrays.  A face index outside 0..V-1 is the library's
    ValueError."""
    rows = camera_rows(cameras)
    B = int(rows.shape[0])
    W, H = check_image(size, B)
    near, point_size = check_near(near), check_point_size(point_size)
    if faces is not None:
        shape = tuple(faces.shape) if hasattr(faces, "shape") else np.shape(faces)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("render: faces are [F,3] vertex indices, not %r" % (shape,))
        if shape[0] > MAX_FACES:
            raise hip.SgError(hip.SG_EUNSUP, "render: %d faces; a call takes at most 2^26" % shape[0])
        if shape[0] == 0:
            faces = None
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, V = device_cloud(xyz, dev, "render")
        d_faces = None if faces is None else device_tensor(faces, torch.int32, dev)
        F = 0 if d_faces is None else int(d_faces.shape[0])
        d_prim = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        d_depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        d_vert = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        d_hits = torch.empty(V, dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_render_ws_bytes(V, F, B, W, H), dev)
        hip.check_arg(lib.sg_render(d_xyz.data_ptr(), int(d_xyz.shape[1]), V, hip.ptr(d_faces), F, point_size, B, rows.ctypes.data, int(bool(ortho)),
                                    near, W, H, d_prim.data_ptr(), d_depth.data_ptr(), d_vert.data_ptr(), d_hits.data_ptr(), ws.data_ptr(),
                                    ws.numel(), stream_ptr(stream)))
        sync(stream)
        return Render(d_prim.cpu().numpy(), d_depth.cpu().numpy(), d_vert.cpu().numpy(), d_hits.cpu().numpy())


def _rgb3(c, what: str) -> np.ndarray:
    a = np.asarray(c)
    if a.shape != (3,) or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
        raise ValueError("%s is three whole numbers 0..255, not %r" % (what, c))
    return np.ascontiguousarray(a, np.uint8)


def colour(vert, labels=None, label_type="instance", second=None, rgb=None, background=(255, 255, 255), shuffle=False, rng=random, device=None,
           stream=None) -> np.ndarray:
    """sg_render_colour: `vert` int32 [...] (a Render's) -> uint8 [..., 3].  Exactly one of `labels` [V] -- coloured as `visualize` colours a
    PLY: colour_vector(labels, label_type, shuffle, second), so a rendered colour is the PLY's colour of the same label -- and `rgb` uint8
    [V,3], the scan's own colours.  An empty pixel takes `background`."""
    if (labels is None) == (rgb is None):
        raise ValueError("colour: exactly one of labels= (with label_type=) and rgb= is needed")
    if labels is not None and label_type not in LABEL_TYPES:
        raise ValueError("colour: label_type (label_type=, --label-type) is %s, not %r" % (", ".join(LABEL_TYPES), label_type))
    bg = _rgb3(background, "background")
    vert = np.asarray(vert)
    if vert.dtype != np.int32:
        raise ValueError("colour: vert is a Render's int32 image, not %s" % vert.dtype)
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.ndim != 2 or rgb.shape[1] != 3 or rgb.dtype != np.uint8 or rgb.shape[0] < 1:
            raise ValueError("colour: rgb is uint8 [V,3], not %s %r" % (rgb.dtype, rgb.shape))
    import torch
    from . import visualize
    dev = torch_device(device)
    lib = hip.lib()
    n = int(vert.size)
    with torch.cuda.device(dev), on_stream(stream):
        d_vert = device_tensor(vert.reshape(-1), torch.int32, dev)
        d_img = torch.empty((max(n, 1), 3), dtype=torch.uint8, device=dev)
        if rgb is None:
            d_cidx = visualize.colour_vector(labels, label_type, shuffle=bool(shuffle), second=second, rng=rng, device=dev)
            d_rgb, V = None, int(d_cidx.shape[0])
        else:
            d_cidx, d_rgb, V = None, device_tensor(rgb, torch.uint8, dev), int(rgb.shape[0])
        if V < 1:
            raise ValueError("colour: no vertex has a colour")
        hip.check_arg(lib.sg_render_colour(d_vert.data_ptr(), n, hip.ptr(d_cidx), hip.ptr(d_rgb), V, bg.ctypes.data, d_img.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
        sync(stream)
        return d_img[:n].cpu().numpy().reshape(vert.shape + (3,))


# ---- images (host) ----------------------------------------------------------------------------------------------------------------------------
def depth_mm(depth) -> np.ndarray:
    """float depth -> uint16 millimetres (rounded, at most 65535), 0 where empty (+inf)"""
    d = np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(d), np.minimum(np.rint(d * 1000.0), 65535.0), 0.0).astype(np.uint16)


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def write_png(path: str, img) -> None:
    """uint8 [H,W,3] -> 8-bit RGB; uint16 [H,W] -> 16-bit grey.  zlib of the standard library, filter 0 on every row."""
    a = np.asarray(img)
    if a.ndim < 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: an image has at least one pixel, not %r" % (a.shape,))
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        bits, colour_type, body = 8, 2, np.ascontiguousarray(a).reshape(a.shape[0], -1)
    elif a.dtype == np.uint16 and a.ndim == 2:
        bits, colour_type, body = 16, 0, np.ascontiguousarray(a.astype(">u2")).view(np.uint8).reshape(a.shape[0], -1)
    else:
        raise ValueError("write_png: an image is uint8 [H,W,3] or uint16 [H,W], not %s %r" % (a.dtype, a.shape))
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), body], 1)             # filter 0 in front of every row
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bits, colour_type, 0, 0, 0)) + \
        _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b"")
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


def contact_sheet(images, cols: int, background=(255, 255, 255)) -> np.ndarray:
    """equal uint8 [H,W,3] images, `cols` a row, row by row -> uint8 [rows * H, cols * W, 3]; what the last row lacks is background"""
    if isinstance(cols, bool) or not isinstance(cols, (int, np.integer)) or cols < 1:
        raise ValueError("sheet columns (cols=, --sheet) are a whole number >= 1, not %r" % (cols,))
    images = [np.asarray(i) for i in images]
    if not images or any(i.dtype != np.uint8 or i.ndim != 3 or i.shape != images[0].shape or i.shape[2] != 3 for i in images):
        raise ValueError("contact_sheet: at least one image, all uint8 [H,W,3] of one size")
    H, W = images[0].shape[:2]
    rows = (len(images) + cols - 1) // cols
    sheet = np.empty((rows * H, cols * W, 3), np.uint8)
    sheet[:] = _rgb3(background, "background")
    for k, im in enumerate(images):
        r, c = divmod(k, cols)
        sheet[r * H:(r + 1) * H, c * W:(c + 1) * W] = im
    return sheet


# ---- scans --------------------------------------------------------------------------------------------------------------------------------------
def parse_views(views: str):
    """'top' | 'orbit:N' | 'poses:FILE.npz' -> ('top', None) | ('orbit', N) | ('poses', path); anything else is a ValueError naming --views"""
    if views == "top":
        return "top", None
    kind, _, arg = views.partition(":")
    if kind == "orbit":
        try:
            n = int(arg)
        except ValueError:
            n = 0
        if not 1 <= n <= MAX_VIEWS:
            raise ValueError("--views orbit:N takes N in 1..%d, not %r" % (MAX_VIEWS, arg))
        return "orbit", n
    if kind == "poses" and arg:
        return "poses", arg
    raise ValueError("--views is top, orbit:N or poses:FILE.npz, not %r" % (views,))


def load_poses(path: str):
    """poses:FILE.npz -> [Camera]: `T` [B,3,4] or [B,4,4] world->camera, `K` [B,4] = fx fy cx cy as given, pixel centres on halves
    (no shift by 0.5 as in from_pose, whose input is ScanNet's)"""
    with np.load(path) as z:
        if "T" not in z.files or "K" not in z.files:
            raise ValueError("--views poses:%s needs the arrays T and K (it has %s)" % (path, ", ".join(z.files)))
        T, K = np.asarray(z["T"], np.float64), np.asarray(z["K"], np.float64)
    if T.ndim != 3 or T.shape[1:] not in ((3, 4), (4, 4)) or K.shape != (T.shape[0], 4) or not 1 <= T.shape[0] <= MAX_VIEWS:
        raise ValueError("--views poses:%s: T is [B,3,4] or [B,4,4] and K [B,4] with B in 1..%d, not %r and %r" % (path, MAX_VIEWS, T.shape, K.shape))
    return [Camera(t[:3], *(float(k) for k in row)) for t, row in zip(T, K)]


def check_command(exp=None, stage=None, layers=None, root=None, labels_from=None, suffix=None, key=None, label_type=None, rgb=False, views="top",
                  size=(640, 480), ortho=False, elevation=30.0, near=0.05, point_size=3, sheet=None, **_) -> dict:
    """every refusal of the command that needs no scan (ValueError naming the flag), before any device work -> the parameters in force"""
    if (exp is not None) + (labels_from is not None) + bool(rgb) != 1:
        raise ValueError("exactly one source of colours is needed: -n EXP (with --stage), --labels-from DIR (with --suffix and --label-type) or --rgb")
    if exp is None and (stage is not None or layers or root is not None):
        raise ValueError("--stage, --layer and --root belong to the experiment route (-n EXP)")
    if labels_from is None and (suffix is not None or key is not None or label_type is not None):
        raise ValueError("--suffix, --key and --label-type belong to --labels-from")
    vectors = ["rgb"]
    if exp is not None:
        vectors = list(layers) if layers else ["final.ins"]
        for v in vectors:
            if v not in hip.LABEL_NAMES:
                raise ValueError("--layer names an exported vector (%s), not %r" % (", ".join(hip.LABEL_NAMES), v))
    if labels_from is not None:
        if suffix is None or not suffix.endswith((".npy", ".npz")):
            raise ValueError("--labels-from needs --suffix, ending in .npy or .npz (the file is DIR/<scene><suffix>)")
        if suffix.endswith(".npz") != (key is not None):
            raise ValueError("--key names the array of an .npz --suffix; a .npy holds one vector")
        if label_type not in LABEL_TYPES:
            raise ValueError("--label-type is needed with --labels-from: %s, not %r" % (", ".join(LABEL_TYPES), label_type))
        vectors = [key or "labels"]
    kind, arg = parse_views(views)
    cams = load_poses(arg) if kind == "poses" else None
    B = 1 if kind == "top" else arg if kind == "orbit" else len(cams)
    W, H = check_image(size, B)
    if kind == "orbit":
        orbit_views(np.zeros(3), np.ones(3), (W, H), arg, elevation)              # --elevation's refusal
    if sheet is not None:
        contact_sheet([np.zeros((1, 1, 3), np.uint8)], sheet)                     # --sheet's refusal
    names = ["top"] if kind == "top" else ["%s%d" % ("orbit" if kind == "orbit" else "pose", k) for k in range(B)]
    return dict(exp=exp, stage=stage or "epoch_last", root=root or ".", labels_from=labels_from, suffix=suffix, key=key, label_type=label_type,
                rgb=bool(rgb), vectors=vectors, kind=kind, views=B, view_names=names, cameras=cams, size=(W, H), ortho=bool(ortho) or kind == "top",
                elevation=float(elevation), near=check_near(near), point_size=check_point_size(point_size), sheet=sheet)


def _vector_type(name: str) -> str:
    return {"seg": "segment", "ins": "instance", "sem": "semantic"}[name.rsplit(".", 1)[1]]


def scene_vectors(scene: str, n: int, rgb, p: dict):
    """-> [(vector name, labels int32 [V] or None, label type or None)]: what the scene's images are coloured by"""
    if p["rgb"]:
        return [("rgb", None, None)]
    if p["exp"] is not None:
        from . import pseudo_labels
        lab = pseudo_labels.load(os.path.join(p["root"], "results", p["exp"], scene, p["stage"]))
        out = [(v, np.ascontiguousarray(lab.vector(v), np.int32), _vector_type(v)) for v in p["vectors"]]
    else:
        from .boxes import scene_labels
        out = [(p["vectors"][0], scene_labels(scene, n, labels_from=p["labels_from"], suffix=p["suffix"], key=p["key"])[0], p["label_type"])]
    for name, vec, _ in out:
        if vec.shape[0] != n:
            raise ValueError("%s: %s holds %d labels for %d vertices" % (scene, name, vec.shape[0], n))
    return out


def first_image(out_dir: str, scene: str, p: dict) -> str:
    return os.path.join(out_dir, "%s.%s.%s.png" % (scene, p["view_names"][0], p["vectors"][0]))


def render_scan(scene_path: str, out_dir: str, p: dict, pointcloud=False, depth=False, npz=False, shuffle=False, force=False, device=None, stream=None):
    """One scan directory -> its images under `out_dir` -> its entry of render_report.json, or None when its first image was there already
    (never overwritten without `force`).  `p` is check_command's."""
    from .prepare import mesh_arrays, read_ply
    scene = scans.scene_name(scene_path)
    if os.path.exists(first_image(out_dir, scene, p)) and not force:
        return None
    xyz, rgb, faces = mesh_arrays(read_ply(os.path.join(scene_path, scene + scans.PLY_SUFFIX)))
    V = int(xyz.shape[0])
    vectors = scene_vectors(scene, V, rgb, p)
    splats = bool(pointcloud) or faces.shape[0] == 0
    import torch
    dev = torch_device(device)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, _ = device_cloud(xyz, dev, "render")
        lo, hi = cloud_box(d_xyz, "render: " + scene)
    W, H = p["size"]
    cams = p["cameras"] if p["kind"] == "poses" else [top_view(lo, hi, (W, H))] if p["kind"] == "top" else \
        orbit_views(lo, hi, (W, H), p["views"], p["elevation"], ortho=p["ortho"])
    img = render(d_xyz, None if splats else faces, cams, (W, H), p["ortho"], p["near"], p["point_size"], device=dev, stream=stream)
    stats = last_stats()
    os.makedirs(out_dir, exist_ok=True)
    arrays = dict(prim=img.prim, vert=img.vert, depth=img.depth, hits=img.hits, cameras=camera_rows(cams))
    tiles = []
    coloured = {}
    for name, vec, kind in vectors:
        if vec is None:
            coloured[name] = colour(img.vert, rgb=rgb, device=dev, stream=stream)
        else:
            coloured[name] = colour(img.vert, labels=vec, label_type=kind, shuffle=shuffle, rng=random.Random("%s/%s" % (scene, name)), device=dev,
                                    stream=stream)
            arrays["label." + name] = np.where(img.vert >= 0, vec[np.maximum(img.vert, 0)], -1).astype(np.int32)
    for b, view in enumerate(p["view_names"]):
        for name, _, _ in vectors:
            write_png(os.path.join(out_dir, "%s.%s.%s.png" % (scene, view, name)), coloured[name][b])
            tiles.append(coloured[name][b])
        if depth:
            write_png(os.path.join(out_dir, "%s.%s.depth.png" % (scene, view)), depth_mm(img.depth[b]))
    if p["sheet"] is not None:
        write_png(os.path.join(out_dir, scene + ".sheet.png"), contact_sheet(tiles, p["sheet"]))
    if npz:
        np.savez(os.path.join(out_dir, scene + NPZ_SUFFIX), **arrays)
    entry = dict(vertices=V, faces=0 if splats else int(faces.shape[0]), splats=splats, vertices_seen=int((img.hits > 0).sum()),
                 views={view: dict(covered=int((img.prim[b] >= 0).sum()), vertices_seen=int(np.unique(img.vert[b][img.vert[b] >= 0]).shape[0]))
                        for b, view in enumerate(p["view_names"])})
    entry.update(stats)
    return entry


def render_scans(scans_dir: str, out_dir: str, scenes=None, workers: int = 4, device=None, pointcloud=False, depth=False, npz=False, shuffle=False,
                 force=False, **options):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    <out_dir>/render_report.json.  `options` are check_command's; the refusals come before the device is asked for."""
    p = check_command(**options)
    dev = torch_device(device)
    if scenes is None and p["exp"] is not None:
        base = os.path.join(p["root"], "results", p["exp"])
        scenes = [s for s in scans.scan_names(scans_dir) if os.path.isdir(os.path.join(base, s, p["stage"]))]
    head = {"parameters": {k: v for k, v in p.items() if k != "cameras" and v is not None}}
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, head,
                           lambda path, stream: render_scan(path, out_dir, p, pointcloud, depth, npz, shuffle, force, dev, stream))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the images and render_report.json go (the report holds the primitive counts per scene, summed over its "
                    "views, and per view the covered pixels and the vertices seen)")
    ap.add_argument("-n", "--exp_name", default=None, help="experiment route: name of the experiment")
    ap.add_argument("--stage", default=None, help="experiment route: the export directory's name (default epoch_last)")
    ap.add_argument("--layer", nargs="+", default=None, metavar="VECTOR", help="experiment route: exported vectors, e.g. final.ins layer_2.seg (default final.ins)")
    ap.add_argument("--root", default=None, help="experiment route: directory holding results/ (default: CWD)")
    ap.add_argument("--labels-from", default=None, metavar="DIR", help="any per-vertex int vector: DIR/<scene><suffix>")
    ap.add_argument("--suffix", default=None, help="--labels-from: the file name after the scene's, ending in .npy or .npz")
    ap.add_argument("--key", default=None, help="--labels-from: the array of an .npz")
    ap.add_argument("--label-type", default=None, help="--labels-from: instance, semantic or segment (the colours `visualize` gives that type)")
    ap.add_argument("--rgb", action="store_true", help="the scan's own colours")
    ap.add_argument("--views", default="top", help="top (default) | orbit:N | poses:FILE.npz (T [B,3,4] or [B,4,4] world->camera, K [B,4] = fx fy cx cy with "
                    "pixel centres on halves: add 0.5 to ScanNet's cx, cy)")
    ap.add_argument("--size", nargs=2, type=int, default=(640, 480), metavar=("W", "H"))
    ap.add_argument("--ortho", action="store_true", help="orthographic orbit and pose views (top always is)")
    ap.add_argument("--elevation", type=float, default=30.0, metavar="DEG", help="orbit views: degrees above the horizon (negative: from below)")
    ap.add_argument("--near", type=float, default=0.05, metavar="D", help="a primitive with a vertex at or behind this depth is dropped")
    ap.add_argument("--point-size", type=int, default=3, metavar="P", help="splats: the side in pixels, odd, 1..15")
    ap.add_argument("--pointcloud", action="store_true", help="draw a scan with faces as splats too")
    ap.add_argument("--depth", action="store_true", help="also <scene>.<view>.depth.png, 16-bit millimetres")
    ap.add_argument("--npz", action="store_true", help="also <scene>.render.npz: prim, vert, depth, hits, cameras, label images")
    ap.add_argument("--sheet", type=int, default=None, metavar="COLS", help="also <scene>.sheet.png: all views x vectors, COLS a row")
    ap.add_argument("--shuffle", action="store_true", help="segment colours shuffled, seeded by scene and vector")
    scans.add_batch_arguments(ap, "overwrite the images of a scene that OUT holds already")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    options = dict(exp=a.exp_name, stage=a.stage, layers=a.layer, root=a.root, labels_from=a.labels_from, suffix=a.suffix, key=a.key,
                   label_type=a.label_type, rgb=a.rgb, views=a.views, size=tuple(a.size), ortho=a.ortho, elevation=a.elevation, near=a.near,
                   point_size=a.point_size, sheet=a.sheet)
    try:
        check_command(**options)
        report, skipped = render_scans(a.scans, a.out, scans.scene_list(a.scenes), a.workers, a.device, a.pointcloud, a.depth, a.npz, a.shuffle,
                                       a.force, **options)
    except ValueError as e:
        ap.error(str(e))
    scans.print_outcome(report, skipped, lambda scene, e: ("render", scene, e["vertices"], "vertices,", len(e["views"]), "views,", e["covered"],
                                                           "pixels covered,", e["vertices_seen"], "vertices seen"),
                        "(its first image is in --out: --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
