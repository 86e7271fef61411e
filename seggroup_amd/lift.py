"""2D label images onto a scan's vertices on the GPU: the way back from `render`.  ScanNet's label-filt / instance-filt frames,
a 2D network's output, an annotator's clicks in photographs are label IMAGES; this fuses them into one label per vertex.

    out = lift(xyz, cameras, labels, depth=depth, tol=0.05)             -- sg_lift + sg_lift_vote: Lift(label, votes, total, seen, tied), each [V]
    out = lift(xyz, cameras, labels, faces=faces, tol=0.05)             -- no depth images: the scan occludes itself (sg_render's depth, on the device)
    img = read_png(path); depth = depth_from_mm(read_png(path))         -- ScanNet's frames: 16-bit label-filt, 8-bit instance-filt, depth in mm

THE RULE (include/seggroup_hip.h; tests/lift_ref.py restates it): every vertex goes into every view by sg_render's own projection (the
same function), lands on the pixel (X >> 8, Y >> 8), and is VISIBLE iff that pixel's depth d is finite and > 0 and |c_2 - d| <= tol in
double; a visible vertex is seen, and votes with the pixel's label unless that is negative.  `label` is the label with the most votes, a tie
to the LOWEST label, -1 where no vote was cast, where votes < min_votes or where votes < min_share * total.  Exact and order-free: equality
with the restatement is the gate, and the same bytes come back on every run.  Any number of views: they go through in chunks of at most 64
views and 2^26 pixels into one table of counts, then one vote.  The camera convention is render's (x right, y DOWN, pixel centres on halves).

    python -m seggroup_amd.lift --scans DIR --out DIR ( --frames DIR | --scannet-frames DIR [--image-kind label-filt|instance-filt] [--every N] )
        --tol T [--min-votes M] [--min-share S] [--ortho] [--near D] [--point-size P] [--pointcloud] [--snap]
        [--style-name NAME --root ROOT --as ins|sem] [--scenes FILE --workers W --device D --force]
    --frames DIR reads DIR/<scene>.frames.npz: `T` [B,3,4] or [B,4,4] world->camera, `K` [B,4] = fx fy cx cy with pixel centres on halves (as
    `render --views poses:` takes them), `label` [B,H,W] whole numbers, optionally `depth` [B,H,W] float32 and `ortho`; without `depth` the
    scan occludes itself: every chunk of views is first drawn by sg_render (triangles; splats of --point-size for a face-less scan or with
    --pointcloud) and that depth is used.  --scannet-frames DIR reads what ScanNet's exporter leaves under DIR/<scene>/: pose/<f>.txt (camera
    to world, through render.from_pose), intrinsic/intrinsic_depth.txt, depth/<f>.png (16-bit millimetres) and <image-kind>/<f>.png, every
    N-th frame in numeric order; the label image is brought to the depth image's size by the integer nearest rule sx = ((2 x + 1) Ws) //
    (2 Wd); a frame whose pose holds a number that is not finite (lost tracking) is skipped and counted.  Written: OUT/<scene>.lift.npz (label,
    votes, total, seen, tied; with --snap label_snapped, constant on the scene's segments by majority) and OUT/lift_report.json: per scene
    the views used and skipped, the seven counts, the vertices seen, labelled and tied, with --snap the share moved.  --style-name NAME
    --root ROOT --as ins|sem also writes ROOT/label/seg/<NAME>/raw/<s>/<s>.{ins,sem}.txt and the resampled label.pth where the scene's
    map.pth exists, as `geodesic` does: the lifted vector (the snapped one with --snap) fills the file --as names, the OTHER file is -1
    throughout (one kind of image gives one vector; the report says so).  A scene whose .npz OUT holds already is skipped without --force.

Not here: reading .sens files, resizing by anything but the integer nearest rule, colour images and any 2D network, soft / weighted /
distance-dependent votes, a tolerance that grows with range, visibility by `vert` identity, clipping at the near plane, lifting onto
segments directly (--snap does that after the fact).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import struct
import sys
import threading
import zlib
from typing import NamedTuple

import numpy as np

from . import hip, render, scans
from .device import device_cloud, device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_VIEWS = render.MAX_VIEWS             # a call's; lift() takes any number, in chunks
MAX_PIXELS = render.MAX_PIXELS
MAX_CLASSES = 4096
MAX_CELLS = 1 << 31                      # V * C
STAT_NAMES = ("behind", "far", "outside", "nodepth", "occluded", "visible", "labelled")      # disjoint: `visible` is seen WITHOUT a vote
REPORT_NAME = "lift_report.json"
NPZ_SUFFIX = ".lift.npz"
FRAMES_SUFFIX = ".frames.npz"
IMAGE_KINDS = ("label-filt", "instance-filt")
_local = threading.local()


class Lift(NamedTuple):
    """lift's result, one value per vertex: `label` int32 (-1: none), `votes` the label's votes, `total` all votes cast for the vertex,
    `seen` the views that see it, `tied` 1 where another label holds as many votes (all int32)"""
    label: np.ndarray
    votes: np.ndarray
    total: np.ndarray
    seen: np.ndarray
    tied: np.ndarray


# ---- refusals (host) ----------------------------------------------------------------------------------------------------------------------------
def _number(x) -> bool:
    return not isinstance(x, (bool, str)) and isinstance(x, (int, float, np.integer, np.floating))


def check_tol(tol) -> float:
    if not _number(tol) or not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol (tol=, --tol) is needed: the depth tolerance in the unit of the coordinates, finite and >= 0, not %r" % (tol,))
    return float(tol)


def check_votes(min_votes, min_share):
    if isinstance(min_votes, bool) or not isinstance(min_votes, (int, np.integer)) or min_votes < 1:
        raise ValueError("min votes (min_votes=, --min-votes) is a whole number >= 1, not %r" % (min_votes,))
    if not _number(min_share) or not 0.0 <= float(min_share) <= 1.0:
        raise ValueError("min share (min_share=, --min-share) is a share of the votes in 0..1, not %r" % (min_share,))
    return int(min_votes), float(min_share)


def view_rows(cameras) -> np.ndarray:
    """a Camera, a sequence of them or [B,16] numbers, ANY B >= 1 -> float64 [B,16]; render.camera_rows' refusals, chunk by chunk"""
    if isinstance(cameras, render.Camera):
        cameras = [cameras]
    if cameras is None or len(cameras) == 0:
        raise ValueError("lift: cameras= is a Camera, a list of them or [B,16] numbers")
    rows = np.stack([c.row() for c in cameras]) if all(isinstance(c, render.Camera) for c in cameras) else np.asarray(cameras, np.float64)
    if rows.shape == (16,):
        rows = rows[None]
    if rows.ndim != 2 or rows.shape[1] != 16:
        raise ValueError("lift: cameras are [B,16] numbers (T row-major 3 x 4, fx fy cx cy), not %r" % (rows.shape,))
    return np.concatenate([render.camera_rows(rows[at:at + MAX_VIEWS]) for at in range(0, rows.shape[0], MAX_VIEWS)])


def check_images(labels, depth, B: int):
    """-> (labels int32 [B,H,W], depth float32 [B,H,W] or None)"""
    lab = np.asarray(labels)
    if lab.ndim != 3 or lab.shape[0] != B or not np.issubdtype(lab.dtype, np.integer) or lab.dtype == np.bool_:
        raise ValueError("lift: labels= is [B,H,W] whole numbers (negative: no label), one image per camera (%d), not %s %r" % (B, lab.dtype, lab.shape))
    H, W = int(lab.shape[1]), int(lab.shape[2])
    if not (1 <= W <= render.MAX_SIDE and 1 <= H <= render.MAX_SIDE):
        raise ValueError("lift: labels= are images of 1..%d pixels a side, not %d x %d" % (render.MAX_SIDE, W, H))
    if lab.size and (int(lab.max()) > 0x7fffffff or int(lab.min()) < -0x80000000):
        raise ValueError("lift: labels= holds a value outside int32")
    if depth is not None:
        depth = np.asarray(depth)
        if depth.shape != lab.shape or not np.issubdtype(depth.dtype, np.floating):
            raise ValueError("lift: depth= is [B,H,W] floats, the size of labels= %r, not %s %r" % (lab.shape, depth.dtype, depth.shape))
        depth = np.ascontiguousarray(depth, np.float32)
    return np.ascontiguousarray(lab, np.int32), depth


def label_classes(labels):
    """int [B,H,W] -> (cols int32 [B,H,W], values int64 [C]): the labels >= 0 ranked to the classes 0..C-1 in ascending order (a tie of the
    vote goes to the lowest class, so to the lowest label), everything negative to -1"""
    labels = np.asarray(labels)
    values = np.unique(labels[labels >= 0]).astype(np.int64)
    cols = np.where(labels >= 0, np.searchsorted(values, labels), -1).astype(np.int32)
    return cols, values


def view_chunks(B: int, W: int, H: int):
    """-> [(first, last + 1)]: at most 64 views and 2^26 pixels a chunk"""
    step = max(1, min(MAX_VIEWS, MAX_PIXELS // (W * H)))
    return [(at, min(at + step, B)) for at in range(0, B, step)]


def last_stats() -> dict:
    """the calling thread's last lift() / fuse(), SUMMED over its chunks -> {behind, far, outside, nodepth, occluded, visible, labelled}: disjoint
    kinds of (view, vertex) pairs that sum to B * V; `visible` is seen without a vote, `labelled` seen with one"""
    return dict(getattr(_local, "stats", dict.fromkeys(STAT_NAMES, 0)))


def call_stats() -> dict:
    """sg_lift_stats: the calling thread's last DEVICE call (one chunk)"""
    h = (C.c_int64 * len(STAT_NAMES))()
    hip.check(hip.lib().sg_lift_stats(h, len(STAT_NAMES)))
    return dict(zip(STAT_NAMES, (int(v) for v in h)))


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------------
def accumulate(d_xyz, rows, d_label, d_depth, tol, d_counts, d_seen, ortho=False, near=0.05, stream=None) -> dict:
    """ONE sg_lift call on device tensors: `rows` float64 [B <= 64, 16] (host), d_label int32 and d_depth float32 [B,H,W], d_counts int32
    [V,C] (read as uint32) and d_seen int32 [V], both ADDED to.  The caller holds the device and the stream (on_stream).  -> the call's
    seven counts.  A visible pixel's label >= C is the library's ValueError."""
    lib = hip.lib()
    B, H, W = (int(s) for s in d_label.shape)
    V, K = (int(s) for s in d_counts.shape)
    ws = workspace(lib.sg_lift_ws_bytes(V, B), d_counts.device)
    hip.check_arg(lib.sg_lift(d_xyz.data_ptr(), int(d_xyz.shape[1]), V, B, rows.ctypes.data, int(bool(ortho)), near, W, H, d_label.data_ptr(),
                              d_depth.data_ptr(), tol, K, d_counts.data_ptr(), d_seen.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
    return call_stats()


def vote(d_counts, stream=None):
    """sg_lift_vote on a device table int32 [V,C] -> (winner, votes, total, tied) int32 [V] device tensors; no synchronisation"""
    import torch
    V, K = (int(s) for s in d_counts.shape)
    out = [torch.empty(V, dtype=torch.int32, device=d_counts.device) for _ in range(4)]
    hip.check_arg(hip.lib().sg_lift_vote(d_counts.data_ptr(), V, K, *(t.data_ptr() for t in out), stream_ptr(stream)))
    return tuple(out)


def _self_depth(d_xyz, V, d_faces, point_size, rows, ortho, near, W, H, dev, stream):
    """sg_render of one chunk of views -> its depth image, ON THE DEVICE (+inf where empty)"""
    import torch
    lib = hip.lib()
    B = int(rows.shape[0])
    F = 0 if d_faces is None else int(d_faces.shape[0])
    d_prim = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    d_depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    ws = workspace(lib.sg_render_ws_bytes(V, F, B, W, H), dev)
    hip.check_arg(lib.sg_render(d_xyz.data_ptr(), int(d_xyz.shape[1]), V, hip.ptr(d_faces), F, point_size, B, rows.ctypes.data, int(bool(ortho)), near, W, H,
                                d_prim.data_ptr(), d_depth.data_ptr(), None, None, ws.data_ptr(), ws.numel(), stream_ptr(stream)))
    return d_depth


def fuse(xyz, cameras, classes, n_classes, depth=None, faces=None, tol=None, ortho=False, near=0.05, point_size=3, counts=None, seen=None, device=None,
         stream=None):
    """The views, chunk by chunk, into ONE table: `classes` int [B,H,W] holds classes already (negative: none; every other value below
    `n_classes`).  `counts` int32 [V,C] / `seen` int32 [V] (arrays or device tensors) are ADDED to where given, else start at zero.
    -> (d_counts int32 [V,C], d_seen int32 [V]) device tensors; last_stats() holds the chunks' sum.  The refusals are lift()'s."""
    tol, near, point_size = check_tol(tol), render.check_near(near), render.check_point_size(point_size)
    rows = view_rows(cameras)
    B = int(rows.shape[0])
    classes, depth = check_images(classes, depth, B)
    H, W = classes.shape[1:]
    if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError("lift: %r classes; the images hold 1..%d distinct labels" % (n_classes, MAX_CLASSES))
    if faces is not None:
        shape = tuple(faces.shape) if hasattr(faces, "shape") else np.shape(faces)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("lift: faces= are [F,3] vertex indices, not %r" % (shape,))
        if shape[0] > render.MAX_FACES:
            raise ValueError("lift: %d faces; a scan's own depth is drawn from at most 2^26" % shape[0])
        if shape[0] == 0:
            faces = None
    import torch
    dev = torch_device(device)
    _local.stats = dict.fromkeys(STAT_NAMES, 0)
    total = dict.fromkeys(STAT_NAMES, 0)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, V = device_cloud(xyz, dev, "lift")
        if V * int(n_classes) > MAX_CELLS:
            raise ValueError("lift: %d vertices x %d classes; the table of counts holds at most 2^31" % (V, n_classes))
        d_faces = None if faces is None or depth is not None else device_tensor(faces, torch.int32, dev)
        d_counts = torch.zeros((V, int(n_classes)), dtype=torch.int32, device=dev) if counts is None else device_tensor(counts, torch.int32, dev).clone()
        d_seen = torch.zeros(V, dtype=torch.int32, device=dev) if seen is None else device_tensor(seen, torch.int32, dev).clone()
        if tuple(d_counts.shape) != (V, int(n_classes)) or tuple(d_seen.shape) != (V,):
            raise ValueError("lift: counts= is [V,C] = [%d,%d] and seen= [%d], not %r and %r" % (V, n_classes, V, tuple(d_counts.shape), tuple(d_seen.shape)))
        for a, b in view_chunks(B, W, H):
            d_label = device_tensor(classes[a:b], torch.int32, dev)
            d_depth = device_tensor(depth[a:b], torch.float32, dev) if depth is not None else \
                _self_depth(d_xyz, V, d_faces, point_size, rows[a:b], ortho, near, W, H, dev, stream)
            one = accumulate(d_xyz, np.ascontiguousarray(rows[a:b]), d_label, d_depth, tol, d_counts, d_seen, ortho, near, stream)
            total = {k: total[k] + one[k] for k in total}
        _local.stats = total
        return d_counts, d_seen


def lift(xyz, cameras, labels, depth=None, faces=None, *, tol, ortho=False, near=0.05, point_size=3, min_votes=1, min_share=0.0, device=None,
         stream=None) -> Lift:
    """sg_lift over all views, then sg_lift_vote.  `xyz` [V, >= 3] (array or tensor; float32); `cameras` a Camera, a list of them or [B,16],
    any B >= 1; `labels` [B,H,W] whole numbers, negative: no label; `depth` [B,H,W] floats in the unit of the coordinates (0, NaN, inf:
    no depth there), or None: the scan is its own occluder, drawn by sg_render from `faces` [F,3] (or, without faces, as splats of side
    `point_size`).  `tol` has no default: it is the sensor's noise plus the mesh's error, a property of the data.  -> Lift of NumPy arrays."""
    min_votes, min_share = check_votes(min_votes, min_share)
    rows = view_rows(cameras)
    labels, depth = check_images(labels, depth, int(rows.shape[0]))
    cols, values = label_classes(labels)
    if values.shape[0] > MAX_CLASSES:
        raise ValueError("lift: labels= holds %d distinct labels; a vote takes at most %d" % (values.shape[0], MAX_CLASSES))
    d_counts, d_seen = fuse(xyz, rows, cols, max(int(values.shape[0]), 1), depth, faces, tol, ortho, near, point_size, device=device, stream=stream)
    import torch
    with torch.cuda.device(d_counts.device), on_stream(stream):
        winner, votes, total, tied = vote(d_counts, stream)
        sync(stream)
        winner, votes, total, tied, seen = (t.cpu().numpy() for t in (winner, votes, total, tied, d_seen))
    return finish(winner, votes, total, seen, tied, values, min_votes, min_share)


def finish(winner, votes, total, seen, tied, values, min_votes=1, min_share=0.0) -> Lift:
    """the vote's outputs -> Lift: classes back to labels, -1 where votes < min_votes or votes < min_share * total"""
    table = np.concatenate([np.asarray(values, np.int64), [-1]]).astype(np.int32)      # class -1 reads the last entry
    keep = (winner >= 0) & (votes >= min_votes) & ~(votes < min_share * total)
    return Lift(np.where(keep, table[winner], -1).astype(np.int32), votes, total, seen, tied)


# ---- images (host) ----------------------------------------------------------------------------------------------------------------------------
def _unfilter(kind: int, row: bytearray, prev: bytearray, bpp: int) -> None:
    n = len(row)
    if kind == 1:                                                                # Sub
        for i in range(bpp, n):
            row[i] = (row[i] + row[i - bpp]) & 255
    elif kind == 2:                                                              # Up
        for i in range(n):
            row[i] = (row[i] + prev[i]) & 255
    elif kind == 3:                                                              # Average
        for i in range(n):
            row[i] = (row[i] + (((row[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
    elif kind == 4:                                                              # Paeth
        for i in range(n):
            a, b, c = (row[i - bpp], prev[i], prev[i - bpp]) if i >= bpp else (0, prev[i], 0)
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            row[i] = (row[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
    elif kind != 0:
        raise ValueError("read_png: scanline filter %d; a PNG has the filters 0..4" % kind)


def read_png(path: str) -> np.ndarray:
    """8-bit grey -> uint8 [H,W]; 16-bit grey -> uint16 [H,W]; 8-bit RGB -> uint8 [H,W,3].  zlib of the standard library, all five scanline
    filters.  Interlaced, palette and every other colour type or depth is a ValueError that names it."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("read_png: %s is not a PNG" % path)
    at, idat, head = 8, [], None
    while at + 12 <= len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        body = raw[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(raw) or struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError("read_png: %s: the chunk %r is cut short or fails its CRC" % (path, kind))
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        at += 12 + n
    if head is None:
        raise ValueError("read_png: %s has no IHDR chunk" % path)
    W, H, bits, colour, comp, filt, lace = head
    if lace != 0:
        raise ValueError("read_png: %s is interlaced (Adam7); only images without interlace are read" % path)
    if colour == 3:
        raise ValueError("read_png: %s is a palette image; 8- and 16-bit grey and 8-bit RGB are read" % path)
    if (bits, colour) not in ((8, 0), (16, 0), (8, 2)) or comp != 0 or filt != 0:
        raise ValueError("read_png: %s has colour type %d at %d bits; 8- and 16-bit grey (type 0) and 8-bit RGB (type 2) are read" % (path, colour, bits))
    bpp = 3 if colour == 2 else bits // 8
    stride = W * bpp
    data = bytearray(zlib.decompress(b"".join(idat)))
    if W < 1 or H < 1 or len(data) != H * (stride + 1):
        raise ValueError("read_png: %s holds %d bytes for %d rows of %d" % (path, len(data), H, stride + 1))
    kinds = bytes(data[0::stride + 1])
    if any(kinds):
        prev = bytearray(stride)
        for y in range(H):
            row = data[y * (stride + 1) + 1:(y + 1) * (stride + 1)]
            _unfilter(kinds[y], row, prev, bpp)
            data[y * (stride + 1) + 1:(y + 1) * (stride + 1)] = row
            prev = row
    body = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8).reshape(H, stride + 1)[:, 1:])
    return body.reshape(H, W, 3) if colour == 2 else body.reshape(H, W) if bits == 8 else body.view(">u2").astype(np.uint16).reshape(H, W)


def depth_from_mm(img, scale: float = 1000.0) -> np.ndarray:
    """whole millimetres (ScanNet's depth frames; `scale` units a metre) -> float32 metres; 0 stays 0, which the rule calls NODEPTH"""
    a = np.asarray(img)
    if not np.issubdtype(a.dtype, np.integer) or not (_number(scale) and math.isfinite(scale) and scale > 0.0):
        raise ValueError("depth_from_mm: an image of whole numbers and a scale > 0, not %s and %r" % (a.dtype, scale))
    return (a.astype(np.float64) / float(scale)).astype(np.float32)


def resize_nearest(img, size) -> np.ndarray:
    """[Hs,Ws,...] -> [Hd,Wd,...] by the integer nearest rule: destination pixel x reads source pixel ((2 x + 1) Ws) // (2 Wd), likewise in y"""
    a = np.asarray(img)
    Wd, Hd = (int(s) for s in size)
    if a.ndim < 2 or a.shape[0] < 1 or a.shape[1] < 1 or Wd < 1 or Hd < 1:
        raise ValueError("resize_nearest: an image of at least one pixel and a size W H >= 1, not %r and %r" % (a.shape, tuple(size)))
    Hs, Ws = a.shape[:2]
    sx = ((2 * np.arange(Wd, dtype=np.int64) + 1) * Ws) // (2 * Wd)
    sy = ((2 * np.arange(Hd, dtype=np.int64) + 1) * Hs) // (2 * Hd)
    return np.ascontiguousarray(a[sy][:, sx])


# ---- frames -----------------------------------------------------------------------------------------------------------------------------------
class Frames(NamedTuple):
    """a scene's views: `rows` float64 [B,16], `label` int32 [B,H,W], `depth` float32 [B,H,W] or None, `ortho`, the frames' names and the
    names skipped"""
    rows: np.ndarray
    label: np.ndarray
    depth: object
    ortho: bool
    used: list
    skipped: list


def load_frames(path: str) -> Frames:
    """--frames: DIR/<scene>.frames.npz"""
    with np.load(path) as z:
        if any(k not in z.files for k in ("T", "K", "label")):
            raise ValueError("--frames: %s needs the arrays T, K and label (it has %s)" % (path, ", ".join(z.files)))
        T, K, label = np.asarray(z["T"], np.float64), np.asarray(z["K"], np.float64), np.asarray(z["label"])
        depth = np.asarray(z["depth"]) if "depth" in z.files else None
        ortho = bool(np.asarray(z["ortho"]).reshape(-1)[0]) if "ortho" in z.files else False
    if T.ndim != 3 or T.shape[1:] not in ((3, 4), (4, 4)) or K.shape != (T.shape[0], 4) or T.shape[0] < 1:
        raise ValueError("--frames: %s: T is [B,3,4] or [B,4,4] and K [B,4] with B >= 1, not %r and %r" % (path, T.shape, K.shape))
    rows = view_rows([render.Camera(t[:3], *(float(k) for k in row)) for t, row in zip(T, K)])
    label, depth = check_images(label, depth, int(rows.shape[0]))
    return Frames(rows, label, depth, ortho, ["frame%d" % b for b in range(rows.shape[0])], [])


def scannet_frame_names(scene_dir: str, every: int = 1):
    """the frames of DIR/<scene>/pose/<f>.txt in NUMERIC order, every `every`-th"""
    pose = os.path.join(scene_dir, "pose")
    if not os.path.isdir(pose):
        raise ValueError("--scannet-frames: %s is missing" % pose)
    stems = [f[:-4] for f in os.listdir(pose) if f.endswith(".txt") and f[:-4].isdigit()]
    return sorted(stems, key=lambda s: (int(s), s))[::every]


def _matrix(path: str) -> np.ndarray:
    if not os.path.exists(path):
        raise ValueError("--scannet-frames: %s is missing" % path)
    with open(path) as f:
        m = np.array([float(t) for t in f.read().split()], np.float64)       # float() reads inf, -inf and nan as the exporter writes them
    if m.size != 16:
        raise ValueError("--scannet-frames: %s holds %d numbers, not a 4 x 4 matrix" % (path, m.size))
    return m.reshape(4, 4)


def load_scannet_frames(scene_dir: str, image_kind: str = IMAGE_KINDS[0], every: int = 1) -> Frames:
    """--scannet-frames: DIR/<scene>/ as ScanNet's exporter leaves it"""
    K = _matrix(os.path.join(scene_dir, "intrinsic", "intrinsic_depth.txt"))
    cams, labels, depths, used, skipped = [], [], [], [], []
    for f in scannet_frame_names(scene_dir, every):
        P = _matrix(os.path.join(scene_dir, "pose", f + ".txt"))
        if not np.isfinite(P).all():                                             # lost tracking
            skipped.append(f)
            continue
        for kind in ("depth", image_kind):
            if not os.path.exists(os.path.join(scene_dir, kind, f + ".png")):
                raise ValueError("--scannet-frames: %s is missing" % os.path.join(scene_dir, kind, f + ".png"))
        d = read_png(os.path.join(scene_dir, "depth", f + ".png"))
        lab = read_png(os.path.join(scene_dir, image_kind, f + ".png"))
        if d.ndim != 2 or d.dtype != np.uint16 or lab.ndim != 2:
            raise ValueError("--scannet-frames: frame %s of %s: depth is 16-bit grey and %s grey, not %s %r and %s %r" %
                             (f, scene_dir, image_kind, d.dtype, d.shape, lab.dtype, lab.shape))
        if depths and d.shape != depths[0].shape:
            raise ValueError("--scannet-frames: frame %s of %s is %r, the frames before it %r" % (f, scene_dir, d.shape, depths[0].shape))
        cams.append(render.from_pose(P, K))
        depths.append(depth_from_mm(d))
        labels.append(resize_nearest(lab, (d.shape[1], d.shape[0])).astype(np.int32))
        used.append(f)
    if not used:
        raise ValueError("--scannet-frames: %s has no frame with a finite pose (%d skipped)" % (scene_dir, len(skipped)))
    return Frames(view_rows(cams), np.stack(labels), np.stack(depths), False, used, skipped)


# ---- scans --------------------------------------------------------------------------------------------------------------------------------------
def check_command(frames=None, scannet_frames=None, image_kind=None, every=None, tol=None, min_votes=1, min_share=0.0, ortho=False, near=0.05,
                  point_size=3, snap=False, style_name=None, root=None, as_=None, **_) -> dict:
    """every refusal of the command that needs no scan (ValueError naming the flag), before any device work -> the parameters in force"""
    if (frames is None) == (scannet_frames is None):
        raise ValueError("exactly one source of frames is needed: --frames DIR (<scene>.frames.npz) or --scannet-frames DIR (<scene>/pose, depth, ...)")
    if scannet_frames is None and (image_kind is not None or every is not None):
        raise ValueError("--image-kind and --every belong to --scannet-frames")
    image_kind = IMAGE_KINDS[0] if image_kind is None else image_kind
    if image_kind not in IMAGE_KINDS:
        raise ValueError("--image-kind is %s, not %r" % (" or ".join(IMAGE_KINDS), image_kind))
    every = 1 if every is None else every
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError("--every takes every N-th frame, N a whole number >= 1, not %r" % (every,))
    try:
        tol = check_tol(tol)
    except ValueError:
        raise ValueError("--tol is needed: the depth tolerance in the unit of the coordinates, finite and >= 0, not %r" % (tol,)) from None
    min_votes, min_share = check_votes(min_votes, min_share)
    if style_name is not None:
        if not style_name or style_name in (".", "..") or os.sep in style_name or "/" in style_name:
            raise ValueError("--style-name is the name of one directory under label/seg, not %r" % (style_name,))
        if root is None or as_ is None:
            raise ValueError("--style-name needs --root ROOT (label/seg/<NAME> is written under it) and --as ins|sem (the file the lifted labels fill)")
    elif as_ is not None:
        raise ValueError("--as belongs to --style-name")
    if as_ is not None and as_ not in ("ins", "sem"):
        raise ValueError("--as is ins or sem, not %r" % (as_,))
    return dict(frames=frames, scannet_frames=scannet_frames, image_kind=image_kind if scannet_frames is not None else None,
                every=int(every) if scannet_frames is not None else None, tol=tol, min_votes=min_votes, min_share=min_share, ortho=bool(ortho),
                near=render.check_near(near), point_size=render.check_point_size(point_size), snap=bool(snap), style_name=style_name, root=root, as_=as_)


def scene_frames(scene: str, p: dict) -> Frames:
    if p["frames"] is not None:
        path = os.path.join(p["frames"], scene + FRAMES_SUFFIX)
        if not os.path.exists(path):
            raise ValueError("%s: --frames: %s is missing" % (scene, path))
        return load_frames(path)
    return load_scannet_frames(os.path.join(p["scannet_frames"], scene), p["image_kind"], p["every"])


def segment_file(scene_path: str, root) -> str:
    """--snap: the scene's segments, in the scan directory or under the root"""
    scene = scans.scene_name(scene_path)
    cands = [os.path.join(scene_path, scene + "_vh_clean_2.0.010000.segs.json")]
    if root is not None:
        cands.append(os.path.join(root, "label", "real", "raw", scene, scene + ".seg.txt"))
    found = [c for c in cands if os.path.exists(c)]
    if not found:
        raise ValueError("%s: --snap needs the scene's segments: %s is not there" % (scene, " nor ".join(cands)))
    return found[0]


def lift_scan(scene_path: str, out_dir: str, p: dict, pointcloud=False, force=False, device=None, stream=None):
    """One scan directory -> OUT/<scene>.lift.npz (and the label files of --style-name) -> its entry of lift_report.json, or None when the
    .npz was there already (never overwritten without `force`).  `p` is check_command's."""
    from . import labels as L
    from .prepare import mesh_arrays, read_ply
    scene = scans.scene_name(scene_path)
    out = os.path.join(out_dir, scene + NPZ_SUFFIX)
    if os.path.exists(out) and not force:
        return None
    seg_path = segment_file(scene_path, p["root"]) if p["snap"] else None
    xyz, _, faces = mesh_arrays(read_ply(os.path.join(scene_path, scene + scans.PLY_SUFFIX)))
    V = int(xyz.shape[0])
    fr = scene_frames(scene, p)
    splats = bool(pointcloud) or faces.shape[0] == 0
    ortho = p["ortho"] or fr.ortho
    res = lift(xyz, fr.rows, fr.label, fr.depth, None if splats else faces, tol=p["tol"], ortho=ortho, near=p["near"], point_size=p["point_size"],
               min_votes=p["min_votes"], min_share=p["min_share"], device=device, stream=stream)
    stats = last_stats()
    arrays = res._asdict()
    entry = dict(vertices=V, views=len(fr.used), views_skipped=len(fr.skipped), image=[int(fr.label.shape[2]), int(fr.label.shape[1])], ortho=bool(ortho),
                 occluder="depth images" if fr.depth is not None else "the scan, as splats" if splats else "the scan's faces",
                 vertices_seen=int((res.seen > 0).sum()), vertices_labelled=int((res.label >= 0).sum()), vertices_tied=int((res.tied > 0).sum()))
    entry.update(stats)
    final = res.label
    if p["snap"]:
        from .geodesic import snap_to_segments
        seg = np.asarray(L.load_labels(seg_path), dtype=np.int64)
        if seg.shape[0] != V:
            raise ValueError("%s: %s holds %d segment ids for %d vertices" % (scene, seg_path, seg.shape[0], V))
        final, entry["moved"] = snap_to_segments(seg, res.label, device=device, stream=stream)
        arrays["label_snapped"] = final.astype(np.int32)
    os.makedirs(out_dir, exist_ok=True)
    np.savez(out, **arrays)
    if p["style_name"] is not None:
        raw = os.path.join(p["root"], "label", "seg", p["style_name"], "raw", scene)
        other = "sem" if p["as_"] == "ins" else "ins"
        L._write_txt(os.path.join(raw, "%s.%s.txt" % (scene, p["as_"])), final)
        L._write_txt(os.path.join(raw, "%s.%s.txt" % (scene, other)), np.full(V, -1, np.int32))
        entry["style"] = "%s.txt holds the lifted labels, %s.txt is -1 throughout: one kind of image gives one vector" % (p["as_"], other)
        if os.path.exists(os.path.join(p["root"], "data", "resampled", scene, scene + ".map.pth")):
            L.generate_weak_label_pth(scene, p["style_name"], p["root"])
            entry["resampled"] = "written"
        else:
            entry["resampled"] = "not written: no data/resampled/%s/%s.map.pth under the root" % (scene, scene)
    return entry


def lift_scans(scans_dir: str, out_dir: str, scenes=None, workers: int = 4, device=None, pointcloud=False, force=False, **options):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    <out_dir>/lift_report.json.  `options` are check_command's; the refusals come before the device is asked for."""
    p = check_command(**options)
    dev = torch_device(device)
    head = {"parameters": {k.rstrip("_"): v for k, v in p.items() if v is not None}}
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, head,
                           lambda path, stream: lift_scan(path, out_dir, p, pointcloud, force, dev, stream))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.lift", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--out", required=True, metavar="DIR", help="where <scene>.lift.npz and lift_report.json go")
    ap.add_argument("--frames", default=None, metavar="DIR", help="DIR/<scene>.frames.npz: T, K (pixel centres on halves), label, optionally depth and ortho")
    ap.add_argument("--scannet-frames", default=None, metavar="DIR", help="DIR/<scene>/{pose,depth,<image-kind>}/<f>.* and intrinsic/intrinsic_depth.txt")
    ap.add_argument("--image-kind", default=None, help="--scannet-frames: label-filt (default) or instance-filt")
    ap.add_argument("--every", type=int, default=None, metavar="N", help="--scannet-frames: every N-th frame in numeric order (default 1)")
    ap.add_argument("--tol", type=float, default=None, metavar="T", help="a vertex is seen where |its depth - the image's| <= T, in the unit of the coordinates")
    ap.add_argument("--min-votes", type=int, default=1, metavar="M", help="a label needs at least M votes (default 1)")
    ap.add_argument("--min-share", type=float, default=0.0, metavar="S", help="a label needs at least this share of its vertex's votes, 0..1 (default 0)")
    ap.add_argument("--ortho", action="store_true", help="orthographic views (a .frames.npz may say so itself)")
    ap.add_argument("--near", type=float, default=0.05, metavar="D", help="a vertex at or behind this depth is not projected")
    ap.add_argument("--point-size", type=int, default=3, metavar="P", help="the scan as its own occluder, splats: the side in pixels, odd, 1..15")
    ap.add_argument("--pointcloud", action="store_true", help="the scan as its own occluder: draw a scan with faces as splats too")
    ap.add_argument("--snap", action="store_true", help="also label_snapped: constant on the scene's segments, by majority")
    ap.add_argument("--style-name", default=None, metavar="NAME", help="also write the labels as the label style label/seg/<NAME> under --root")
    ap.add_argument("--root", default=None, help="the dataset root of --style-name (and of --snap's label/real/raw/<s>/<s>.seg.txt)")
    ap.add_argument("--as", dest="as_", default=None, metavar="ins|sem", help="--style-name: the file the lifted labels fill; the other is -1 throughout")
    scans.add_batch_arguments(ap, "overwrite the files of a scene that OUT holds already")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    options = dict(frames=a.frames, scannet_frames=a.scannet_frames, image_kind=a.image_kind, every=a.every, tol=a.tol, min_votes=a.min_votes,
                   min_share=a.min_share, ortho=a.ortho, near=a.near, point_size=a.point_size, snap=a.snap, style_name=a.style_name, root=a.root, as_=a.as_)
    try:
        check_command(**options)
        report, skipped = lift_scans(a.scans, a.out, scans.scene_list(a.scenes), a.workers, a.device, a.pointcloud, a.force, **options)
    except ValueError as e:
        ap.error(str(e))
    scans.print_outcome(report, skipped, lambda scene, e: ("lift", scene, e["vertices"], "vertices,", e["views"], "views,", e["vertices_seen"], "seen,",
                                                           e["vertices_labelled"], "labelled,", e["vertices_tied"], "tied"),
                        "(its .lift.npz is in --out: --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
