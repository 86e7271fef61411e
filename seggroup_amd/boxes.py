"""Boxes of labelled points on the GPU: any per-vertex integer vector -- instances, components, planes -- turned into one
count, centre, extent and box per value.

    index   = label_index(labels)                       -- sg_label_index: the labelled points (labels >= 0) by label, ascending index
                                                           within a label; the distinct values and their offsets
    m       = label_moments(xyz, index)                 -- sg_label_moments: count | sum q | sum q q^T per label (q = p - the label's
                                                           first point) on fixed trees, the float minima and maxima per axis
    yaw     = yaw_boxes(xyz, index, angles)             -- sg_label_yaw_boxes: the footprint extents at `angles` steps of (pi/2)/angles
                                                           about z, the step of least area
    R       = box_axes(m.moments[l])                    -- sg_box_axes (host): the label's principal frame
    ext     = frame_extents(xyz, index, R)              -- sg_label_frame_extents: the extents in each label's own frame

`label_boxes` puts them together for `kind` = "aabb" (axis-aligned), "yaw" (the upright box of least footprint over the sweep; z is up:
`planes --level` makes such a scan) or "pca".  Minima and maxima are exact and the index is integers, so the boxes of kind aabb and yaw
are the same on every run to the last bit; the sums are deterministic.

    python -m seggroup_amd.boxes --scans DIR --out DIR
        ( -n EXP --stage S [--layer final] [--root .]            # <layer>.ins, class = <layer>.sem at the instance's lowest vertex
        | --labels-from DIR --suffix .planes.npz --key labels )   # any per-vertex int vector: DIR/<scene><suffix>[key]; .npy: no --key
        [--kind aabb|yaw|pca] [--angles A] [--min-points M] [--classes scannet18|all]
        [--detector-files] [--ply] [--scenes FILE --workers W --device D --force]
    per scene OUT/<scene>.boxes.npz (Boxes.arrays(), and `sem` where there is one) and one OUT/boxes_report.json (per scene V, instances,
    kept, ignored vertices, kind and the parameters).  On the experiment route ins <= 0 is ignored, --min-points defaults to 100 and
    --classes to scannet18 (AP's rules); on the --labels-from route negative labels are ignored, --min-points has no default and there are
    no classes.  --detector-files: OUT/<scene>_bbox.npy, float64 [K,7] = centre (3), full size (3), class id -- axis-aligned from lo / hi
    whatever --kind is.  --ply: OUT/<scene>.boxes.ply, 8 vertices and 12 triangles per kept box in the label palette.

Not here: exact minimum-area rectangles (rotating calipers on a hull), merging or splitting instances, an up axis other than z; box IoU
and detection mAP against ground-truth boxes are `python -m seggroup_amd.boxap` (seggroup_amd/boxap.py); which boxes hold a
point, and weak labels from boxes, are `python -m seggroup_amd.boxlabels` (seggroup_amd/boxlabels.py); removing stacked or
duplicate boxes (non-maximum suppression) is `python -m seggroup_amd.boxnms` (seggroup_amd/boxnms.py).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import sys
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import hip, scans
from .boxset import NPY_SUFFIX, NPZ_SUFFIX                                     # the two files written here; boxset.py reads them
from .device import device_rows, device_tensor, on_stream, stream_ptr, sync, torch_device, workspace

MAX_POINTS = 1 << 24
MAX_ANGLES = 1024
DEFAULT_ANGLES = 90
KINDS = ("aabb", "yaw", "pca")
REPORT_NAME = "boxes_report.json"
AP_MIN_POINTS = 100
# the corners of a box, corner k at (+/-, +/-, +/-) half sizes with bit a of k the sign on axis a, and 12 triangles over them
CORNER_SIGNS = np.array([[(k >> a & 1) * 2 - 1 for a in range(3)] for k in range(8)], np.float64)
BOX_FACES = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5],
                      [3, 7, 5]], np.int32)


class LabelIndex(NamedTuple):
    """label_index's result: device tensors `order` int32 [M], `values` int32 [L], `start` int32 [L + 1], and how many points were ignored"""
    order: object
    values: object
    start: object
    ignored: int


class Moments(NamedTuple):
    """label_moments' result, device tensors: `moments` float64 [L,10], `lo` / `hi` float32 [L,3]"""
    moments: object
    lo: object
    hi: object


@dataclass
class Boxes:
    """What label_boxes returns, one row per kept label in ascending value.  `values` int32; `count` int64; `first` int32, the label's
    lowest vertex index; `lo`, `hi` float32 [L,3]; `centroid` float64 [L,3] = p_first + sum q / count; `cov` float64 [L,6] (xx xy xz yy
    yz zz); `R` float64 [L,3,3], rows are the box axes (identity for aabb, the z-rotation for yaw); `center` [L,3] in the world; `size`
    [L,3] along the rows of R; `yaw` radians (NaN unless kind is yaw).  The rest are the parameters used (`angles` 0 unless yaw)."""
    values: np.ndarray
    count: np.ndarray
    first: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    centroid: np.ndarray
    cov: np.ndarray
    R: np.ndarray
    center: np.ndarray
    size: np.ndarray
    yaw: np.ndarray
    kind: str
    angles: int
    min_points: int

    def arrays(self) -> dict:
        """everything as arrays, as <scene>.boxes.npz holds it"""
        out = {k: getattr(self, k) for k in ("values", "count", "first", "lo", "hi", "centroid", "cov", "R", "center", "size", "yaw")}
        out.update(kind=np.array(self.kind), angles=np.int32(self.angles), min_points=np.int64(self.min_points))
        return out

    def corners(self) -> np.ndarray:
        """float64 [L,8,3]: corner k = center + sum_a sign(k, a) * size[a] / 2 * R[a], bit a of k set: the positive side of axis a"""
        half = CORNER_SIGNS[None, :, :] * (0.5 * self.size)[:, None, :]                     # [L,8,3] in the box frame
        return self.center[:, None, :] + np.einsum("lka,lac->lkc", half, self.R)


def label_index(labels, device=None, stream=None) -> LabelIndex:
    """sg_label_index of an int vector [N] -> LabelIndex.  A point is labelled when its label is >= 0."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_lab = device_tensor(labels, torch.int32, dev)
        if d_lab.dim() != 1:
            raise ValueError("label_index: labels are one integer per point, [N]")
        n = int(d_lab.shape[0])
        need = lib.sg_label_index_ws_bytes(n)
        if need == 0:
            raise hip.SgError(hip.SG_EUNSUP, "label_index: %d points; a call takes at most 2^24" % n)
        order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        values = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        start = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ws = workspace(need, dev)
        count, ignored = C.c_int(0), C.c_int(0)
        hip.check_arg(lib.sg_label_index(d_lab.data_ptr() if n else None, n, order.data_ptr(), values.data_ptr(), start.data_ptr(),
                                         C.byref(count), C.byref(ignored), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
        l, m = int(count.value), n - int(ignored.value)
        return LabelIndex(order[:m], values[:l], start[:l + 1], int(ignored.value))


def _sizes(d_xyz, index: LabelIndex, who: str):
    n, l = int(d_xyz.shape[0]), int(index.values.shape[0])
    if int(index.start.shape[0]) != l + 1 or int(index.order.shape[0]) + int(index.ignored) != n:
        raise ValueError("%s: the index is not one of this cloud (%d points)" % (who, n))
    return n, l


def label_moments(xyz, index: LabelIndex, device=None, stream=None) -> Moments:
    """sg_label_moments -> Moments.  A labelled point with a coordinate that is not finite is a ValueError."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "label_moments", MAX_POINTS)
        n, l = _sizes(d_xyz, index, "label_moments")
        m = torch.empty((l, 10), dtype=torch.float64, device=dev)
        lo = torch.empty((l, 3), dtype=torch.float32, device=dev)
        hi = torch.empty((l, 3), dtype=torch.float32, device=dev)
        ws = workspace(lib.sg_label_moments_ws_bytes(n, l), dev)
        if l:
            hip.check_arg(lib.sg_label_moments(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, index.order.data_ptr(), index.start.data_ptr(), l,
                                               m.data_ptr(), lo.data_ptr(), hi.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return Moments(m, lo, hi)


def check_angles(angles, who: str = "yaw_boxes") -> int:
    if isinstance(angles, bool) or not isinstance(angles, (int, np.integer)) or not 1 <= int(angles) <= MAX_ANGLES:
        raise ValueError("%s: angles (angles=, --angles) is a whole number of steps in 1..%d, not %r" % (who, MAX_ANGLES, angles))
    return int(angles)


def angle_table(angles: int) -> np.ndarray:
    """float64 [A,2]: (cos, sin) of a * (pi/2) / A, taken on the host in double"""
    theta = np.arange(angles, dtype=np.float64) * ((math.pi / 2.0) / angles)
    return np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta)], 1))


def yaw_boxes(xyz, index: LabelIndex, angles=DEFAULT_ANGLES, cs=None, all_extents: bool = False, device=None, stream=None):
    """sg_label_yaw_boxes -> (best int32 [L], ext float64 [L,4] = umin umax vmin vmax at best, all float64 [L,A,4] or None), device tensors.
    `cs` float64 [A,2] replaces the table of `angles` steps over a quarter turn."""
    import torch
    if cs is None:
        cs = angle_table(check_angles(angles))
    cs = np.ascontiguousarray(cs, dtype=np.float64)
    if cs.ndim != 2 or cs.shape[1] != 2 or not 1 <= cs.shape[0] <= MAX_ANGLES or not np.isfinite(cs).all():
        raise ValueError("yaw_boxes: cs is [A,2] finite (cos, sin) rows, 1 <= A <= %d" % MAX_ANGLES)
    a = int(cs.shape[0])
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "yaw_boxes", MAX_POINTS)
        n, l = _sizes(d_xyz, index, "yaw_boxes")
        best = torch.empty(l, dtype=torch.int32, device=dev)
        ext = torch.empty((l, 4), dtype=torch.float64, device=dev)
        every = None
        if all_extents:
            if l * a > 1 << 24:
                raise hip.SgError(hip.SG_EUNSUP, "yaw_boxes: all_extents holds at most 2^24 (label, angle) rows (%d x %d)" % (l, a))
            every = torch.empty((l, a, 4), dtype=torch.float64, device=dev)
        ws = workspace(lib.sg_label_yaw_boxes_ws_bytes(n, l, a), dev)
        if l:
            hip.check_arg(lib.sg_label_yaw_boxes(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, index.order.data_ptr(), index.start.data_ptr(), l,
                                                 cs.ctypes.data, a, best.data_ptr(), ext.data_ptr(), hip.ptr(every), ws.data_ptr(), ws.numel(),
                                                 stream_ptr(stream)))
        sync(stream)
    return best, ext, every


def frame_extents(xyz, index: LabelIndex, frames, device=None, stream=None):
    """sg_label_frame_extents: `frames` float64 [L,3,3] -> float64 [L,6] device tensor, min and max of dot(row_k, p) for k = 0, 1, 2"""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "frame_extents", MAX_POINTS)
        n, l = _sizes(d_xyz, index, "frame_extents")
        d_fr = device_tensor(frames, torch.float64, dev)
        if tuple(d_fr.shape) not in ((l, 3, 3), (l, 9)):
            raise ValueError("frame_extents: one 3 x 3 frame per label, [%d,3,3]" % l)
        ext = torch.empty((l, 6), dtype=torch.float64, device=dev)
        ws = workspace(lib.sg_label_frame_extents_ws_bytes(n, l), dev)
        if l:
            hip.check_arg(lib.sg_label_frame_extents(d_xyz.data_ptr(), int(d_xyz.shape[1]), n, index.order.data_ptr(), index.start.data_ptr(), l,
                                                     d_fr.data_ptr(), ext.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    return ext


def box_axes(m):
    """sg_box_axes (host only, runs without a GPU): one row of label_moments' sums -> (R float64 [3,3], eig float64 [3]): the eigenvectors
    of the label's covariance as rows, by descending eigenvalue, rows 0 and 1 with their largest-magnitude component positive, row 2 their
    cross product.  One point, or points that coincide, get the identity.  count < 1 or a non-finite moment is a ValueError."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (10,):
        raise ValueError("box_axes: 10 moments")
    r, eig = np.zeros(9), np.zeros(3)
    hip.check_arg(hip.lib().sg_box_axes(m.ctypes.data, r.ctypes.data, eig.ctypes.data))
    return r.reshape(3, 3), eig


def check_box_parameters(kind, angles, min_points) -> tuple:
    """what label_boxes and the command refuse before anything runs (ValueError) -> (kind, angles or 0, min_points)"""
    if kind not in KINDS:
        raise ValueError("label_boxes: kind (kind=, --kind) is one of %s, not %r" % (", ".join(KINDS), kind))
    if angles is not None and kind != "yaw":
        raise ValueError("label_boxes: angles (angles=, --angles) belongs to kind yaw, not to %s" % kind)
    a = check_angles(DEFAULT_ANGLES if angles is None else angles, "label_boxes") if kind == "yaw" else 0
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or int(min_points) < 1:
        raise ValueError("label_boxes: min_points (min_points=, --min-points) is a whole number >= 1, not %r" % (min_points,))
    return kind, a, int(min_points)


def _check_pair(xyz, labels) -> None:
    xs, ls = (tuple(v.shape) if hasattr(v, "shape") else np.shape(v) for v in (xyz, labels))
    if len(xs) != 2 or xs[1] < 3:
        raise ValueError("label_boxes: a cloud is [N, >= 3] rows with xyz first")
    if ls != (xs[0],):
        raise ValueError("label_boxes: labels must be [%d], one per point, not %r" % (xs[0], ls))


def assemble(kind: str, angles: int, min_points: int, values, start, order_first, m, lo, hi, p_first, best=None, ext=None, R=None) -> Boxes:
    """Host arithmetic from the reductions to Boxes, in double, one NumPy statement per operation (tests/boxes_ref.py states the same):
    `m` [L,10], `lo` / `hi` float32 [L,3], `p_first` float32 [L,3]; yaw: `best` [L] and `ext` [L,4]; pca: `R` [L,3,3] and `ext` [L,6]."""
    l = int(values.shape[0])
    count = m[:, 0].astype(np.int64)
    n = m[:, 0][:, None]
    mean_q = m[:, 1:4] / n
    centroid = p_first.astype(np.float64) + mean_q
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = np.stack([(m[:, 4 + k] - m[:, 1 + r] * m[:, 1 + c] / m[:, 0]) / m[:, 0] for k, (r, c) in enumerate(pairs)], 1) if l else np.zeros((0, 6))
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    yaw = np.full(l, np.nan)
    if kind == "aabb":
        R = np.tile(np.eye(3), (l, 1, 1))
        mins, maxs = lo64, hi64
    elif kind == "yaw":
        theta = best.astype(np.float64) * ((math.pi / 2.0) / angles)
        c, s = np.cos(theta), np.sin(theta)
        R = np.zeros((l, 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, s, -s, c, 1.0
        mins = np.stack([ext[:, 0], ext[:, 2], lo64[:, 2]], 1)
        maxs = np.stack([ext[:, 1], ext[:, 3], hi64[:, 2]], 1)
        yaw = theta
    else:
        R = np.asarray(R, np.float64).reshape(l, 3, 3)
        mins, maxs = ext[:, 0::2], ext[:, 1::2]
    mid = 0.5 * (mins + maxs)
    size = maxs - mins
    center = (mid[:, 0:1] * R[:, 0, :] + mid[:, 1:2] * R[:, 1, :]) + mid[:, 2:3] * R[:, 2, :]
    keep = count >= min_points
    return Boxes(values=values[keep].astype(np.int32), count=count[keep], first=order_first[keep].astype(np.int32), lo=lo[keep], hi=hi[keep],
                 centroid=centroid[keep], cov=cov[keep], R=R[keep], center=center[keep], size=size[keep], yaw=yaw[keep], kind=kind,
                 angles=angles, min_points=min_points)


def label_boxes(xyz, labels, kind="yaw", angles=None, min_points=1, device=None, stream=None) -> Boxes:
    """One box per distinct label >= 0 of `labels` [N] over the cloud `xyz` [N, >= 3] -> Boxes.  `kind`: "aabb", "yaw" (`angles` steps of
    (pi/2)/angles about z, default 90) or "pca".  `min_points` drops smaller labels from the RESULT: the kernels see every label.  A shape
    mismatch, angles outside 1..1024, an unknown kind and angles with a kind other than yaw are refused before any device call."""
    import torch
    kind, a, min_points = check_box_parameters(kind, angles, min_points)
    _check_pair(xyz, labels)
    dev = torch_device(device)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz = device_rows(xyz, dev, "label_boxes", MAX_POINTS)
    index = label_index(labels, dev, stream)
    mom = label_moments(d_xyz, index, dev, stream)
    best = ext = frames = None
    with torch.cuda.device(dev), on_stream(stream):
        m, lo, hi = mom.moments.cpu().numpy(), mom.lo.cpu().numpy(), mom.hi.cpu().numpy()
        values, start = index.values.cpu().numpy(), index.start.cpu().numpy()
        first = index.order[index.start[:-1].long()].cpu().numpy() if values.shape[0] else np.zeros(0, np.int32)
        p_first = d_xyz[torch.from_numpy(first).to(dev).long(), :3].cpu().numpy()
    if kind == "yaw":
        d_best, d_ext, _ = yaw_boxes(d_xyz, index, a, device=dev, stream=stream)
        with torch.cuda.device(dev), on_stream(stream):
            best, ext = d_best.cpu().numpy(), d_ext.cpu().numpy()
    elif kind == "pca":
        frames = np.stack([box_axes(row)[0] for row in m]) if m.shape[0] else np.zeros((0, 3, 3))
        d_ext = frame_extents(d_xyz, index, frames, dev, stream)
        with torch.cuda.device(dev), on_stream(stream):
            ext = d_ext.cpu().numpy()
    return assemble(kind, a, min_points, values, start, first, m, lo, hi, p_first, best, ext, frames)


# ---- scans ----------------------------------------------------------------------------------------------------------------------------
def check_command(exp, labels_from, suffix, key, kind, angles, min_points, classes, detector_files) -> tuple:
    """the combinations of the command's options that are refused before anything runs (ValueError) -> (kind, angles, min_points, classes)"""
    if (exp is None) == (labels_from is None):
        raise ValueError("exactly one source of labels is needed: -n EXP (with --stage) or --labels-from DIR (with --suffix)")
    if exp is not None:
        if suffix is not None or key is not None:
            raise ValueError("--suffix and --key belong to --labels-from")
        if min_points is None:
            min_points = AP_MIN_POINTS
        if classes is None:
            classes = "scannet18"
    else:
        if suffix is None:
            raise ValueError("--labels-from needs --suffix (the file is DIR/<scene><suffix>)")
        if suffix.endswith(".npy") and key is not None:
            raise ValueError("--key names an array of an .npz: a .npy holds one vector")
        if suffix.endswith(".npz") and key is None:
            raise ValueError("--suffix names an .npz: --key (the array in it) is needed")
        if not suffix.endswith((".npy", ".npz")):
            raise ValueError("--suffix must end in .npy or .npz")
        if classes is not None:
            raise ValueError("--classes needs the classes of an experiment (-n EXP): --labels-from has none")
        if detector_files:
            raise ValueError("--detector-files writes a class id per box: --labels-from has no classes")
        if min_points is None:
            raise ValueError("--min-points (min_points=) is required with --labels-from: the fewest points of a box depends on what the labels "
                             "are; there is no default")
    if classes not in (None, "scannet18", "all"):
        raise ValueError("--classes is scannet18 or all, not %r" % (classes,))
    kind, a, min_points = check_box_parameters(kind, angles, min_points)
    return kind, a, min_points, classes


def scene_labels(scene: str, n: int, exp=None, stage="epoch_last", layer="final", root=".", labels_from=None, suffix=None, key=None):
    """-> (labels int32 [V] with the ignored vertices negative, sem int32 [V] or None)"""
    if exp is not None:
        from . import pseudo_labels
        lab = pseudo_labels.load(os.path.join(root, "results", exp, scene, stage))
        ins, sem = lab.vector(layer + ".ins"), lab.vector(layer + ".sem")
        labels = np.where(ins > 0, ins, -1).astype(np.int32)                # AP's rule: instance ids start at 1
    else:
        path = os.path.join(labels_from, scene + suffix)
        if suffix.endswith(".npy"):
            vec = np.load(path)
        else:
            with np.load(path) as z:
                if key not in z.files:
                    raise ValueError("%s has no array %r (it has %s)" % (path, key, ", ".join(z.files)))
                vec = z[key]
        if vec.ndim != 1 or not np.issubdtype(vec.dtype, np.integer):
            raise ValueError("%s: a per-vertex integer vector is needed, not %s %r" % (path, vec.dtype, vec.shape))
        if vec.size and (int(vec.max()) > 0x7fffffff or int(vec.min()) < -0x80000000):
            raise ValueError("%s: a label outside int32" % path)
        labels, sem = vec.astype(np.int32), None
    if labels.shape[0] != n:
        raise ValueError(f"{scene}: {labels.shape[0]} labels for {n} vertices")
    return labels, sem


def detector_rows(boxes: Boxes, sem) -> np.ndarray:
    """float64 [K,7] = centre, full size, class id; axis-aligned from lo / hi whatever the kind"""
    lo, hi = boxes.lo.astype(np.float64), boxes.hi.astype(np.float64)
    return np.concatenate([0.5 * (lo + hi), hi - lo, np.asarray(sem, np.float64).reshape(-1, 1)], 1)


def box_mesh(boxes: Boxes):
    """-> (xyz float32 [8K,3], rgb uint8 [8K,3], faces int32 [12K,3]): every box as 12 triangles, coloured by its value in the label palette"""
    from .visualize import colors, num_colors
    k = int(boxes.values.shape[0])
    xyz = boxes.corners().reshape(-1, 3).astype(np.float32)
    palette = np.asarray(colors, np.uint8)
    rgb = np.repeat(palette[1 + boxes.values.astype(np.int64) % num_colors], 8, 0).reshape(-1, 3)
    faces = (BOX_FACES[None, :, :] + 8 * np.arange(k, dtype=np.int32)[:, None, None]).reshape(-1, 3).astype(np.int32)
    return xyz, rgb, faces


def boxes_scan(scene_path: str, out_dir: str, exp=None, stage="epoch_last", layer="final", root=".", labels_from=None, suffix=None, key=None,
               kind="yaw", angles=None, min_points=None, classes=None, detector_files: bool = False, ply: bool = False, force: bool = False,
               device=None, stream=None):
    """One scan directory -> <out_dir>/<scene>.boxes.npz (and _bbox.npy / .boxes.ply) -> its entry of boxes_report.json, or None when the
    .npz was there already (never overwritten without `force`)."""
    from .prepare import mesh_arrays, read_ply, write_ply
    kind, a, min_points, classes = check_command(exp, labels_from, suffix, key, kind, angles, min_points, classes, detector_files)
    scene = scans.scene_name(scene_path)
    npz = os.path.join(out_dir, scene + NPZ_SUFFIX)
    if os.path.exists(npz) and not force:
        return None
    xyz = mesh_arrays(read_ply(os.path.join(scene_path, scene + scans.PLY_SUFFIX)))[0]
    labels, sem = scene_labels(scene, int(xyz.shape[0]), exp, stage, layer, root, labels_from, suffix, key)
    found = label_boxes(xyz, labels, kind, a if kind == "yaw" else None, 1, device=device, stream=stream)
    instances = int(found.values.shape[0])
    keep = found.count >= min_points
    box_sem = None
    if sem is not None:
        box_sem = sem[found.first].astype(np.int32)
        if classes == "scannet18":
            from .ap import CLASS_IDS
            keep &= np.isin(box_sem, CLASS_IDS)
        box_sem = box_sem[keep]
    fields = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in vars(found).items()}
    kept = Boxes(**dict(fields, min_points=min_points))
    os.makedirs(out_dir, exist_ok=True)
    arrays = kept.arrays()
    if box_sem is not None:
        arrays["sem"] = box_sem
    np.savez(npz, **arrays)
    if detector_files:
        np.save(os.path.join(out_dir, scene + NPY_SUFFIX), detector_rows(kept, box_sem))
    if ply:
        write_ply(os.path.join(out_dir, scene + ".boxes.ply"), *box_mesh(kept))
    return {"V": int(xyz.shape[0]), "instances": instances, "kept": int(kept.values.shape[0]), "ignored": int((labels < 0).sum())}


def boxes_scans(scans_dir: str, out_dir: str, scenes=None, workers: int = 4, device=None, **options):
    """Every scan directory under `scans_dir` (or the named ones) -> (report {scene: entry}, skipped scene names); writes
    <out_dir>/boxes_report.json.  Workers are threads, each with its own stream; `options` are boxes_scan's."""
    kind, a, min_points, classes = check_command(options.get("exp"), options.get("labels_from"), options.get("suffix"), options.get("key"),
                                                 options.get("kind", "yaw"), options.get("angles"), options.get("min_points"),
                                                 options.get("classes"), options.get("detector_files", False))
    dev = torch_device(device)
    if scenes is None and options.get("exp") is not None:
        base = os.path.join(options.get("root", "."), "results", options["exp"])
        scenes = [s for s in scans.scan_names(scans_dir) if os.path.isdir(os.path.join(base, s, options.get("stage", "epoch_last")))]
    head = {"kind": kind, "angles": a, "min_points": min_points, "classes": classes}
    head.update({k: options[k] for k in ("exp", "stage", "layer", "labels_from", "suffix", "key") if options.get(k) is not None})
    return scans.run_scans(scans_dir, scenes, workers, dev, out_dir, REPORT_NAME, head,
                           lambda path, stream: boxes_scan(path, out_dir, device=dev, stream=stream, **options))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.boxes", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of scan directories (<scene>/<scene>_vh_clean_2.ply)")
    ap.add_argument("--out", required=True, help="where <scene>.boxes.npz, boxes_report.json, _bbox.npy and .boxes.ply go")
    ap.add_argument("-n", "--exp_name", default=None, help="experiment route: name of the experiment")
    ap.add_argument("--stage", default=None, help="experiment route: the export directory's name (default epoch_last)")
    ap.add_argument("--layer", default=None, help="experiment route: final or layer_1 .. layer_4 (default final)")
    ap.add_argument("--root", default=None, help="experiment route: directory holding results/ (default: CWD)")
    ap.add_argument("--labels-from", default=None, metavar="DIR", help="any per-vertex int vector: DIR/<scene><suffix>")
    ap.add_argument("--suffix", default=None, help="--labels-from: the file name after the scene's, ending in .npy or .npz")
    ap.add_argument("--key", default=None, help="--labels-from: the array of an .npz")
    ap.add_argument("--kind", default="yaw", help="aabb, yaw or pca (default yaw)")
    ap.add_argument("--angles", type=int, default=None, metavar="A", help="kind yaw: steps of (pi/2)/A about z, 1..1024 (default 90)")
    ap.add_argument("--min-points", type=int, default=None, metavar="M",
                    help="drop boxes of fewer points (experiment route: default 100; --labels-from: no default)")
    ap.add_argument("--classes", default=None, help="experiment route: scannet18 (default) keeps the instances of the 18 benchmark classes; all")
    ap.add_argument("--detector-files", action="store_true", help="write <scene>_bbox.npy, float64 [K,7] = centre, full size, class id")
    ap.add_argument("--ply", action="store_true", help="write <scene>.boxes.ply, 8 vertices and 12 triangles per box")
    scans.add_batch_arguments(ap, "overwrite existing results")
    a = ap.parse_args(argv)
    scans.check_workers(ap, a.workers)
    if a.exp_name is None and (a.stage is not None or a.layer is not None or a.root is not None):
        ap.error("--stage, --layer and --root belong to the experiment route (-n EXP)")
    try:
        check_command(a.exp_name, a.labels_from, a.suffix, a.key, a.kind, a.angles, a.min_points, a.classes, a.detector_files)
    except ValueError as e:
        ap.error(str(e))
    route = dict(labels_from=a.labels_from, suffix=a.suffix, key=a.key)
    if a.exp_name is not None:
        route = dict(exp=a.exp_name, stage=a.stage or "epoch_last", layer=a.layer or "final", root=a.root or ".")
    report, skipped = boxes_scans(a.scans, a.out, scans.scene_list(a.scenes), a.workers, a.device, kind=a.kind, angles=a.angles,
                                  min_points=a.min_points, classes=a.classes, detector_files=a.detector_files, ply=a.ply, force=a.force, **route)
    scans.print_outcome(report, skipped, lambda scene, e: ("boxes", scene, e["V"], "vertices,", e["instances"], "instances,", e["kept"], "kept,",
                                                           e["ignored"], "ignored"), "(its .boxes.npz exists; --force overwrites)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
