"""THE RULE of sg_lift and sg_lift_vote (include/seggroup_hip.h) restated in NumPy, for the tests.  For every (view b, vertex
v), in this order: sg_render's projection (render_ref.project, imported: BEHIND, FAR, or X, Y in 1/256 pixel and c_2); the pixel px = X >> 8,
py = Y >> 8, OUTSIDE when it is off the image; d = depth[b,py,px], NODEPTH unless d is finite and > 0; OCCLUDED iff |c_2 - (double)d| > tol;
otherwise seen[v] += 1 and, with l = label[b,py,px], VISIBLE (seen, no vote) for l < 0 and LABELLED, counts[v,l] += 1, for 0 <= l < C.  A pair
with l >= C is refused: it adds nothing anywhere, and `bad` counts it (the library returns SG_EINVAL).  Every quantity is an integer or one
double operation rounded once, so the library's tables EQUAL these.

    accumulate(xyz, cams, labels, depth, tol, C, ortho, near, counts=None, seen=None) -> (counts int64 [V,C], seen int64 [V], stats, bad)
    vote(counts) -> (winner, votes, total, tied)          -- argmax takes the first maximum, so the lowest class
    lift(xyz, cams, labels, depth, tol, ...) -> Lift      -- what seggroup_amd.lift.lift returns: labels ranked to classes and mapped back

Also the tests' inputs: `soup_points` / `soup_images` (points of every kind and images with every kind of depth), `write_filtered_png` (a PNG
encoder with a chosen scanline filter per row, by the definitions of the PNG specification) and `scannet_tree` (what ScanNet's exporter leaves,
in small).
"""
import os
import struct
import zlib
from typing import NamedTuple

import numpy as np

import render_ref as R

STAT_NAMES = ("behind", "far", "outside", "nodepth", "occluded", "visible", "labelled")


class Lift(NamedTuple):
    label: np.ndarray
    votes: np.ndarray
    total: np.ndarray
    seen: np.ndarray
    tied: np.ndarray


def classify(xyz, cam, label, depth, tol, C, ortho, near):
    """one view -> (kind int8 [V]: the index into STAT_NAMES, 7 for a refused pair; the class voted for, int64 [V], -1 where none)"""
    H, W = label.shape
    X, Y, z, code = R.project(xyz, cam, ortho, near)
    px, py = X >> 8, Y >> 8
    kind = np.full(X.shape[0], -1, np.int8)
    kind[code == 1] = 0
    kind[code == 2] = 1
    inside = (code == 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    kind[(code == 0) & ~inside] = 2
    cx, cy = np.where(inside, px, 0), np.where(inside, py, 0)
    d = np.asarray(depth, np.float32)[cy, cx]
    with np.errstate(invalid="ignore"):
        has = inside & np.isfinite(d) & (d > 0)
        kind[inside & ~has] = 3
        hidden = has & (np.abs(z - d.astype(np.float64)) > float(tol))
    kind[hidden] = 4
    vis = has & ~hidden
    l = np.asarray(label, np.int64)[cy, cx]
    kind[vis & (l < 0)] = 5
    kind[vis & (l >= 0) & (l < C)] = 6
    kind[vis & (l >= C)] = 7
    assert (kind >= 0).all()
    return kind, np.where(kind == 6, l, -1)


def accumulate(xyz, cams, labels, depth, tol, C, ortho=False, near=0.05, counts=None, seen=None):
    """cams [B,16], labels and depth [B,H,W] -> (counts int64 [V,C], seen int64 [V], stats dict, the refused pairs)"""
    xyz = np.asarray(xyz, np.float32)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    V = xyz.shape[0]
    counts = np.zeros((V, C), np.int64) if counts is None else np.array(counts, np.int64)
    seen = np.zeros(V, np.int64) if seen is None else np.array(seen, np.int64)
    tally, bad = np.zeros(7, np.int64), 0
    for b, cam in enumerate(cams):
        kind, cls = classify(xyz, cam, labels[b], depth[b], tol, C, ortho, near)
        tally += np.bincount(kind[kind < 7], minlength=7)
        bad += int((kind == 7).sum())
        np.add.at(seen, np.flatnonzero((kind == 5) | (kind == 6)), 1)
        v = np.flatnonzero(kind == 6)
        np.add.at(counts, (v, cls[v]), 1)
    return counts, seen, dict(zip(STAT_NAMES, (int(t) for t in tally))), bad


def vote(counts):
    """counts [V,C] -> winner (-1 where the row is all zero), votes, total, tied, all int32"""
    counts = np.asarray(counts, np.int64)
    first = counts.argmax(1)
    votes = counts[np.arange(counts.shape[0]), first]
    winner = np.where(votes > 0, first, -1)
    tied = (votes > 0) & ((counts == votes[:, None]).sum(1) > 1)
    return winner.astype(np.int32), votes.astype(np.int32), counts.sum(1).astype(np.int32), tied.astype(np.int32)


def classes(labels):
    """labels -> (classes, values): the labels >= 0 ranked in ascending order, negatives to -1"""
    labels = np.asarray(labels)
    values = np.unique(labels[labels >= 0]).astype(np.int64)
    return np.where(labels >= 0, np.searchsorted(values, labels), -1).astype(np.int64), values


def lift(xyz, cams, labels, depth, tol, ortho=False, near=0.05, min_votes=1, min_share=0.0):
    """-> (Lift, counts, stats): seggroup_amd.lift.lift's result for explicit depth images"""
    cols, values = classes(labels)
    counts, seen, stats, bad = accumulate(xyz, cams, cols, depth, tol, max(values.shape[0], 1), ortho, near)
    assert bad == 0
    winner, votes, total, tied = vote(counts)
    keep = (winner >= 0) & (votes >= min_votes) & ~(votes < min_share * total)
    label = np.where(keep, np.concatenate([values, [-1]])[winner], -1).astype(np.int32)
    return Lift(label, votes, total, seen.astype(np.int32), tied), counts, stats


# ---- PNGs and a ScanNet-shaped tree, for the tests of the reader ------------------------------------------------------------------------------------
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def write_filtered_png(path, img, filters, lace=0, colour=None):
    """uint8 [H,W], uint16 [H,W] or uint8 [H,W,3] -> a PNG with the scanline filter filters[y % len] on row y, encoded by the definitions of
    the PNG specification, in two IDAT chunks behind a text chunk; `lace` and `colour` overwrite the header's fields (for the refusals)"""
    a = np.asarray(img)
    bits = 16 if a.dtype == np.uint16 else 8
    colour = (2 if a.ndim == 3 else 0) if colour is None else colour
    bpp = 3 if a.ndim == 3 else bits // 8
    raw = (a.astype(">u2").view(np.uint8) if bits == 16 else a).reshape(a.shape[0], -1).astype(np.int64)
    out = bytearray()
    prev = np.zeros(raw.shape[1], np.int64)
    for y, row in enumerate(raw):
        f = filters[y % len(filters)]
        left = np.concatenate([np.zeros(bpp, np.int64), row[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]])
        pred = {0: 0 * row, 1: left, 2: prev, 3: (left + prev) // 2, 4: np.array([_paeth(int(p), int(q), int(r)) for p, q, r in zip(left, prev, upleft)])}[f]
        out += bytes([f]) + ((row - pred) % 256).astype(np.uint8).tobytes()
        prev = row
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], bits, colour, 0, 0, lace))
    body = zlib.compress(bytes(out), 6)
    half = len(body) // 2
    data += _chunk(b"tEXt", b"Comment\0two IDAT chunks follow") + _chunk(b"IDAT", body[:half]) + _chunk(b"IDAT", body[half:]) + _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(data)


def scannet_tree(base, scene="scene0000_00", frames=("0", "1", "2", "10", "11"), lost=("2",), size=(8, 6), label_size=(16, 12), seed=0):
    """what ScanNet's exporter leaves, in small: <base>/<scene>/{pose,depth,label-filt,instance-filt}/<f>.* and intrinsic/intrinsic_depth.txt
    -> (the scene's directory, K, {frame: (pose, depth uint16, label-filt uint16, instance-filt uint8)}); the poses of `lost` hold -inf, as
    ScanNet writes lost tracking"""
    rng = np.random.RandomState(seed)
    d = os.path.join(str(base), scene)
    for sub in ("pose", "depth", "label-filt", "instance-filt", "intrinsic"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    K = np.array([[7.0, 0, 3.5, 0], [0, 7.0, 2.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    np.savetxt(os.path.join(d, "intrinsic", "intrinsic_depth.txt"), K)
    out = {}
    for f in frames:
        P = np.eye(4)
        P[:3, 3] = rng.uniform(-0.2, 0.2, 3)
        if f in lost:
            P[:] = -np.inf
        with open(os.path.join(d, "pose", f + ".txt"), "w") as fh:
            fh.write("\n".join(" ".join(repr(float(x)) for x in row) for row in P) + "\n")
        depth = rng.randint(0, 3000, (size[1], size[0])).astype(np.uint16)
        lab = rng.randint(0, 41, (label_size[1], label_size[0])).astype(np.uint16)
        ins = rng.randint(0, 9, (label_size[1], label_size[0])).astype(np.uint8)
        write_filtered_png(os.path.join(d, "depth", f + ".png"), depth, (0, 1, 2))
        write_filtered_png(os.path.join(d, "label-filt", f + ".png"), lab, (4, 3))
        write_filtered_png(os.path.join(d, "instance-filt", f + ".png"), ins, (0, 4, 1))
        out[f] = (P, depth, lab, ins)
    return d, K, out


def soup_points(n=3000, seed=0):
    """n random points in front of render_ref.soup_cameras, about a tenth of them with a NaN coordinate, behind the camera or nearer than
    SOUP_NEAR, or beyond the guard band (both projections) -> xyz float32 [n,3]"""
    rng = np.random.RandomState(seed)
    xyz = np.stack([rng.uniform(-2.2, 2.2, n), rng.uniform(-1.6, 1.6, n), rng.uniform(1.0, 3.0, n)], 1)
    what = rng.uniform(0.0, 1.0, n)
    xyz[what < 0.02, rng.randint(0, 3)] = np.nan
    near = (what >= 0.02) & (what < 0.06)
    xyz[near, 2] = rng.choice([-0.5, 0.0, 0.01, R.SOUP_NEAR], int(near.sum()))
    far = (what >= 0.06) & (what < 0.1)
    xyz[far, 0] = rng.choice([-3000.0, 3000.0], int(far.sum()))
    return xyz.astype(np.float32)


def soup_images(xyz, cams, size, C, ortho, near=R.SOUP_NEAR, seed=1):
    """random label images in -1..C-1 and depth images that agree with about half of the vertices that land on them (the others a random
    depth), with zeros, NaNs, +inf and negatives planted -> (labels int32 [B,H,W], depth float32 [B,H,W], tol)"""
    rng = np.random.RandomState(seed)
    W, H = size
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    labels = rng.randint(-1, C, (cams.shape[0], H, W)).astype(np.int32)
    depth = rng.uniform(1.0, 3.0, (cams.shape[0], H, W)).astype(np.float32)
    for b, cam in enumerate(cams):
        X, Y, z, code = R.project(xyz, cam, ortho, near)
        px, py = X >> 8, Y >> 8
        ok = np.flatnonzero((code == 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H))
        ok = ok[rng.uniform(0, 1, ok.shape[0]) < 0.5]
        depth[b, py[ok], px[ok]] = (z[ok] + rng.uniform(-0.1, 0.1, ok.shape[0])).astype(np.float32)
    bad = rng.uniform(0, 1, depth.shape)
    depth[bad < 0.03] = 0.0
    depth[(bad >= 0.03) & (bad < 0.06)] = np.nan
    depth[(bad >= 0.06) & (bad < 0.09)] = np.inf
    depth[(bad >= 0.09) & (bad < 0.1)] = -1.5
    return labels, depth, 0.06
