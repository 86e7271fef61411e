"""THE RULE of sg_render (include/seggroup_hip.h) restated in NumPy, for the tests: fixed-point screen coordinates, int64
edge functions, a uint64 key (float depth bits << 32 | primitive index) of which a pixel keeps the minimum.  Every quantity is an integer or
one double operation rounded once, so the library's images EQUAL these, bit for bit.

    render(xyz, faces, cams, size, ortho, near, point_size) -> Image(prim, depth, vert [B,H,W], hits [V], stats)

`render` loops over the primitives in index order and vectorises over each box's pixels.  With buckets=True the boxes of at most 16 x 16
pixels are taken many at a time (np.minimum.at): the same arithmetic per (primitive, pixel), for meshes of tens of thousands of faces;
tests/test_render_ref.py holds the two to each other.  `inside_exact` is a second statement of coverage, in exact rationals, and
`read_png` the minimal PNG reader of the tests.
"""
import struct
import zlib
from fractions import Fraction
from typing import NamedTuple

import numpy as np

GUARD = 16384.0
SMALL = 8                              # the build's small-primitive threshold: `large` counts the kept triangles whose clipped box exceeds it
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_NAMES = ("kept", "behind", "far", "degenerate", "large", "covered")


class Image(NamedTuple):
    prim: np.ndarray
    depth: np.ndarray
    vert: np.ndarray
    hits: np.ndarray
    stats: dict


def camera_row(T, fx, fy, cx, cy) -> np.ndarray:
    """-> the 16 doubles of one view: T (3 x 4, or the top of a 4 x 4) row-major, then fx fy cx cy"""
    return np.concatenate([np.asarray(T, np.float64)[:3, :4].reshape(12), [fx, fy, cx, cy]])


def project(xyz, cam, ortho, near):
    """one view -> X, Y int64 [V], z float64 [V], code int8 [V]: 0 in view, 1 behind, 2 far"""
    p = np.asarray(xyz, np.float32)[:, :3]
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    T = np.asarray(cam, np.float64)[:12].reshape(3, 4)
    fx, fy, cx, cy = (float(v) for v in np.asarray(cam, np.float64)[12:16])
    with np.errstate(all="ignore"):
        c = [((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)]
        ok = np.isfinite(p).all(1) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & (c[2] > near)
        zs = np.where(ok, c[2], 1.0)
        if ortho:
            u, v = fx * c[0] + cx, fy * c[1] + cy
        else:
            u, v = fx * (c[0] / zs) + cx, fy * (c[1] / zs) + cy
        near_enough = ok & (np.abs(u) <= GUARD) & (np.abs(v) <= GUARD)
        X = np.where(near_enough, np.floor(u * 256.0 + 0.5), 0.0).astype(np.int64)
        Y = np.where(near_enough, np.floor(v * 256.0 + 0.5), 0.0).astype(np.int64)
    code = np.where(~ok, 1, np.where(~near_enough, 2, 0)).astype(np.int8)
    return X, Y, np.where(code == 0, c[2], 0.0), code


def _edges(X, Y, cx, cy):
    """corner arrays X, Y [3][...] and centres cx, cy (broadcastable) -> w_0, w_1, w_2, A, all with A > 0 where A != 0"""
    w = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        w.append((X[k] - X[j]) * (cy - Y[j]) - (Y[k] - Y[j]) * (cx - X[j]))
    A = w[0] + w[1] + w[2]
    s = np.where(A < 0, -1, 1)
    return w[0] * s, w[1] * s, w[2] * s, A * s


def _keys(w0, w1, w2, A, z, ortho, prim):
    """-> uint64 keys (valid where every w_i >= 0 and A > 0); z [3][...] the corners' c_2"""
    q = z if ortho else [1.0 / z[0], 1.0 / z[1], 1.0 / z[2]]
    with np.errstate(all="ignore"):
        s = (w0.astype(np.float64) * q[0] + w1.astype(np.float64) * q[1]) + w2.astype(np.float64) * q[2]
        r = s / A.astype(np.float64)
        depth = (r if ortho else 1.0 / r).astype(np.float32)
    return (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(prim).astype(np.uint64)


def _box(X, Y, W, H):
    """corner arrays [3][n] -> the clipped box of pixel centres inside the corners' bounding box: x0, x1, y0, y1 (inclusive; empty iff x0 > x1 or y0 > y1)"""
    xmin, xmax = np.minimum(np.minimum(X[0], X[1]), X[2]), np.maximum(np.maximum(X[0], X[1]), X[2])
    ymin, ymax = np.minimum(np.minimum(Y[0], Y[1]), Y[2]), np.maximum(np.maximum(Y[0], Y[1]), Y[2])
    return (np.maximum((xmin + 127) >> 8, 0), np.minimum((xmax - 128) >> 8, W - 1), np.maximum((ymin + 127) >> 8, 0), np.minimum((ymax - 128) >> 8, H - 1))


def _raster_loop(keys, todo, Xc, Yc, zc, box, ortho):
    """the primitives `todo` in index order, each vectorised over its box"""
    x0, x1, y0, y1 = box
    for p in todo:
        cx = 256 * np.arange(x0[p], x1[p] + 1, dtype=np.int64)[None, :] + 128
        cy = 256 * np.arange(y0[p], y1[p] + 1, dtype=np.int64)[:, None] + 128
        w0, w1, w2, A = _edges([Xc[i][p] for i in range(3)], [Yc[i][p] for i in range(3)], cx, cy)
        inside = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
        if not inside.any():
            continue
        k = _keys(w0, w1, w2, A + 0 * w0, [zc[i][p] for i in range(3)], ortho, p)
        view = keys[y0[p]:y1[p] + 1, x0[p]:x1[p] + 1]
        view[inside] = np.minimum(view[inside], k[inside])


def _raster_buckets(keys, todo, Xc, Yc, zc, box, ortho, side, chunk):
    """the primitives `todo`, whose boxes are at most side x side, `chunk` at a time over a side x side grid of offsets"""
    x0, x1, y0, y1 = box
    W = keys.shape[1]
    flat = keys.reshape(-1)
    oy, ox = (o.reshape(1, -1) for o in np.meshgrid(np.arange(side, dtype=np.int64), np.arange(side, dtype=np.int64), indexing="ij"))
    for at in range(0, todo.shape[0], chunk):
        p = todo[at:at + chunk]
        px, py = x0[p][:, None] + ox, y0[p][:, None] + oy
        w0, w1, w2, A = _edges([Xc[i][p][:, None] for i in range(3)], [Yc[i][p][:, None] for i in range(3)], 256 * px + 128, 256 * py + 128)
        inside = (px <= x1[p][:, None]) & (py <= y1[p][:, None]) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
        k = _keys(w0, w1, w2, A + 0 * w0, [zc[i][p][:, None] + 0.0 * w0 for i in range(3)], ortho, p[:, None] + 0 * w0)
        np.minimum.at(flat, (py * W + px)[inside], k[inside])


def render_view(xyz, faces, cam, size, ortho, near, point_size=3, buckets=False):
    """one view -> (keys uint64 [H,W], counts [kept, behind, far, degenerate, large], projection)"""
    W, H = size
    X, Y, z, code = project(xyz, cam, ortho, near)
    keys = np.full((H, W), EMPTY, np.uint64)
    if faces is None:
        kept = np.flatnonzero(code == 0)
        half = point_size >> 1
        for p in kept:
            cx, cy = int(X[p]) >> 8, int(Y[p]) >> 8
            a0, a1, b0, b1 = max(cx - half, 0), min(cx + half, W - 1), max(cy - half, 0), min(cy + half, H - 1)
            if a0 <= a1 and b0 <= b1:
                k = (np.uint64(np.float32(z[p]).view(np.uint32)) << np.uint64(32)) | np.uint64(p)
                keys[b0:b1 + 1, a0:a1 + 1] = np.minimum(keys[b0:b1 + 1, a0:a1 + 1], k)
        return keys, [int(kept.size), int((code == 1).sum()), int((code == 2).sum()), 0, 0], (X, Y, z)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fc = code[f]
    behind = (fc == 1).any(1)
    far = ~behind & (fc == 2).any(1)
    Xc, Yc, zc = ([a[f[:, i]] for i in range(3)] for a in (X, Y, z))
    A = (Xc[1] - Xc[0]) * (Yc[2] - Yc[0]) - (Yc[1] - Yc[0]) * (Xc[2] - Xc[0])
    degenerate = ~behind & ~far & (A == 0)
    kept = ~behind & ~far & (A != 0)
    box = _box(Xc, Yc, W, H)
    bw, bh = box[1] - box[0] + 1, box[3] - box[2] + 1
    drawn = kept & (bw > 0) & (bh > 0)
    large = drawn & ((bw > SMALL) | (bh > SMALL))
    if buckets:
        side = np.maximum(bw, bh)
        _raster_buckets(keys, np.flatnonzero(drawn & (side <= 4)), Xc, Yc, zc, box, ortho, 4, 16384)
        _raster_buckets(keys, np.flatnonzero(drawn & (side > 4) & (side <= 16)), Xc, Yc, zc, box, ortho, 16, 2048)
        _raster_loop(keys, np.flatnonzero(drawn & (side > 16)), Xc, Yc, zc, box, ortho)
    else:
        _raster_loop(keys, np.flatnonzero(drawn), Xc, Yc, zc, box, ortho)
    return keys, [int(kept.sum()), int(behind.sum()), int(far.sum()), int(degenerate.sum()), int(large.sum())], (X, Y, z)


def resolve(keys, faces, proj):
    """keys [H,W] -> prim int32, depth float32, vert int32"""
    H, W = keys.shape
    covered = keys != EMPTY
    prim = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(covered, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).astype(np.float32)
    if faces is None:
        return prim, depth, prim.copy()
    vert = np.full((H, W), -1, np.int32)
    py, px = np.nonzero(covered)
    if py.size:
        X, Y, _ = proj
        f = np.asarray(faces, np.int64).reshape(-1, 3)[prim[py, px]]
        w0, w1, w2, _ = _edges([X[f[:, i]] for i in range(3)], [Y[f[:, i]] for i in range(3)], 256 * px.astype(np.int64) + 128, 256 * py.astype(np.int64) + 128)
        corner = np.where(w1 > w0, np.where(w2 > w1, 2, 1), np.where(w2 > w0, 2, 0))      # the largest, a tie to the lower corner
        vert[py, px] = f[np.arange(f.shape[0]), corner]
    return prim, depth, vert


def render(xyz, faces, cams, size, ortho=False, near=0.05, point_size=3, buckets=False) -> Image:
    """cams [B,16] -> Image over all B views"""
    xyz = np.asarray(xyz, np.float32)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    if faces is not None and np.asarray(faces).shape[0] == 0:
        faces = None
    out, counts = [], np.zeros(5, np.int64)
    hits = np.zeros(xyz.shape[0], np.int64)
    for cam in cams:
        keys, c, proj = render_view(xyz, faces, cam, size, ortho, near, point_size, buckets)
        counts += np.asarray(c, np.int64)
        out.append(resolve(keys, faces, proj))
        v = out[-1][2]
        hits += np.bincount(v[v >= 0], minlength=xyz.shape[0])
    prim, depth, vert = (np.stack([o[i] for o in out]) for i in range(3))
    stats = dict(zip(STAT_NAMES, [int(x) for x in counts] + [int((prim >= 0).sum())]))
    return Image(prim, depth, vert, hits.astype(np.int32), stats)


# ---- a second statement of coverage: exact rationals -----------------------------------------------------------------------------------------
def inside_exact(corners, px, py) -> bool:
    """corners: three (X, Y) in fixed point (Python integers).  The centre C of pixel (px, py) as C = P0 + a (P1 - P0) + b (P2 - P0) by
    Cramer's rule in exact rationals: inside the closed triangle iff a >= 0, b >= 0 and a + b <= 1.  A triangle of no area holds nothing."""
    (x0, y0), (x1, y1), (x2, y2) = ((int(x), int(y)) for x, y in corners)
    cx, cy = 256 * int(px) + 128, 256 * int(py) + 128
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if det == 0:
        return False
    a = Fraction((cx - x0) * (y2 - y0) - (x2 - x0) * (cy - y0), det)
    b = Fraction((x1 - x0) * (cy - y0) - (cx - x0) * (y1 - y0), det)
    return a >= 0 and b >= 0 and a + b <= 1


def covered_exact(corners, W, H):
    """-> the set of pixels (px, py) of a W x H image whose centres `inside_exact` holds"""
    return {(px, py) for py in range(H) for px in range(W) if inside_exact(corners, px, py)}


# ---- the camera of the hand cases ---------------------------------------------------------------------------------------------------------
def pixel_camera():
    """orthographic, world x = u, world y = v in pixels, depth = world z: X = 256 x exactly for x on the 1/256 grid"""
    return camera_row(np.eye(4), 1.0, 1.0, 0.0, 0.0)


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------------
SOUP_NEAR = 0.05


def soup_cameras(size=(67, 45)):
    """-> (perspective row, orthographic row) that put the soup's middle in the middle of a `size` image"""
    W, H = size
    return camera_row(np.eye(4), 40.0, 40.0, 0.5 * W, 0.5 * H), camera_row(np.eye(4), 20.0, 20.0, 0.5 * W, 0.5 * H)


def soup(n=1500, seed=0):
    """n random triangles in front of soup_cameras: most sub-pixel or a few pixels wide (many hold no pixel centre), some tens of pixels,
    a few across the whole image (the queue path), many partly off-screen; about 3 % with a vertex behind the camera or nearer than
    SOUP_NEAR, 2 % with a vertex beyond the guard band, 1 % naming one vertex twice (degenerate).  -> xyz float32 [3n,3], faces int32 [n,3]"""
    rng = np.random.RandomState(seed)
    centre = np.stack([rng.uniform(-2.2, 2.2, n), rng.uniform(-1.6, 1.6, n), rng.uniform(1.0, 3.0, n)], 1)
    kind = rng.choice(4, n, p=[0.45, 0.35, 0.18, 0.02])
    extent = np.array([0.01, 0.08, 0.6, 6.0])[kind]
    xyz = centre[:, None, :] + rng.uniform(-1.0, 1.0, (n, 3, 3)) * extent[:, None, None] * np.array([1.0, 1.0, 0.3])
    xyz[:, :, 2] = np.maximum(xyz[:, :, 2], 0.2)
    what = rng.uniform(0.0, 1.0, n)
    corner = rng.randint(0, 3, n)
    rows = np.arange(n)
    xyz[rows[what < 0.03], corner[what < 0.03], 2] = rng.choice([-0.5, 0.0, 0.01, SOUP_NEAR], int((what < 0.03).sum()))
    far = (what >= 0.03) & (what < 0.05)
    xyz[rows[far], corner[far], 0] = rng.choice([-3000.0, 3000.0], int(far.sum()))
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    twice = (what >= 0.05) & (what < 0.06)
    faces[twice, 2] = faces[twice, 0]
    return xyz.reshape(-1, 3).astype(np.float32), faces


def pixel_lattice(nx=11, ny=11, step=3, seed=4):
    """2 (nx-1)(ny-1) triangles whose corners are pixel CENTRES (k + 0.5) under pixel_camera, every cell cut along the same diagonal: an inner
    vertex is shared by six triangles, and many pixel centres lie exactly on edges and on corners.  Depths on a coarse grid, so float
    depths tie.  -> xyz float32, faces int32"""
    rng = np.random.RandomState(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    xyz = np.stack([i * step + 0.5, j * step + 0.5, rng.randint(4, 9, (nx, ny)) / 4.0], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)]).astype(np.int32)
    return xyz.astype(np.float32), faces


def folded_sheet(nx=200, ny=100, seed=3):
    """about nx * ny vertices: a sheet over [0, 4] x [0, 2] at z = 1 whose last third is folded back UNDER it (z = 0.6), the crease along
    x = 4, jittered.  -> xyz float32 [V,3], faces int32 [F,3], hidden bool [V]: the vertices of the folded part well inside the sheet's
    shadow, which no view from above sees."""
    rng = np.random.RandomState(seed)
    s, t = np.meshgrid(np.linspace(0.0, 6.0, nx), np.linspace(0.0, 2.0, ny), indexing="ij")
    x = np.where(s <= 4.0, s, 8.0 - s)
    z = np.where(s <= 4.0, 1.0, 1.0 - 0.4 * np.minimum((s - 4.0) / 0.2, 1.0))
    xyz = np.stack([x, t, z], -1).reshape(-1, 3) + rng.uniform(-0.002, 0.002, (nx * ny, 3))
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)]).astype(np.int32)
    hidden = ((s > 4.5) & (s < 5.8) & (t > 0.1) & (t < 1.9)).reshape(-1)
    return xyz.astype(np.float32), faces, hidden


# ---- PNG --------------------------------------------------------------------------------------------------------------------------------------
def read_png(path) -> np.ndarray:
    """8-bit RGB -> uint8 [H,W,3]; 16-bit grey -> uint16 [H,W].  Filter 0 rows only, no interlace: what render.write_png writes."""
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    at, idat, head = 8, b"", None
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        body = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == (zlib.crc32(kind + body) & 0xFFFFFFFF), "a chunk's CRC"
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    W, H, bits, colour, comp, filt, lace = head
    assert (comp, filt, lace) == (0, 0, 0) and (bits, colour) in ((8, 2), (16, 0))
    row = W * (3 if colour == 2 else 2)
    data = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, row + 1)
    assert (data[:, 0] == 0).all(), "a row with another filter than 0"
    body = np.ascontiguousarray(data[:, 1:])
    return body.reshape(H, W, 3) if colour == 2 else body.view(">u2").astype(np.uint16).reshape(H, W)
