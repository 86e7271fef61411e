"""The grid-indexed kNN's search rule restated in NumPy float32, on top of pcseg_ref.pair_scores: the same cell assignment,
the same delta, the same lower bound Lb, rings with a limit and a fallback.  It exists to prove the rule without a device
(tests/test_knn_grid_ref.py) and is the statement tests/test_gpu_knn_grid.py holds the kernel's table to beside pcseg_ref.knn_table.

Every operation of the settled test is one NumPy call on float32 operands, in the order the kernel writes it.  Nothing here calls the
library.
"""
import numpy as np

import pcseg_ref

F32 = np.float32
CELL_LIMIT = F32(2097152.0)                     # 2^21 cells per axis
MIN_CELLS = 1 << 22                             # the dense table holds max(2^22, 4 N) cells
RING_LIMIT = 8                                  # the library's default
SHRINK = F32(0.998046875)                       # 1 - 2^-9
DELTA_FLOOR = F32(2.0 ** -100)
SHIFTS = ((100.0, -50.0, 5.0), (300.0, 200.0, 10.0), (1000.0, 1000.0, 1000.0))
MARGIN_SHIFT = (300.0, 200.0, 10.0)             # the shift whose room needs delta: an unguarded search gets rows wrong there
OUTLIERS = np.array([[9.0, 9.0, 9.0], [-7.0, 3.0, 1.0]], F32)


class CellRange(ValueError):
    """a forced cell the grid path refuses: an axis of 2^21 cells or more, or more cells than the dense table holds"""


def shifted(xyz, shift):
    return np.ascontiguousarray((np.asarray(xyz, F32) + np.asarray(shift, F32)[None, :]).astype(F32))


def with_outliers(xyz):
    return np.ascontiguousarray(np.concatenate([np.asarray(xyz, F32), OUTLIERS], 0))


def m2_of(x):
    return pcseg_ref._sq(x).max()


def delta_of(x):
    """2^-19 * max |p|^2 (32 u M2, u = 2^-24; the roundings of pair_score add up to about 19 u M2), not below 2^-100"""
    return max(F32(2.0 ** -19) * m2_of(x), DELTA_FLOOR)


def score_error(x, chunk=512):
    """max |score + d2| over all pairs, d2 in float64"""
    worst = 0.0
    x64 = x.astype(np.float64)
    for i in range(0, x.shape[0], chunk):
        s = pcseg_ref.pair_scores(x[i:i + chunk], x).astype(np.float64)
        d = x64[i:i + chunk, None, :] - x64[None, :, :]
        worst = max(worst, float(np.abs(s + (d * d).sum(2)).max()))
    return worst


class Grid:
    """the cells of a cloud at edge h: 8g's formula floor((p - lo) / h) per axis, keys (cz * ny + cy) * nx + cx, the points sorted by key
    (stable: ascending index inside a cell) and start[c] = the number of keys below c"""

    def __init__(self, x, h):
        self.x = x = np.ascontiguousarray(np.asarray(x, F32)[:, :3])
        self.h = h = F32(h)
        if not np.isfinite(x).all() or not (np.isfinite(h) and h > 0):
            raise ValueError("grid: a finite cloud and a finite cell edge > 0")
        lo, hi = x.min(0), x.max(0)
        self.ext = ext = (hi - lo).astype(F32)
        with np.errstate(all="ignore"):
            if not ((ext / h) < CELL_LIMIT).all():
                raise CellRange("cell too small for the cloud's extent")
            self.nc = nc = np.floor(ext / h).astype(np.int64) + 1
            c = np.floor((x - lo) / h).astype(np.int64)
        if int(nc.prod()) > max(MIN_CELLS, 4 * x.shape[0]):
            raise CellRange("more cells than the dense table holds")
        self.cell = c
        self.key = key = (c[:, 2] * nc[1] + c[:, 1]) * nc[0] + c[:, 0]
        self.order = np.argsort(key, kind="stable")
        self.start = np.searchsorted(key[self.order], np.arange(int(nc.prod()) + 1))
        self.slack = F32(np.ldexp(ext.max(), -21))               # 8 u E
        self.delta = delta_of(x)

    def occupied(self):
        return int(np.unique(self.key).shape[0])

    def largest_cell(self):
        return int(np.diff(self.start).max())

    def ranges(self, g, r):
        """the sorted-point ranges that ring r adds round cell g = (gx, gy, gz): ring 1 is the 3 x 3 x 3 block, ring r > 1 the shell at
        Chebyshev distance r (whole row pieces where |dy| or |dz| is r, the two end cells elsewhere)"""
        nx, ny, nz = (int(v) for v in self.nc)
        gx, gy, gz = (int(v) for v in g)
        d = np.arange(-r, r + 1)
        dz, dy = np.meshgrid(d, d, indexing="ij")
        dz, dy = dz.reshape(-1), dy.reshape(-1)
        z, y = gz + dz, gy + dy
        ok = (z >= 0) & (z < nz) & (y >= 0) & (y < ny)
        z, y, dz, dy = z[ok], y[ok], dz[ok], dy[ok]
        row = (z * ny + y) * nx
        inner = (np.maximum(np.abs(dy), np.abs(dz)) < r) & (r > 1)
        x0, x1 = max(gx - r, 0), min(gx + r, nx - 1)
        a = [self.start[row[~inner] + x0]]
        b = [self.start[row[~inner] + x1 + 1]]
        if gx - r >= 0:
            a.append(self.start[row[inner] + gx - r]); b.append(self.start[row[inner] + gx - r + 1])
        if gx + r < nx:
            a.append(self.start[row[inner] + gx + r]); b.append(self.start[row[inner] + gx + r + 1])
        a, b = np.concatenate(a), np.concatenate(b)
        keep = b > a
        return a[keep], b[keep]

    def covers(self, g, r):
        return all(int(g[a]) - r <= 0 and int(g[a]) + r >= int(self.nc[a]) - 1 for a in range(3))


def settled(r, h, slack, delta, s_kth):
    """the kernel's test after ring r, op by op in float32: every unseen point is at least gap = r h - slack away along one axis"""
    with np.errstate(all="ignore"):
        gap = F32(r) * F32(h) - F32(slack)
        lhs = (gap * gap) * SHRINK
        rhs = F32(delta) - F32(s_kth)
    return bool(gap > 0 and lhs > rhs)


def _best(sc, idx, kk):
    """the kk best of (score, original index): descending score, the lower index first among equal scores"""
    order = np.lexsort((idx, -sc))[:kk]
    return sc[order], idx[order]


def knn_rows(grid, rows, k=10, ring_limit=RING_LIMIT, delta=None):
    """The search of the rows `rows` -> (table int32 [len(rows), k+1], rings int [len(rows)]: the ring that settled the row, 0 where the
    whole cloud finished it).  `delta`: the margin of the settled test (default: the grid's; 0 shows what the margin is for)."""
    x, kk = grid.x, k + 1
    if x.shape[0] <= k:
        raise ValueError("%d points for k = %d" % (x.shape[0], k))
    delta = grid.delta if delta is None else F32(delta)
    out = np.empty((len(rows), kk), np.int32)
    rings = np.zeros(len(rows), np.int64)
    for n, i in enumerate(rows):
        q = x[i:i + 1]
        g = grid.cell[i]
        sc, idx = np.empty(0, F32), np.empty(0, np.int64)
        done = False
        for r in range(1, ring_limit + 1):
            a, b = grid.ranges(g, r)
            if a.shape[0]:
                length = b - a
                pos = np.repeat(a - np.concatenate([[0], np.cumsum(length)[:-1]]), length) + np.arange(int(length.sum()))
                cand = grid.order[pos]
                sc = np.concatenate([sc, pcseg_ref.pair_scores(q, x[cand])[0]])
                idx = np.concatenate([idx, cand])
                sc, idx = _best(sc, idx, kk)
            if grid.covers(g, r) or (sc.shape[0] == kk and settled(r, grid.h, grid.slack, delta, sc[kk - 1])):
                out[n], rings[n], done = idx, r, True
                break
        if not done:
            out[n] = pcseg_ref._top(pcseg_ref.pair_scores(q, x), kk)[0]
    return out, rings


def knn_table_grid(xyz, k=10, cell=0.1, ring_limit=RING_LIMIT, rows=None, delta=None):
    """-> (table of the rows (all when None), rings, the Grid)"""
    grid = Grid(xyz, cell)
    rows = np.arange(grid.x.shape[0]) if rows is None else np.asarray(rows)
    table, rings = knn_rows(grid, rows, k, ring_limit, delta)
    return table, rings, grid


def brute_rows(xyz, rows, k=10):
    """pcseg_ref.knn_table's rows `rows`"""
    x = np.ascontiguousarray(np.asarray(xyz, F32)[:, :3])
    rows = np.asarray(rows)
    out = np.empty((rows.shape[0], k + 1), np.int32)
    for i in range(0, rows.shape[0], 512):
        out[i:i + 512] = pcseg_ref._top(pcseg_ref.pair_scores(x[rows[i:i + 512]], x), k + 1)
    return out
