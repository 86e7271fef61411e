"""The grid-indexed nearest point between two clouds restated in NumPy float32, on top of pcseg_ref.pair_scores and
knn_grid_ref: the box, the largest extent and M2 over the UNION of queries and candidates, 8g's cell formula for both, the index over
the candidates, rings with a limit, 8h's guarded test with a list of one entry, and the queue.  `brute` is the plain statement: the
first argmax of every row of pair_scores(x, y).

The result of the rule does not depend on the order in which a block's cells are visited, so the statement takes a block as what it is --
the candidates whose cell is within Chebyshev distance r of the query's -- and evaluates ring after ring on whole arrays.  Every
operation of the settled test is one NumPy call on float32 operands, in the order the kernel writes it.  Nothing here calls the library.
"""
import concurrent.futures

import numpy as np

import knn_grid_ref as G
import pcseg_ref

F32 = np.float32
RING_LIMIT = G.RING_LIMIT


def _xyz(a):
    return np.ascontiguousarray(np.asarray(a, F32)[:, :3])


def brute(x, y, chunk=512, threads=4):
    """-> int64 [U]: per query the FIRST argmax of its row of pair_scores(x, y) -- the best score, the lowest candidate among equals"""
    x, y = _xyz(x), _xyz(y)
    out = np.empty(x.shape[0], np.int64)

    def one(i):
        out[i:i + chunk] = pcseg_ref.pair_scores(x[i:i + chunk], y).argmax(1)
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(0, x.shape[0], chunk)))
    return out


def d2_of(x, y, idx):
    """(dx*dx + dy*dy) + dz*dz of d = x[u] - y[idx[u]], every operation rounded once"""
    d = _xyz(x) - _xyz(y)[np.asarray(idx)]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def delta_of(x, y):
    """2^-19 * max |p|^2 over BOTH clouds, not below 2^-100"""
    return max(G.delta_of(_xyz(x)), G.delta_of(_xyz(y)))


def score_error(x, y, chunk=512):
    """max |score + d2| over all pairs (query, candidate), d2 in float64"""
    x, y = _xyz(x), _xyz(y)
    worst, y64 = 0.0, y.astype(np.float64)
    for i in range(0, x.shape[0], chunk):
        s = pcseg_ref.pair_scores(x[i:i + chunk], y).astype(np.float64)
        d = x[i:i + chunk].astype(np.float64)[:, None, :] - y64[None, :, :]
        worst = max(worst, float(np.abs(s + (d * d).sum(2)).max()))
    return worst


class Grid(G.Grid):
    """the cells of the candidates y at edge h over the box of the UNION of x and y: lo, the extents, the slack (8 u E) and delta are the
    union's, the sorted order and start[] the candidates'; qcell holds the queries' cells on the same formula"""

    def __init__(self, x, y, h):
        self.q = x = _xyz(x)
        self.x = y = _xyz(y)                                    # G.Grid's name for the indexed cloud
        self.h = h = F32(h)
        if not (np.isfinite(x).all() and np.isfinite(y).all()) or not (np.isfinite(h) and h > 0):
            raise ValueError("grid: finite clouds and a finite cell edge > 0")
        if y.shape[0] < 1:
            raise ValueError("grid: at least one candidate")
        both = np.concatenate([x, y], 0)
        lo, hi = both.min(0), both.max(0)
        self.ext = ext = (hi - lo).astype(F32)
        with np.errstate(all="ignore"):
            if not ((ext / h) < G.CELL_LIMIT).all():
                raise G.CellRange("cell too small for the clouds' extent")
            self.nc = nc = np.floor(ext / h).astype(np.int64) + 1
            c = np.floor((y - lo) / h).astype(np.int64)
            self.qcell = np.floor((x - lo) / h).astype(np.int64)
        if int(nc.prod()) > max(G.MIN_CELLS, 4 * y.shape[0]):
            raise G.CellRange("more cells than the dense table holds")
        self.cell = c
        self.key = key = (c[:, 2] * nc[1] + c[:, 1]) * nc[0] + c[:, 0]
        self.order = np.argsort(key, kind="stable")
        self.start = np.searchsorted(key[self.order], np.arange(int(nc.prod()) + 1))
        self.slack = F32(np.ldexp(ext.max(), -21))
        self.delta = delta_of(x, y)


def settled(r, h, slack, delta, s_best):
    """8h's test after ring r for an array of best scores, op by op in float32 (G.settled for one score)"""
    with np.errstate(all="ignore"):
        gap = F32(r) * F32(h) - F32(slack)
        lhs = (gap * gap) * G.SHRINK
        rhs = F32(delta) - np.asarray(s_best, F32)
    return (gap > 0) & (lhs > rhs)


def nearest_grid(x, y, cell, ring_limit=RING_LIMIT, rows=None, delta=None, chunk=256, threads=4):
    """The search of the queries `rows` of x (all when None) -> (idx int64, rings int64: the ring that settled the query, 0 where the
    queue -- every candidate -- finished it, the Grid; grid.whole holds brute()'s answer for the same rows, which the pass has at
    hand).  `delta`: the margin of the settled test (default: the union's; 0 shows what the margin is for)."""
    grid = Grid(x, y, cell)
    rows = np.arange(grid.q.shape[0]) if rows is None else np.asarray(rows)
    delta = grid.delta if delta is None else F32(delta)
    idx = np.empty(rows.shape[0], np.int64)
    rings = np.zeros(rows.shape[0], np.int64)
    grid.whole = whole = np.empty(rows.shape[0], np.int64)
    nc = grid.nc
    qc32, cc32 = grid.qcell.astype(np.int32), grid.cell.astype(np.int32)

    def one(i):
        sel = rows[i:i + chunk]
        qc = grid.qcell[sel]
        s = pcseg_ref.pair_scores(grid.q[sel], grid.x)
        cheb = np.zeros(s.shape, np.int32)                      # Chebyshev distance of the candidates' cells from the query's
        for a in range(3):
            np.maximum(cheb, np.abs(qc32[sel, a][:, None] - cc32[None, :, a]), out=cheb)
        out = s.argmax(1)                                       # the queue: every candidate, the first of equal scores
        whole[i:i + chunk] = out
        ring = np.zeros(sel.shape[0], np.int64)
        pending = np.arange(sel.shape[0])
        for r in range(1, ring_limit + 1):
            if not pending.shape[0]:
                break
            seen = np.where(cheb[pending] <= r, s[pending], F32(-np.inf))
            best, arg = seen.max(1), seen.argmax(1)             # the first of equal scores: the lowest original index
            covers = ((qc[pending] - r <= 0) & (qc[pending] + r >= nc[None, :] - 1)).all(1)
            ok = covers | ((best > F32(-np.inf)) & settled(r, grid.h, grid.slack, delta, best))
            out[pending[ok]], ring[pending[ok]] = arg[ok], r
            pending = pending[~ok]
        idx[i:i + chunk], rings[i:i + chunk] = out, ring
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(0, rows.shape[0], chunk)))
    return idx, rings, grid


def stats_of(grid, rings):
    """what sg_nearest_point_grid_stats reports of a forced cell"""
    return dict(cells=tuple(int(v) for v in grid.nc), occupied=grid.occupied(), largest_cell=grid.largest_cell(),
                max_ring=int(rings.max()) if rings.size else 0, fallback=int((rings == 0).sum()))


# ---- the pairs (queries, candidates) of tests/test_nearest_grid_ref.py and tests/test_gpu_nearest_grid.py -----------------------------
_pairs = {}


def case_pairs():
    """name -> (queries f32 [U,3], candidates f32 [N,3])"""
    if not _pairs:
        c = {k: v[0] for k, v in pcseg_ref.case_clouds(include_large=True).items()}
        room, big = c["room_j5e-4"], c["room_20k"]
        _pairs["plain"] = (room, np.ascontiguousarray(room[::2]))
        _pairs["lattice"] = (c["room_j0"], np.ascontiguousarray(c["room_j0"][::2]))
        _pairs["dup"] = (c["room_dup"], c["room_dup"])
        _pairs["all_equal"] = (room, c["all_equal"])
        mid = F32(0.5) * (big[:, 0].min() + big[:, 0].max())
        _pairs["half_room"] = (big, np.ascontiguousarray(big[big[:, 0] < mid]))
        _pairs["outliers"] = (G.with_outliers(room), room)
        sh = G.shifted(room, G.MARGIN_SHIFT)
        _pairs["shifted"] = (sh, np.ascontiguousarray(sh[::2]))
    return _pairs


# two forced cells per pair: a small one (several rings) and one of many points per cell
CELLS = {"plain": (0.04, 0.3), "lattice": (0.04, 0.3), "dup": (0.04, 0.3), "all_equal": (0.04, 0.3), "half_room": (0.02, 0.2),
         "outliers": (0.1, 0.5), "shifted": (0.05, 0.3)}
