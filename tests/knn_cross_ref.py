"""The exact k nearest candidates of every query between two clouds and the vote over them restated in NumPy float32, on
top of nearest_grid_ref (the union box, 8g's cells, the index over the candidates, 8h's guarded test) and pcseg_ref.pair_scores.

    brute(x, y, k)                  the plain statement: the first k columns of a STABLE descending sort of every row of pair_scores(x, y)
    knn_cross_grid(x, y, k, cell)   the ring walk with a list of k entries: a list that is not full is unsettled, a full one settles by
                                    8h's test on its LAST score, queries unsettled at the ring limit take the queue (= brute's row)
    vote(knn, labels)               c(t) = the entries of the row that carry entry t's label; the first t with the largest c wins

As in nearest_grid_ref a block is taken as what it is -- the candidates whose cell is within Chebyshev distance r of the query's --, so
the k best of a block are the first k of the row's stable order that lie in it.  Nothing here calls the library.
"""
import concurrent.futures

import numpy as np

import knn_grid_ref as G
import nearest_grid_ref as NG
import pcseg_ref

F32 = np.float32
KS = (5, 10, 20)
RING_LIMIT = NG.RING_LIMIT
BLOCK = F32(0.25)                                   # the edge of the label blocks of labels_of
NOISE = 0.15                                        # the share of candidates relabelled at random


def _order(x, y):
    """per row of pair_scores(x, y) its columns in descending score, the lower column first among equal scores -> (order, scores)"""
    s = pcseg_ref.pair_scores(x, y)
    return np.argsort(-s, axis=1, kind="stable"), s


def brute(x, y, k, chunk=256, threads=4):
    """-> int32 [U, k]"""
    x, y = NG._xyz(x), NG._xyz(y)
    if y.shape[0] < k:
        raise ValueError("%d candidates for k = %d" % (y.shape[0], k))
    out = np.empty((x.shape[0], k), np.int32)

    def one(i):
        out[i:i + chunk] = _order(x[i:i + chunk], y)[0][:, :k]
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(0, x.shape[0], chunk)))
    return out


def d2_of(x, y, knn):
    """[U, k]: (dx*dx + dy*dy) + dz*dz of d = x[u] - y[knn[u][t]], every operation rounded once"""
    d = NG._xyz(x)[:, None, :] - NG._xyz(y)[np.asarray(knn)]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_cross_grid(x, y, k, cell, ring_limit=RING_LIMIT, rows=None, delta=None, chunk=256, threads=4):
    """The search of the queries `rows` of x (all when None) -> (knn int32 [len(rows), k], rings int64: the ring that settled the query, 0
    where the queue finished it, the Grid; grid.whole holds brute()'s rows, which the pass has at hand)."""
    grid = NG.Grid(x, y, cell)
    n = grid.x.shape[0]
    if n < k:
        raise ValueError("%d candidates for k = %d" % (n, k))
    rows = np.arange(grid.q.shape[0]) if rows is None else np.asarray(rows)
    delta = grid.delta if delta is None else F32(delta)
    knn = np.empty((rows.shape[0], k), np.int32)
    rings = np.zeros(rows.shape[0], np.int64)
    grid.whole = whole = np.empty((rows.shape[0], k), np.int32)
    nc = grid.nc
    qc32, cc32 = grid.qcell.astype(np.int32), grid.cell.astype(np.int32)

    def one(i):
        sel = rows[i:i + chunk]
        qc = grid.qcell[sel]
        order, s = _order(grid.q[sel], grid.x)
        s_sorted = np.take_along_axis(s, order, 1)
        cheb = np.zeros(s.shape, np.int32)                      # Chebyshev distance of the candidates' cells from the query's
        for a in range(3):
            np.maximum(cheb, np.abs(qc32[sel, a][:, None] - cc32[None, :, a]), out=cheb)
        cheb = np.take_along_axis(cheb, order, 1)               # in the row's stable order
        out = order[:, :k].astype(np.int32)                     # the queue: every candidate
        whole[i:i + chunk] = out
        ring = np.zeros(sel.shape[0], np.int64)
        pending = np.arange(sel.shape[0])
        for r in range(1, ring_limit + 1):
            if not pending.shape[0]:
                break
            seen = cheb[pending] <= r
            cnt = np.cumsum(seen, 1, dtype=np.int32)
            full = cnt[:, -1] >= k
            kth = (cnt >= k).argmax(1)                          # where the block's k-th best stands in the row's order (full lists)
            s_last = s_sorted[pending, kth]
            covers = ((qc[pending] - r <= 0) & (qc[pending] + r >= nc[None, :] - 1)).all(1)
            ok = covers | (full & NG.settled(r, grid.h, grid.slack, delta, s_last))
            if ok.any():
                take = seen[ok] & (cnt[ok] <= k)
                out[pending[ok]] = order[pending[ok]][take].reshape(-1, k)
                ring[pending[ok]] = r
            pending = pending[~ok]
        knn[i:i + chunk], rings[i:i + chunk] = out, ring
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(0, rows.shape[0], chunk)))
    return knn, rings, grid


def vote(knn, labels):
    """-> (winner int32 [U], rep int32 [U], count int32 [U], tied int32 [U]) of the rows of knn [U, k] over labels [N]"""
    knn, labels = np.asarray(knn), np.asarray(labels, np.int32)
    if knn.size and (knn.min() < 0 or knn.max() >= labels.shape[0]):
        raise ValueError("vote: a neighbour outside 0..%d" % (labels.shape[0] - 1))
    lab = labels[knn]
    c = (lab[:, :, None] == lab[:, None, :]).sum(2)
    t = c.argmax(1)                                             # the FIRST of the largest counts
    u = np.arange(knn.shape[0])
    winner, count = lab[u, t], c[u, t]
    tied = ((c == count[:, None]) & (lab != winner[:, None])).any(1)
    return winner.astype(np.int32), knn[u, t].astype(np.int32), count.astype(np.int32), tied.astype(np.int32)


def labels_of(y, seed=7):
    """Source labels of the vote checks: the candidates' 0.25-unit blocks (from the cloud's lower corner) numbered (bz * 64 + by) * 64 + bx,
    then 15 % of the candidates relabelled uniformly at random among the labels present -> int32 [N]"""
    y = NG._xyz(y)
    b = np.floor((y - y.min(0)) / BLOCK).astype(np.int64)
    if b.max(initial=0) >= 64:
        raise ValueError("labels_of: more than 64 blocks on an axis")
    lab = ((b[:, 2] * 64 + b[:, 1]) * 64 + b[:, 0]).astype(np.int32)
    rng = np.random.default_rng(seed)
    noisy = rng.random(y.shape[0]) < NOISE
    present = np.unique(lab)
    lab[noisy] = present[rng.integers(0, present.shape[0], int(noisy.sum()))]
    return lab
