// Exact grid-indexed kNN of a point cloud: the table of sg_pointcloud_knn -- every point's k + 1 best-scoring points of the
// WHOLE cloud in sgcloud::pair_score, descending score, the lower original index first among equal scores -- bit for bit, without scoring
// every pair.  A uniform grid over the bounding box; a query walks the cells round its own in rings and stops once no point outside the
// block it has seen can reach its list: the rule is  Lb > delta - s_kth  with Lb a true lower bound of the squared distance to any unseen
// point and delta = 2^-19 * max|p|^2 a bound of |score + d^2| (the score is not the distance: its rounding error grows with |p|^2).
// Queries the rings do not settle are queued and finished by sgcloud::top_scores over the whole cloud, so the ring limit is a
// performance knob only, as is the cell edge.
//
//   k_grid_box          coordinates finite (one flag word), (x, y, z, |p|^2) per point, the bounding box, M2 = max |p|^2
//   k_grid_cells        per point its cell on 8g's formula floor((p - lo) / h) and the key (cz * ny + cy) * nx + cx: x runs fastest, so
//                       the cells (cx - r .. cx + r, y, z) of one row are ONE contiguous range of the sorted points
//   sort                stable radix sort of (key, index) over the key's bits in use (sort_device.h); k_grid_gather: the points in sorted order
//   k_grid_table        dense: start[c] = the first sorted point whose key is >= c, c = 0 .. cells; k_grid_cellstats: occupied, the largest
//   k_ring_search       one wave per 64 sorted points.  The lanes of one cell form a group and share their candidates: the rows of the
//                       block are staged through LDS in tiles of 256 (float4 + original index), every lane of the group scores its own
//                       query and inserts by (score, original index) into a register list.  Ring 1 is the 3 x 3 x 3 block, ring r adds
//                       the shell at Chebyshev distance r; a group stops when all its lanes are settled or its block covers the grid.
//   k_queue_search      the queued queries against the whole cloud in original order (cloud_knn_device.h)
//
// The lists are written at the ORIGINAL row with ORIGINAL indices.  Plain launches, vector stores.
//
// sg_nearest_point_grid is the two-cloud, one-entry form: the same stages index the candidates y (box, E and M2 over the union
// of both clouds), the queries x are binned by the same formula and sorted by cell key, the same search walks the rings with a list of one
// entry, and the queue is finished by sg_nearest_point's own kernel (sgcloud::launch_nearest).
//
// sg_cloud_knn_cross_grid is the two-cloud form with a list of k entries: the index and the sorted queries of 8i, the walk,
// the `full` condition and the queue kernel of 8h.  Both two-cloud forms leave the squared distances per entry where they are asked for
// (k_list_d2).  sg_knn_vote is the majority vote over such rows (k_knn_vote): integers only.
//
// One of each for the three: k_ring_search<KK, Queries, Out> takes where its queries come from as a type (the sorted candidates
// themselves, or the sorted queries' original rows) and instantiates at KK = 6, 11, 21 (8h), 1 with int64 rows (8i) and 5, 10, 20 (8o);
// k_queue_search<KK> takes (queries, candidates), the self-kNN passing its candidates twice; k_list_d2<I> takes the index type.  On the
// host with_list maps k to the list length and grid_search drives everything behind an entry point's argument checks.
//
// The index's own pieces (k_grid_box .. k_grid_cellstats, the Grid, the workspace plan), the steps of its build and the search skeleton
// (group pick, tile staging, the kernels' leave) live in grid_index_device.h, which the radius graph (kernels_radius.hip)
// includes as well; the ring walk with its settled test, the cell-edge choice (fit, the probe, the occupancy correction) and the entry
// points are here.
#include <cmath>
#include <cstring>
#include <type_traits>

#include "sg_common.h"
#include "sort_device.h"
#include "cloud_knn_device.h"
#include "overseg_device.h"
#include "grid_index_device.h"

namespace {

using namespace sggrid;
using sgcloud::kTile;

// (score, original index): the higher score first, the lower index first among equal scores -- whatever order the candidates arrive in
template <int KK>
__device__ __forceinline__ void insert(float sc, int id, float (&bs)[KK], int (&bi)[KK]) {
    if (sc > bs[KK - 1] || (sc == bs[KK - 1] && id < bi[KK - 1])) {
        float v = sc;
        int w = id;
        bool placed = false;
#pragma unroll
        for (int t = 0; t < KK; ++t) {
            if (placed || v > bs[t] || (v == bs[t] && w < bi[t])) {
                placed = true;
                const float tv = bs[t]; const int ti = bi[t];
                bs[t] = v; bi[t] = w; v = tv; w = ti;
            }
        }
    }
}

// the sorted points [a, b) (wave-uniform) through LDS in tiles; the lanes with `active` score them
template <int KK>
__device__ __forceinline__ void scan_range(int a, int b, bool active, const float4& me, const float4* __restrict__ spts,
                                           const int* __restrict__ sidx, float4* tile, int* tidx, float (&bs)[KK], int (&bi)[KK],
                                           unsigned int& evals) {
    for (int c0 = a; c0 < b; c0 += kGTile) {
        const int n = stage_tile(c0, b, spts, sidx, tile, tidx);
        if (active) {
            for (int j = 0; j < n; ++j) insert<KK>(sgcloud::pair_score(me.x, me.y, me.z, me.w, tile[j]), tidx[j], bs, bi);
            evals += (unsigned int)n;
        }
    }
}

// ring r round the cell (gx, gy, gz): ring 1 is the 3 x 3 x 3 block, ring r > 1 the shell at Chebyshev distance r (whole row pieces where
// |dy| or |dz| is r, the two end cells elsewhere).  Wave-uniform; the lanes with `act` score what is staged.
template <int KK>
__device__ __forceinline__ void scan_ring(const Grid& g, int gx, int gy, int gz, int r, const int* __restrict__ start, bool act, const float4& me,
                                          const float4* __restrict__ spts, const int* __restrict__ sidx, float4* tile, int* tidx, float (&bs)[KK],
                                          int (&bi)[KK], unsigned int& evals) {
    const int nx = g.nc[0], ny = g.nc[1], nz = g.nc[2];
    for (int dz = -r; dz <= r; ++dz) {
        const int z = gz + dz;
        if (z < 0 || z >= nz) continue;
        for (int dy = -r; dy <= r; ++dy) {
            const int y = gy + dy;
            if (y < 0 || y >= ny) continue;
            const int row = (z * ny + y) * nx;
            const bool inner = r > 1 && max(abs(dy), abs(dz)) < r;
            if (!inner) {                                   // the whole row piece of the block
                const int x0 = max(gx - r, 0), x1 = min(gx + r, nx - 1);
                scan_range<KK>(start[row + x0], start[row + x1 + 1], act, me, spts, sidx, tile, tidx, bs, bi, evals);
            } else {                                        // the block of ring r - 1 holds the middle: the two end cells
                if (gx - r >= 0) scan_range<KK>(start[row + gx - r], start[row + gx - r + 1], act, me, spts, sidx, tile, tidx, bs, bi, evals);
                if (gx + r < nx) scan_range<KK>(start[row + gx + r], start[row + gx + r + 1], act, me, spts, sidx, tile, tidx, bs, bi, evals);
            }
        }
    }
}

// after ring r: every point outside the block is at least gap away along one axis; the whole grid seen settles everybody.
// s_last: the last score of the list, full: the list holds that many candidates
__device__ __forceinline__ bool ring_settles(const Grid& g, int gx, int gy, int gz, int r, float s_last, bool full) {
    const bool all = gx - r <= 0 && gx + r >= g.nc[0] - 1 && gy - r <= 0 && gy + r >= g.nc[1] - 1 && gz - r <= 0 && gz + r >= g.nc[2] - 1;
    const float gap = (float)r * g.h - g.slack;
    const float lhs = (gap * gap) * kShrink;
    const float rhs = g.delta - s_last;
    return all || (full && gap > 0.0f && lhs > rhs);
}

struct Walk {
    bool queued;                    // the rings did not settle this lane's query: it goes to the queue
    int ring;                       // the ring that settled it (0: none)
    unsigned int evals;             // pair scores this lane evaluated
};

// The walk of one wave: its groups in turn, each ring by ring until all its lanes are settled or the ring limit is reached;
// the list is left in bs / bi.  The counters are locals returned by value, as pick_group's are.
template <int KK>
__device__ __forceinline__ Walk ring_walk(const Grid& g, bool live, int mycell, const float4& me, const int* __restrict__ start,
                                          const float4* __restrict__ spts, const int* __restrict__ sidx, float4* tile, int* tidx, float (&bs)[KK],
                                          int (&bi)[KK]) {
#pragma unroll
    for (int t = 0; t < KK; ++t) { bs[t] = -INFINITY; bi[t] = 0x7fffffff; }
    bool done = !live, queued = false;
    int myr = 0;
    unsigned int evals = 0u;
    while (const unsigned long long pending = pending_lanes(done)) {
        const Group grp = pick_group(g, pending, done, mycell);
        for (int r = 1; r <= g.rmax; ++r) {
            const bool act = grp.in && !done;
            scan_ring<KK>(g, grp.x, grp.y, grp.z, r, start, act, me, spts, sidx, tile, tidx, bs, bi, evals);
            if (act && ring_settles(g, grp.x, grp.y, grp.z, r, bs[KK - 1], bi[KK - 1] != 0x7fffffff)) { done = true; myr = r; }
            if (__builtin_amdgcn_ballot_w64(grp.in && !done) == 0ull) break;
        }
        if (grp.in && !done) { done = true; queued = true; }
    }
    return Walk{queued, myr, evals};
}

// Where a wave's 64 queries come from, as a type (no run-time branch): slot sl of the sorted order -> the query, returned by value as
// pick_group's Group is.  Both read (points, sorted keys, sorted indices), plain kernel arguments.
struct Query {
    float4 me;                          // (x, y, z, |q|^2)
    int cell, orig;                     // its cell key; the row its list goes to
};
struct SortedCandidates {               // the self-kNN (8h): the sorted candidates are the queries, pts is in sorted order
    static __device__ __forceinline__ Query load(const float4* __restrict__ pts, const unsigned long long* __restrict__ key,
                                                 const int* __restrict__ idx, int sl) {
        return Query{pts[sl], (int)key[sl], idx[sl]};
    }
};
struct SortedQueries {                  // two clouds (8i, 8o): the queries' sorted keys name their ORIGINAL rows, pts is in original order
    static __device__ __forceinline__ Query load(const float4* __restrict__ pts, const unsigned long long* __restrict__ key,
                                                 const int* __restrict__ idx, int sl) {
        const int orig = idx[sl];
        return Query{pts[orig], (int)key[sl], orig};
    }
};

// The search: one wave per 64 of the Q queries in the order of their cell keys; the lanes of one cell form a group
// and share the staged candidate tiles through ring_walk, each with a list of KK entries.  A list that is not full is unsettled
// (ring_settles takes `full`): with KK = 1 a query whose block holds no candidate keeps -inf and walks on.  Row orig of `out` [Q, KK]
// receives the list, original candidate indices; queries unsettled at the ring limit are queued with their original row.
template <int KK, class Queries, class Out>
__global__ __launch_bounds__(kWave) void k_ring_search(const float4* __restrict__ spts, const int* __restrict__ sidx, const int* __restrict__ start,
                                                       Grid g, const float4* __restrict__ qpts, const unsigned long long* __restrict__ qskey,
                                                       const int* __restrict__ qsidx, int Q, Out* __restrict__ out, int* __restrict__ queue,
                                                       Misc* __restrict__ m, int counting) {
    __shared__ float4 tile[kGTile];
    __shared__ int tidx[kGTile];
    const int s = blockIdx.x * kWave + threadIdx.x;
    const bool live = s < Q;
    const Query q = Queries::load(qpts, qskey, qsidx, live ? s : Q - 1);
    const int orig = q.orig;
    float bs[KK];
    int bi[KK];
    const Walk w = ring_walk<KK>(g, live, q.cell, q.me, start, spts, sidx, tile, tidx, bs, bi);
    if (live) {
        if (w.queued) {
            queue[atomicAdd(&m->nq, 1)] = orig;
        } else {
#pragma unroll
            for (int t = 0; t < KK; ++t) out[(size_t)orig * KK + t] = (Out)bi[t];
        }
    }
    search_epilogue(w.ring, w.evals, counting, m);
}

// The queued queries (rows of qpts [U]) against all N candidates in original order, by sgcloud::top_scores: k_pc_knn for a compacted
// list.  The self-kNN passes its candidates as the queries.  Every caller has N >= KK, so top_scores leaves a full list of real indices
// and the clamp never acts; it only keeps a stored index inside the cloud whatever happens.
template <int KK>
__global__ __launch_bounds__(kTile) void k_queue_search(const float4* __restrict__ cand, int N, const float4* __restrict__ qpts, int U,
                                                        const int* __restrict__ queue, int nq, int32_t* __restrict__ out, Misc* __restrict__ m,
                                                        int counting) {
    __shared__ float4 tile[kTile];
    const int u = blockIdx.x * kTile + threadIdx.x;
    const bool live = u < nq;
    const int q = live ? queue[u] : 0;
    const bool sane = (unsigned)q < (unsigned)U;
    const float4 me = qpts[sane ? q : 0];
    float bs[KK];
    int bi[KK];
    sgcloud::top_scores<KK>(cand, N, me, tile, bs, bi);
    if (live && sane) {
#pragma unroll
        for (int t = 0; t < KK; ++t) out[(size_t)q * KK + t] = bi[t] < N ? bi[t] : N - 1;
    }
    if (counting && threadIdx.x == 0) atomicAdd(&m->evals, (unsigned long long)min(kTile, nq - blockIdx.x * kTile) * (unsigned long long)N);
}

// d2[u][t] = (dx*dx + dy*dy) + dz*dz with d = x[u] - y[idx[u][t]], every operation rounded once (the file is built without contraction);
// INFINITY for an index outside the candidates.  One thread per entry (total = U k < 2^31).  K: the entries a row when the caller knows
// them at compile time (the nearest point: 1, which spares the division), 0: k.
template <class I, int K>
__global__ __launch_bounds__(kBlock) void k_list_d2(const float* __restrict__ x, int xs, const float* __restrict__ y, int ys, int N, int k,
                                                    int total, const I* __restrict__ idx, float* __restrict__ d2) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (long long)total) return;
    const int u = (int)(e / (K ? K : k));
    const I j = idx[e];
    if ((std::make_unsigned_t<I>)j >= (std::make_unsigned_t<I>)N) { d2[e] = INFINITY; return; }
    const float dx = x[(size_t)u * xs] - y[(size_t)j * ys], dy = x[(size_t)u * xs + 1] - y[(size_t)j * ys + 1];
    const float dz = x[(size_t)u * xs + 2] - y[(size_t)j * ys + 2];
    d2[e] = (dx * dx + dy * dy) + dz * dz;
}

// The vote over a row of neighbours: one thread per row, the row's labels in registers (KC >= k slots, the loops unrolled
// over them), k^2 equality compares.  c(t) = the entries that carry entry t's label; the first t with the largest c wins.  A later t with
// the same count and another label marks a tie; a strictly larger count clears it (nothing earlier reaches it).  An index outside 0..N-1
// sets the flag and leaves the row unwritten.
template <int KC>
__global__ __launch_bounds__(kBlock) void k_knn_vote(const int32_t* __restrict__ knn, int U, int k, const int32_t* __restrict__ label, int N,
                                                     int32_t* __restrict__ winner, int32_t* __restrict__ rep, int32_t* __restrict__ count,
                                                     int32_t* __restrict__ tied, int* __restrict__ flag) {
    const long long u = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (u >= (long long)U) return;
    const int32_t* row = knn + (size_t)u * k;
    int lab[KC];
    bool bad = false;
#pragma unroll
    for (int t = 0; t < KC; ++t) {
        lab[t] = 0;
        if (t < k) {
            const int j = row[t];
            const bool ok = (unsigned)j < (unsigned)N;
            bad |= !ok;
            lab[t] = label[ok ? j : 0];
        }
    }
    if (bad) { atomicOr(flag, 1); return; }
    int best = 0, bestc = 0, bestlab = 0, tie = 0;
#pragma unroll
    for (int t = 0; t < KC; ++t) {
        if (t < k) {
            int c = 0;
#pragma unroll
            for (int s = 0; s < KC; ++s) c += (s < k && lab[s] == lab[t]) ? 1 : 0;
            if (c > bestc) { bestc = c; best = t; bestlab = lab[t]; tie = 0; }
            else if (c == bestc && lab[t] != bestlab) tie = 1;
        }
    }
    winner[u] = bestlab;
    rep[u] = row[best];
    if (count) count[u] = bestc;
    if (tied) tied[u] = tie;
}


// the queries of the two-cloud search: (x, y, z, |q|^2) in original order, their cell keys and the sort's buffers, the queue
struct QueryPlan {
    float4* pts;
    unsigned long long *k0, *k1;
    int *v0, *v1;
    int* hist;
    int* queue;
};

void carve(sg::Carver& cv, QueryPlan& q, int U) {
    const size_t n = (size_t)std::max(U, 1);
    q.pts = cv.take<float4>(n);
    q.k0 = cv.take<unsigned long long>(n);
    q.k1 = cv.take<unsigned long long>(n);
    q.v0 = cv.take<int>(n);
    q.v1 = cv.take<int>(n);
    q.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    q.queue = cv.take<int>(n);
}

size_t query_plan_bytes(int U) {
    const size_t n = (size_t)std::max(U, 1);
    return sg::align_up(n * 16) + 2 * sg::align_up(n * 8) + 3 * sg::align_up(n * 4) + sg::align_up(sgsort::hist_ints((long long)n) * 4);
}


constexpr int kStages = 7;
const char* const kStageNames[kStages] = {"box", "probe", "cells", "sort", "table", "search", "fallback"};

// what a thread asked for and what its last call left: one set per entry point (the kNN, the nearest point, the two-cloud kNN)
struct Session {
    sgos::StageTimes<kStages> times;
    int64_t stats[kNumStats];
    int target = 0, ring_limit = 0;         // 0: the defaults
};
thread_local Session t_knn, t_nearest, t_cross;

int stats_of(const Session& s, const char* who, int64_t* h, int cap) {
    SG_REQUIRE(h && cap >= kNumStats, "%s: room for %d words is needed", who, kNumStats);
    for (int i = 0; i < kNumStats; ++i) h[i] = s.stats[i];
    return kNumStats;
}

int set_tuning(Session& s, const char* who, int target_occupancy, int ring_limit) {
    SG_REQUIRE(target_occupancy >= 0 && target_occupancy <= 4096 && ring_limit >= 0 && ring_limit <= kMaxRingLimit,
               "%s: target occupancy 0..4096 and ring limit 0..%d (0: the default)", who, kMaxRingLimit);
    s.target = target_occupancy;
    s.ring_limit = ring_limit;
    return SG_OK;
}

// The stages box, probe, cells, sort and table over the N candidates of `d_points`, through grid_index_device.h's
// steps: measure, the cell edge (the caller's, or the probe's below), bin, sort_cells, finish_index.  With queries (d_q, U > 0) the box
// covers both clouds and q_pts receives the queries; the index itself holds the candidates only.  `brute`: the entry point that decides a
// cloud whose score margin is not finite.
int build_index(const char* who, const char* brute, const Session& ses, const float* d_points, int stride, int N, const float* d_q, int qstride,
                int U, float4* q_pts, float cell, const Plan& p, sgos::StageClock<kStages>& clock, hipStream_t st, Index* out) {
    const int nb = sg::cdiv(N, kBlock);
    Grid& g = out->g;
    Measured ms;
    if (const int rc = measure(who, d_points, stride, N, d_q, qstride, U, q_pts, p, st, &g, &ms)) return rc;
    float m2;
    std::memcpy(&m2, &ms.hm.m2, 4);
    g.delta = std::max(std::ldexp(m2, -19), std::ldexp(1.0f, -100));
    if (!std::isfinite(4.0f * m2) || !std::isfinite(g.delta))
        return sg::fail(SG_EUNSUP, "%s: the coordinates are too large for the grid's score margin (max |p|^2 = %g); the brute-force path "
                                   "(%s) decides such a cloud", who, (double)m2, brute);
    clock.tick();
    g.rmax = ses.ring_limit > 0 ? ses.ring_limit : kRingLimit;
    const long long cap = cell_cap(N);
    long long total = 0;
    // h, enlarged until no axis reaches 2^21 cells and the grid fits the table
    auto fit = [&](float h) {
        if (!(h > 0.0f) || !std::isfinite(h)) h = 1.0f;
        for (int tries = 0; tries < 400; ++tries) {
            if (cells_of(ms.ext, h, g.nc, &total) && total <= cap) return h;
            h *= 1.25f;
        }
        return ms.emax > 0.0f ? ms.emax * 2.0f : 1.0f;  // one cell per axis
    };
    Sorted sorted{};
    bool binned = false;
    if (cell > 0.0f) {
        if (const int rc = check_cell(who, ms, cell, N, &g, &total)) return rc;
        clock.tick();
    } else {
        // first guess: the cloud as a surface of the box's half area (a line: its length), `target` points per cell
        const float target = (float)(ses.target > 0 ? ses.target : kTargetOccupancy);
        const float area = ms.ext[0] * ms.ext[1] + ms.ext[1] * ms.ext[2] + ms.ext[0] * ms.ext[2];
        const float h0 = fit(std::max(std::sqrt(target * area / (float)N), target * ms.emax / (float)N));
        bin(ms, h0, p, N, st, &g);
        sorted = sort_cells(p.k0, p.k1, p.v0, p.v1, p.hist, N, g.ncells, st);
        k_grid_heads<<<nb, kBlock, 0, st>>>(sorted.key, N, &p.misc->heads);
        int heads = 0;
        SG_HIP(hipMemcpyAsync(&heads, &p.misc->heads, 4, hipMemcpyDeviceToHost, st));
        SG_HIP(hipStreamSynchronize(st));
        SG_LAUNCH_CHECK();
        if (heads < 1 || heads > N) return sg::fail(SG_EHIP, "%s: %d occupied cells from %d points", who, heads, N);
        // one correction towards the target: on a surface the occupancy grows with h^2
        const float occ = (float)N / (float)heads;
        cell = h0;
        binned = true;
        if (occ < 0.75f * target || occ > 1.5f * target) {
            const float h1 = fit(h0 * std::sqrt(target / occ));
            if (h1 != h0) { cell = h1; binned = false; }
        }
        clock.tick();
    }
    if (!binned) bin(ms, cell, p, N, st, &g);
    clock.tick();
    if (!binned) sorted = sort_cells(p.k0, p.k1, p.v0, p.v1, p.hist, N, g.ncells, st);
    finish_index(p, sorted, N, clock, st, out);
    return SG_OK;
}

// k in {5, 10, 20} (the entry points refuse every other) -> f(the list length k + kExtra as a constant)
template <int kExtra, class F>
void with_list(int k, F&& f) {
    if (k == 5) f(std::integral_constant<int, 5 + kExtra>{});
    else if (k == 10) f(std::integral_constant<int, 10 + kExtra>{});
    else f(std::integral_constant<int, 20 + kExtra>{});
}

enum class Form { kSelf, kNearest, kCross };     // 8h: lists of k + 1 over the cloud itself; 8i: one entry, int64; 8o: lists of k

// Everything behind an entry point's argument checks: the workspace, the index (build_index: the stages box .. table), for two clouds
// the queries binned by the index's formula and sorted by cell key, then the stage "search" -- the ring search and the read-back of what
// it left -- and the stage "fallback": the queue against every candidate (8i: by sg_nearest_point's own kernel, its nq * N scores counted
// here) and the squared distances where they are asked for.  kSelf takes no queries (d_x = nullptr, U = 0): the N candidates are the queries.
template <Form F, class Out>
int grid_search(const char* who, const char* brute, Session& ses, const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N,
                int k, float cell, Out* d_out, float* d_d2, void* d_ws, size_t ws_bytes, void* stream) {
    constexpr bool kSelf = F == Form::kSelf;
    using Queries = std::conditional_t<kSelf, SortedCandidates, SortedQueries>;
    auto for_list = [&](auto&& f) {
        if constexpr (F == Form::kNearest) f(std::integral_constant<int, 1>{});
        else with_list<kSelf ? 1 : 0>(k, f);
    };
    Plan p{};
    QueryPlan q{};
    sg::Carver cv(d_ws, ws_bytes);
    carve(cv, p, N);
    if (!kSelf) carve(cv, q, U);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu bytes)", who, ws_bytes);
    hipStream_t st = sg::as_stream(stream);
    const int counting = ses.times.timing ? 1 : 0;
    sgos::StageClock<kStages> clock(st, ses.times.timing, ses.times.us);
    Index ix{};
    const int rc = build_index(who, brute, ses, d_y, y_stride, N, d_x, x_stride, U, q.pts, cell, p, clock, st, &ix);
    if (rc != SG_OK) return rc;
    const Grid& g = ix.g;
    const int Q = kSelf ? N : U;
    const float4* qpts = kSelf ? p.cand : q.pts;
    int* queue = kSelf ? p.queue : q.queue;
    Sorted s{ix.skey, ix.sidx};
    if (!kSelf) {
        // the queries in the order of their cell keys: 64 consecutive ones are a wave's groups
        k_grid_cells<<<sg::cdiv(U, kBlock), kBlock, 0, st>>>(q.pts, U, g, q.k0, q.v0);
        s = sort_cells(q.k0, q.k1, q.v0, q.v1, q.hist, U, g.ncells, st);
    }
    const float4* from = kSelf ? p.spts : q.pts;                  // what Queries::load reads: SortedCandidates the sorted points themselves
    for_list([&](auto kk) {
        k_ring_search<decltype(kk)::value, Queries, Out><<<sg::cdiv(Q, kWave), kWave, 0, st>>>(p.spts, ix.sidx, p.start, g, from, s.key, s.idx, Q,
                                                                                              d_out, queue, p.misc, counting);
    });
    clock.tick();
    Misc hm{};
    SG_HIP(hipMemcpyAsync(&hm, p.misc, sizeof(Misc), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    const int nq = hm.nq;
    if (nq < 0 || nq > Q) return sg::fail(SG_EHIP, "%s: %d queued queries from %d%s", who, nq, Q, kSelf ? " points" : "");
    if (nq > 0) {
        if constexpr (F == Form::kNearest) {
            // sg_nearest_point's kernel, scattered to the queries' rows
            sgcloud::launch_nearest(d_x, x_stride, queue, nq, p.cand, N, d_out, 1, st);
            if (counting) hm.evals += (unsigned long long)nq * (unsigned long long)N;
        } else {
            for_list([&](auto kk) {
                k_queue_search<decltype(kk)::value><<<sg::cdiv(nq, kTile), kTile, 0, st>>>(p.cand, N, qpts, Q, queue, nq, d_out, p.misc, counting);
            });
            if (counting) SG_HIP(hipMemcpyAsync(&hm.evals, &p.misc->evals, 8, hipMemcpyDeviceToHost, st));
            if (counting || kSelf) SG_HIP(hipStreamSynchronize(st));      // 8h has always returned with its queue finished
        }
    }
    if (d_d2) {
        constexpr int kOne = F == Form::kNearest ? 1 : 0;
        const int per = kOne ? 1 : k, total = U * per;
        k_list_d2<Out, kOne><<<sg::cdiv(total, kBlock), kBlock, 0, st>>>(d_x, x_stride, d_y, y_stride, N, per, total, d_out, d_d2);
    }
    clock.tick();
    SG_LAUNCH_CHECK();
    index_stats(ses.stats, g, hm);
    ses.stats[6] = hm.maxring; ses.stats[7] = nq; ses.stats[8] = (int64_t)hm.evals;
    return SG_OK;
}

// What the two two-cloud entry points refuse alike, in their order, behind the checks that are their own; `entries` a row (8i: 1)
template <Form F, class Out>
int two_cloud_search(const char* who, Session& ses, const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, int entries,
                     float cell, Out* d_out, float* d_d2, void* d_ws, size_t ws_bytes, void* stream) {
    if (N > SG_MAX_GRID_POINTS) return sg::fail(SG_EUNSUP, "%s: %d candidates; the grid path holds at most %d", who, N, SG_MAX_GRID_POINTS);
    if (U > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d queries; a call takes at most %d", who, U, SG_MAX_CLOUD_POINTS);
    if ((long long)U * entries > 0x7fffffffll)
        return sg::fail(SG_EUNSUP, "%s: %d queries of %d neighbours; a table holds at most 2^31 - 1 entries", who, U, entries);
    SG_REQUIRE(y_stride >= 3 && x_stride >= 3, "%s: rows of at least 3 floats (x: %d, y: %d)", who, x_stride, y_stride);
    SG_REQUIRE(std::isfinite(cell) && cell >= 0.0f, "%s: the cell edge must be finite and positive, or 0 for the library's choice (%g)", who, (double)cell);
    if (U == 0) return SG_OK;
    SG_REQUIRE(d_x && d_y && d_out && d_ws, "%s: bad arguments", who);
    const size_t need = plan_bytes(N) + query_plan_bytes(U);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    return grid_search<F>(who, "sg_nearest_point", ses, d_x, x_stride, U, d_y, y_stride, N, entries, cell, d_out, d_d2, d_ws, ws_bytes, stream);
}

// sg_<family>_stats and sg_<family>_set_tuning over the family's Session
#define SG_GRID_SESSION_API(family, ses)                                                                                      \
    int sg_##family##_stats(int64_t* h, int cap) { return stats_of(ses, "sg_" #family "_stats", h, cap); }                   \
    int sg_##family##_set_tuning(int target_occupancy, int ring_limit) {                                                      \
        return set_tuning(ses, "sg_" #family "_set_tuning", target_occupancy, ring_limit);                                   \
    }

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(pointcloud_knn_grid, t_knn.times, kStageNames)
SG_GRID_SESSION_API(pointcloud_knn_grid, t_knn)

size_t sg_pointcloud_knn_grid_ws_bytes(int N, int k) {
    if (N < 1 || N > SG_MAX_GRID_POINTS || (k != 5 && k != 10 && k != 20)) return 0;
    return plan_bytes(N);
}

int sg_pointcloud_knn_grid(const float* d_points, int stride, int N, int k, float cell, int32_t* d_knn, void* d_ws, size_t ws_bytes,
                           void* stream) {
    const char* who = "sg_pointcloud_knn_grid";
    for (int i = 0; i < kNumStats; ++i) t_knn.stats[i] = 0;
    if (k != 5 && k != 10 && k != 20) return sg::fail(SG_EUNSUP, "%s: k = %d is not built (5, 10 = the reference's default, 20)", who, k);
    SG_REQUIRE(N > 0, "%s: bad arguments", who);
    if (N <= k) return sg::fail(SG_EINVAL, "%s: %d points for k = %d (topk(k + 1) raises in the reference)", who, N, k);
    if (N > SG_MAX_GRID_POINTS) return sg::fail(SG_EUNSUP, "%s: %d points; the grid path holds at most %d", who, N, SG_MAX_GRID_POINTS);
    SG_REQUIRE(d_points && stride >= 3 && d_knn && d_ws, "%s: bad arguments", who);
    SG_REQUIRE(std::isfinite(cell) && cell >= 0.0f, "%s: the cell edge must be finite and positive, or 0 for the library's choice (%g)", who, (double)cell);
    if (ws_bytes < plan_bytes(N)) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, plan_bytes(N));
    return grid_search<Form::kSelf>(who, "sg_pointcloud_knn", t_knn, nullptr, 0, 0, d_points, stride, N, k, cell, d_knn, nullptr, d_ws, ws_bytes,
                                    stream);
}

SG_STAGE_TIMER_API(nearest_point_grid, t_nearest.times, kStageNames)
SG_GRID_SESSION_API(nearest_point_grid, t_nearest)

size_t sg_nearest_point_grid_ws_bytes(int U, int N) {
    if (U < 0 || U > SG_MAX_CLOUD_POINTS || N < 1 || N > SG_MAX_GRID_POINTS) return 0;
    return plan_bytes(N) + query_plan_bytes(U);
}

int sg_nearest_point_grid(const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, float cell, int64_t* d_idx, float* d_d2,
                          void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_nearest_point_grid";
    for (int i = 0; i < kNumStats; ++i) t_nearest.stats[i] = 0;
    SG_REQUIRE(N >= 1 && U >= 0, "%s: bad arguments (%d queries, %d candidates)", who, U, N);
    return two_cloud_search<Form::kNearest>(who, t_nearest, d_x, x_stride, U, d_y, y_stride, N, 1, cell, d_idx, d_d2, d_ws, ws_bytes, stream);
}

SG_STAGE_TIMER_API(cloud_knn_cross_grid, t_cross.times, kStageNames)
SG_GRID_SESSION_API(cloud_knn_cross_grid, t_cross)

size_t sg_cloud_knn_cross_grid_ws_bytes(int U, int N, int k) {
    if ((k != 5 && k != 10 && k != 20) || U < 0 || U > SG_MAX_CLOUD_POINTS || N < k || N > SG_MAX_GRID_POINTS) return 0;
    if ((long long)U * k > 0x7fffffffll) return 0;
    return plan_bytes(N) + query_plan_bytes(U);
}

int sg_cloud_knn_cross_grid(const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, int k, float cell, int32_t* d_knn,
                            float* d_d2, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_cloud_knn_cross_grid";
    for (int i = 0; i < kNumStats; ++i) t_cross.stats[i] = 0;
    if (k != 5 && k != 10 && k != 20) return sg::fail(SG_EUNSUP, "%s: k = %d is not built (5, 10, 20)", who, k);
    SG_REQUIRE(U >= 0, "%s: bad arguments (%d queries, %d candidates)", who, U, N);
    if (N < k) return sg::fail(SG_EINVAL, "%s: %d candidates for k = %d", who, N, k);
    return two_cloud_search<Form::kCross>(who, t_cross, d_x, x_stride, U, d_y, y_stride, N, k, cell, d_knn, d_d2, d_ws, ws_bytes, stream);
}

int sg_knn_vote(const int32_t* d_knn, int U, int k, const int32_t* d_label, int N, int32_t* d_winner, int32_t* d_rep, int32_t* d_count,
                int32_t* d_tied, void* stream) {
    const char* who = "sg_knn_vote";
    SG_REQUIRE(k >= 1 && k <= 32, "%s: 1 <= k <= 32 neighbours a row (%d)", who, k);
    SG_REQUIRE(U >= 0 && N >= 1, "%s: bad arguments (%d rows, %d labels)", who, U, N);
    if (U == 0) return SG_OK;
    SG_REQUIRE(d_knn && d_label && d_winner && d_rep, "%s: bad arguments", who);
    hipStream_t st = sg::as_stream(stream);
    int* d_flag = nullptr;                                      // the call has no workspace: its one flag word
    SG_HIP(hipMalloc((void**)&d_flag, sizeof(int)));
    int flag = 0;
    hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(int), st);
    if (e == hipSuccess) {
        const int nb = sg::cdiv(U, kBlock);
        if (k <= 5) k_knn_vote<5><<<nb, kBlock, 0, st>>>(d_knn, U, k, d_label, N, d_winner, d_rep, d_count, d_tied, d_flag);
        else if (k <= 10) k_knn_vote<10><<<nb, kBlock, 0, st>>>(d_knn, U, k, d_label, N, d_winner, d_rep, d_count, d_tied, d_flag);
        else if (k <= 20) k_knn_vote<20><<<nb, kBlock, 0, st>>>(d_knn, U, k, d_label, N, d_winner, d_rep, d_count, d_tied, d_flag);
        else k_knn_vote<32><<<nb, kBlock, 0, st>>>(d_knn, U, k, d_label, N, d_winner, d_rep, d_count, d_tied, d_flag);
        e = hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    (void)hipFree(d_flag);
    if (e != hipSuccess) return sg::fail(SG_EHIP, "%s: %s", who, hipGetErrorString(e));
    if (flag) return sg::fail(SG_EINVAL, "%s: a neighbour index outside 0..%d", who, N - 1);
    return SG_OK;
}

}  // extern "C"
