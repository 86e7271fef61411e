// The radius graph on the exact grid index: every pair of points with  j != i  and  d2 <= r2 , d = p_j - p_i,
// d2 = (d0*d0 + d1*d1) + d2*d2 in fp32 with every operation rounded once (the file is built without contraction), r2 = radius * radius
// rounded once on the host -- 8j's pair predicate, over ALL pairs and not over a kNN table.  Two things are computed inside the search,
// without an adjacency: count[i] = the pairs of i (sg_radius_count_grid) and the connected components of the graph (sg_components_radius,
// 8j's outputs and conventions).
//
//   index     grid_index_device.h: measure (box and finite check), bin (cells on 8g's formula), sort_cells, finish_index (gather, dense
//             table) -- the grid kNN's (8h); the cell edge and the rings are chosen here (rings_for)
//   R         the block of Chebyshev radius R round a query's cell holds every point that can pass: the smallest R with
//             gap = fl(fl(R h) - slack) > 0  and  fl(fl(gap * gap) * (1 - 2^-9)) > r2  (8h item 3 bounds the axis gap of a point outside the
//             block from below; 8k shows that the 2^-9 also pays for the roundings of d2).  Computed on the host, the same for every
//             query; no queue and no fallback.  cell = 0: h just large enough for R = 1, enlarged only until the grid fits the table.
//   search    k_radius_search<Visitor>: the grid kNN's search (k_ring_search) in shape, on the same pieces (pick_group, stage_tile, wave_sum).  One wave per 64
//             consecutive sorted points; the lanes of one cell form a group, taken in turn by ballot; the (2R+1)^2 row ranges of the
//             block come from the table; candidates are staged through LDS in tiles of 256 (float4 + original index); each lane of the
//             group tests its own query.  Nothing is indexed at run time.
//   Count     a register counter, one plain vector store at the original row
//   Hook      for a passing pair with original j > i (each edge once) and equal labels: 8j's hook (components_device.h) on the parent
//             array; k_cc_init before, k_cc_flatten and k_cc_sizes after, as they are.  The hooks run inside a divergent wave loop; no lane
//             waits for another, and the step budget bounds every lane's loop.
//   List      DESIGN.md 8l, sg_radius_neighbours_grid: the pairs written down in CSR form.  Count, a 64-bit exclusive scan (scan64_device.h),
//             T read back, the same search again with the n-th passing pair of i stored at raw[off[i] + n], then k_rn_rows puts every row
//             into ascending index (a rank sort, one wave per row) -- the stored order does not depend on the cell edge
#include <cmath>
#include <cstring>

#include "sg_common.h"
#include "grid_index_device.h"
#include "components_device.h"
#include "scan64_device.h"

namespace {

using sggrid::Grid;
using sggrid::Index;
using sggrid::kGTile;
using sggrid::kWave;

constexpr int kMaxR = 16;
constexpr int kNumStats = 9;
constexpr float kMinR2 = 7.8886090522101181e-31f;       // 2^-100: below, squares underflow and the relative error bounds of 8k do not hold

struct Tally {
    unsigned long long evals, passed;       // pair tests evaluated, pairs passed (timed calls only)
};

__global__ void k_radius_init(Tally* __restrict__ t) { t->evals = 0ull; t->passed = 0ull; }

struct CountVisitor {
    int32_t* count;
    __device__ __forceinline__ void pair(int, int, int) const {}
    __device__ __forceinline__ void finish(int i, int n) const { count[i] = n; }
};

struct HookVisitor {
    int* parent;
    const int32_t* label;
    sgcc::Misc* misc;
    int V;
    __device__ __forceinline__ void pair(int i, int j, int) const {
        if (j > i && (!label || label[i] == label[j])) sgcc::hook(parent, i, j, V, misc);
    }
    __device__ __forceinline__ void finish(int, int) const {}
};

// the n-th passing pair of i goes to the n-th place of i's row, in search order (k_rn_rows orders the row afterwards)
struct ListVisitor {
    const int64_t* off;
    int32_t* idx;
    __device__ __forceinline__ void pair(int i, int j, int n) const { idx[off[i] + n] = j; }
    __device__ __forceinline__ void finish(int, int) const {}
};

template <class Visitor>
__global__ __launch_bounds__(kWave) void k_radius_search(const float4* __restrict__ spts, const int* __restrict__ sidx,
                                                         const unsigned long long* __restrict__ skey, const int* __restrict__ start, Grid g, int N,
                                                         float r2, Visitor vis, Tally* __restrict__ tally, int counting) {
    __shared__ float4 tile[kGTile];
    __shared__ int tidx[kGTile];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * kWave + lane;
    const bool live = s < N;
    const int sl = live ? s : N - 1;
    const float4 me = spts[sl];
    const int mycell = (int)skey[sl];
    const int orig = sidx[sl];
    const int nx = g.nc[0], ny = g.nc[1], nz = g.nc[2], R = g.rmax;
    bool done = !live;
    int passed = 0;
    unsigned int evals = 0u;
    while (const unsigned long long pending = sggrid::pending_lanes(done)) {
        const sggrid::Group grp = sggrid::pick_group(g, pending, done, mycell);
        const int x0 = max(grp.x - R, 0), x1 = min(grp.x + R, nx - 1);
        for (int z = max(grp.z - R, 0); z <= min(grp.z + R, nz - 1); ++z) {
            for (int y = max(grp.y - R, 0); y <= min(grp.y + R, ny - 1); ++y) {
                const int row = (z * ny + y) * nx;
                const int a = start[row + x0], b = start[row + x1 + 1];          // one contiguous range of the sorted points
                for (int c0 = a; c0 < b; c0 += kGTile) {
                    const int n = sggrid::stage_tile(c0, b, spts, sidx, tile, tidx);
                    if (grp.in) {
                        for (int t = 0; t < n; ++t) {
                            const float4 c = tile[t];
                            const int j = tidx[t];
                            const float d0 = c.x - me.x, d1 = c.y - me.y, d2 = c.z - me.z;
                            const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
                            if (j != orig && dd <= r2) {
                                vis.pair(orig, j, passed);
                                ++passed;
                            }
                        }
                        evals += (unsigned int)n;
                    }
                }
            }
        }
        if (grp.in) done = true;
    }
    if (live) vis.finish(orig, passed);
    if (counting) {
        const unsigned long long e = sggrid::wave_sum(evals), p = sggrid::wave_sum(live ? (unsigned long long)passed : 0ull);
        if (lane == 0) { atomicAdd(&tally->evals, e); atomicAdd(&tally->passed, p); }
    }
}


// ---- the neighbour lists: off = the exclusive sum of count in 64 bits, the rows filled in search order, then ordered ----
constexpr int kRowBlock = 256;                              // k_rn_rows: four rows per block, one wave each

// One wave per row: raw[off[i] .. off[i+1]) in search order -> idx, the same entries in ascending index.  The entries of a row are
// distinct, so an entry's place is the number of entries below it: the wave holds 64 of its own entries and passes the row by in chunks
// of 64, each lane's chunk entry read across the wave.  A rank is below the row's length whatever the row holds: nothing is written
// outside the row.  The work of a row is its length squared / 64 (the envelope).
__global__ __launch_bounds__(kRowBlock) void k_rn_rows(const int64_t* __restrict__ off, const int32_t* __restrict__ raw, int N,
                                                       int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kRowBlock / 64) + (threadIdx.x >> 6);
    if (i >= N) return;                                      // whole waves leave; there is no barrier below
    const int64_t lo = off[i];
    const int64_t len = off[i + 1] - lo;
    const int32_t* __restrict__ row = raw + lo;
    int32_t* __restrict__ out = idx + lo;
    const int top = 0x7fffffff;                              // never below an entry
    for (int64_t e0 = 0; e0 < len; e0 += 64) {
        const bool mine_live = e0 + lane < len;
        const int mine = mine_live ? row[e0 + lane] : top;
        int64_t rank = 0;
        for (int64_t c0 = 0; c0 < len; c0 += 64) {
            const int c = c0 + lane < len ? row[c0 + lane] : top;
#pragma unroll
            for (int u = 0; u < 64; ++u) rank += __builtin_amdgcn_readlane(c, u) < mine ? 1 : 0;
        }
        if (mine_live) out[rank] = mine;
    }
}

struct Plan {
    sggrid::Plan grid;
    Tally* tally;
    sgcc::Misc* misc;
    int* parent;
    int* count;
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, int N) {
    Plan p{};
    sg::Carver cv(d_ws, ws_bytes);
    sggrid::carve(cv, p.grid, N);
    p.tally = cv.take<Tally>(1);
    p.misc = cv.take<sgcc::Misc>(1);
    p.parent = cv.take<int>((size_t)N);
    p.count = cv.take<int>((size_t)N);
    p.ok = cv.ok;
    return p;
}

constexpr int kStages = 7;
const char* const kStageNames[kStages] = {"box", "cells", "sort", "table", "init", "search", "finish"};

struct Session {
    sgos::StageTimes<kStages> times;
    int64_t stats[kNumStats];
};
thread_local Session t_ses;

// the smallest block radius at cell edge h that no passing point can lie outside of; 0: above kMaxR
int rings_for(float h, float slack, float r2) {
    for (int r = 1; r <= kMaxR; ++r) {
        const float gap = (float)r * h - slack;
        const float lhs = (gap * gap) * sggrid::kShrink;
        if (gap > 0.0f && lhs > r2) return r;
    }
    return 0;
}

// box, cells, sort, table: grid_index_device.h's steps with the cell edge decided by the radius -- the caller's cell with as many rings
// as it needs, or the smallest edge that one ring serves.  Synchronises the stream once (the box).
template <class Clock>
int build_index(const char* who, const float* d_points, int stride, int N, float radius, float r2, float cell, const Plan& p, Clock& clock,
                hipStream_t st, Index* out) {
    const sggrid::Plan& gp = p.grid;
    k_radius_init<<<1, 1, 0, st>>>(p.tally);
    Grid& g = out->g;
    sggrid::Measured ms;
    if (const int rc = sggrid::measure(who, d_points, stride, N, nullptr, 0, 0, nullptr, gp, st, &g, &ms)) return rc;
    clock.tick();
    const float emax = ms.emax;
    if (!std::isfinite(emax)) return sg::fail(SG_EUNSUP, "%s: the extent of the cloud is not finite", who);
    const long long cap = sggrid::cell_cap(N);
    long long total = 0;
    if (cell > 0.0f) {
        g.rmax = rings_for(cell, g.slack, r2);
        if (g.rmax == 0)
            return sg::fail(SG_EUNSUP, "%s: a cell of %g needs a block of more than %d rings for a radius of %g", who, (double)cell, kMaxR,
                            (double)radius);
        if (const int rc = sggrid::check_cell(who, ms, cell, N, &g, &total)) return rc;
    } else {
        // just large enough for one ring; a larger edge keeps one ring (gap grows with h)
        cell = radius * 1.00390625f + g.slack;
        for (int tries = 0; tries < 64 && rings_for(cell, g.slack, r2) != 1; ++tries) cell *= 1.0009765625f;
        for (int tries = 0; tries < 400 && !(sggrid::cells_of(ms.ext, cell, g.nc, &total) && total <= cap); ++tries) cell *= 1.25f;
        if (!(sggrid::cells_of(ms.ext, cell, g.nc, &total) && total <= cap)) cell = std::max(cell, emax);      // at most two cells per axis
        g.rmax = rings_for(cell, g.slack, r2);
        if (g.rmax != 1 || !std::isfinite(cell) || !sggrid::cells_of(ms.ext, cell, g.nc, &total) || total > cap)
            return sg::fail(SG_EINTERNAL, "%s: no cell edge for a radius of %g on an extent of %g", who, (double)radius, (double)emax);
    }
    sggrid::bin(ms, cell, gp, N, st, &g);
    clock.tick();
    const sggrid::Sorted sorted = sggrid::sort_cells(gp.k0, gp.k1, gp.v0, gp.v1, gp.hist, N, g.ncells, st);
    sggrid::finish_index(gp, sorted, N, clock, st, out);
    return SG_OK;
}

void leave_stats(const Grid& g, const sggrid::Misc& hm, const Tally& t) {
    int64_t* s = t_ses.stats;
    sggrid::index_stats(s, g, hm);
    s[6] = g.rmax; s[7] = (int64_t)t.evals; s[8] = (int64_t)t.passed;
}

// everything that is checked before the first HIP call
int check_args(const char* who, const float* d_points, int stride, int N, float radius, float cell, const void* d_out, const void* d_ws,
               size_t ws_bytes, float* r2) {
    SG_REQUIRE(N >= 1, "%s: %d points", who, N);
    if (N > SG_MAX_GRID_POINTS) return sg::fail(SG_EUNSUP, "%s: %d points; the grid path holds at most %d", who, N, SG_MAX_GRID_POINTS);
    SG_REQUIRE(d_points && d_out && d_ws, "%s: a null pointer", who);
    SG_REQUIRE(stride >= 3, "%s: rows of at least 3 floats (%d)", who, stride);
    SG_REQUIRE(std::isfinite(radius) && radius > 0.0f, "%s: the radius must be finite and positive (%g)", who, (double)radius);
    *r2 = radius * radius;                       // one fp32 multiplication
    SG_REQUIRE(std::isfinite(*r2) && *r2 >= kMinR2, "%s: the square of the radius must be finite and at least 2^-100 (radius %g)", who, (double)radius);
    SG_REQUIRE(std::isfinite(cell) && cell >= 0.0f, "%s: the cell edge must be finite and positive, or 0 for the library's choice (%g)", who, (double)cell);
    if (ws_bytes < sg_radius_grid_ws_bytes(N))
        return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_radius_grid_ws_bytes(N));
    return SG_OK;
}

// the lists' own stages (sg_pcseg_edges_radius reports them in front of its own)
constexpr int kListStages = 8;
const char* const kListStageNames[kListStages] = {"box", "cells", "sort", "table", "count", "scan", "fill", "rows"};
thread_local sgos::StageTimes<kListStages> t_list;

size_t lists_ws_bytes(int N, long long capacity) {
    return sg_radius_grid_ws_bytes(N) + sg::align_up(((size_t)sgscan::tiles_of(N) + 1) * 8) + sg::align_up((size_t)capacity * 4);
}

const char* const kPairsWayOut = "take a smaller radius, or thin the cloud first";

}  // namespace

namespace sg {
void radius_lists_timing(bool on) { t_list.timing = on; }
const float* radius_lists_stage_us() { return t_list.us; }
const char* radius_lists_stage_name(int i) { return sgos::stage_name(kListStageNames, i); }

int radius_lists(const char* who, const float* d_points, int stride, int N, float radius, float cell, int64_t capacity, int64_t* d_off,
                 int32_t* d_idx, int64_t* h_T, void* d_ws, size_t ws_bytes, void* stream) {
    for (int i = 0; i < kNumStats; ++i) t_ses.stats[i] = 0;
    SG_REQUIRE(h_T, "%s: a null pointer", who);
    *h_T = 0;
    float r2 = 0.0f;
    if (const int rc = check_args(who, d_points, stride, N, radius, cell, d_off, d_ws, ws_bytes, &r2)) return rc;
    SG_REQUIRE(capacity >= 0 && (capacity == 0 || d_idx), "%s: room for %lld pairs at a null pointer", who, (long long)capacity);
    if (capacity > SG_MAX_RADIUS_PAIRS)
        return sg::fail(SG_EUNSUP, "%s: room for %lld pairs; the lists hold at most %lld: %s", who, (long long)capacity,
                        (long long)SG_MAX_RADIUS_PAIRS, kPairsWayOut);
    if (ws_bytes < lists_ws_bytes(N, capacity))
        return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, lists_ws_bytes(N, capacity));
    const Plan p = carve(d_ws, ws_bytes, N);
    const size_t base = sg_radius_grid_ws_bytes(N);
    sg::Carver cv((char*)d_ws + base, ws_bytes - base);
    const int nt = sgscan::tiles_of(N);
    long long* tsum = cv.take<long long>((size_t)nt + 1);
    int32_t* raw = cv.take<int32_t>((size_t)capacity);
    if (!p.ok || !cv.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, lists_ws_bytes(N, capacity));
    hipStream_t st = sg::as_stream(stream);
    const int counting = t_list.timing ? 1 : 0;
    sgos::StageClock<kListStages> clock(st, t_list.timing, t_list.us);
    Index ix{};
    if (const int rc = build_index(who, d_points, stride, N, radius, r2, cell, p, clock, st, &ix)) return rc;
    k_radius_search<CountVisitor><<<sg::cdiv(N, kWave), kWave, 0, st>>>(p.grid.spts, ix.sidx, ix.skey, p.grid.start, ix.g, N, r2,
                                                                       CountVisitor{p.count}, p.tally, counting);
    clock.tick();
    sgscan::exclusive_scan64(p.count, N, tsum, d_off, st);
    int64_t T = 0;
    sggrid::Misc hm{};
    Tally ht{};
    SG_HIP(hipMemcpyAsync(&T, d_off + N, 8, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&hm, p.grid.misc, sizeof(hm), hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&ht, p.tally, sizeof(ht), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    clock.tick();
    SG_LAUNCH_CHECK();
    if (T < 0 || T > (int64_t)N * (N - 1)) return sg::fail(SG_EINTERNAL, "%s: %lld pairs from %d points", who, (long long)T, N);
    *h_T = T;
    leave_stats(ix.g, hm, ht);
    if (T > SG_MAX_RADIUS_PAIRS)
        return sg::fail(SG_EUNSUP, "%s: %lld pairs; the lists hold at most %lld: %s", who, (long long)T, (long long)SG_MAX_RADIUS_PAIRS,
                        kPairsWayOut);
    if (T > capacity) return sg::fail(SG_ENOMEM, "%s: %lld pairs; the caller's lists hold %lld", who, (long long)T, (long long)capacity);
    if (T > 0) {
        k_radius_search<ListVisitor><<<sg::cdiv(N, kWave), kWave, 0, st>>>(p.grid.spts, ix.sidx, ix.skey, p.grid.start, ix.g, N, r2,
                                                                          ListVisitor{d_off, raw}, p.tally, 0);
        clock.tick();
        k_rn_rows<<<sg::cdiv(N, kRowBlock / 64), kRowBlock, 0, st>>>(d_off, raw, N, d_idx);
        clock.tick();
    }
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    return SG_OK;
}
}  // namespace sg

extern "C" {

size_t sg_radius_neighbours_ws_bytes(int N, int64_t capacity) {
    if (N < 1 || N > SG_MAX_GRID_POINTS || capacity < 0 || capacity > SG_MAX_RADIUS_PAIRS) return 0;
    return lists_ws_bytes(N, capacity);
}

int sg_radius_neighbours_grid(const float* d_points, int stride, int N, float radius, float cell, int64_t capacity, int64_t* d_off,
                              int32_t* d_idx, int64_t* h_T, void* d_ws, size_t ws_bytes, void* stream) {
    return sg::radius_lists("sg_radius_neighbours_grid", d_points, stride, N, radius, cell, capacity, d_off, d_idx, h_T, d_ws, ws_bytes, stream);
}

SG_STAGE_TIMER_API(radius_grid, t_ses.times, kStageNames)

int sg_radius_grid_stats(int64_t* h, int cap) {
    SG_REQUIRE(h && cap >= kNumStats, "sg_radius_grid_stats: room for %d words is needed", kNumStats);
    for (int i = 0; i < kNumStats; ++i) h[i] = t_ses.stats[i];
    return kNumStats;
}

size_t sg_radius_grid_ws_bytes(int N) {
    if (N < 1 || N > SG_MAX_GRID_POINTS) return 0;
    return sggrid::plan_bytes(N) + sg::align_up(sizeof(Tally)) + sg::align_up(sizeof(sgcc::Misc)) + 2 * sg::align_up((size_t)N * 4);
}

int sg_radius_count_grid(const float* d_points, int stride, int N, float radius, float cell, int32_t* d_count, void* d_ws, size_t ws_bytes,
                         void* stream) {
    const char* who = "sg_radius_count_grid";
    for (int i = 0; i < kNumStats; ++i) t_ses.stats[i] = 0;
    float r2 = 0.0f;
    if (const int rc = check_args(who, d_points, stride, N, radius, cell, d_count, d_ws, ws_bytes, &r2)) return rc;
    const Plan p = carve(d_ws, ws_bytes, N);
    if (!p.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_radius_grid_ws_bytes(N));
    hipStream_t st = sg::as_stream(stream);
    const int counting = t_ses.times.timing ? 1 : 0;
    sgos::StageClock<kStages> clock(st, t_ses.times.timing, t_ses.times.us);
    Index ix{};
    if (const int rc = build_index(who, d_points, stride, N, radius, r2, cell, p, clock, st, &ix)) return rc;
    clock.tick();                                // init: nothing to do
    k_radius_search<CountVisitor><<<sg::cdiv(N, kWave), kWave, 0, st>>>(p.grid.spts, ix.sidx, ix.skey, p.grid.start, ix.g, N, r2,
                                                                       CountVisitor{d_count}, p.tally, counting);
    clock.tick();
    sggrid::Misc hm{};
    Tally ht{};
    SG_HIP(hipMemcpyAsync(&hm, p.grid.misc, sizeof(hm), hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&ht, p.tally, sizeof(ht), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    clock.tick();
    SG_LAUNCH_CHECK();
    leave_stats(ix.g, hm, ht);
    return SG_OK;
}

int sg_components_radius(const float* d_points, int stride, int N, float radius, float cell, const int32_t* d_label, int32_t* d_comp,
                         int32_t* d_size, int* h_C, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_components_radius";
    for (int i = 0; i < kNumStats; ++i) t_ses.stats[i] = 0;
    SG_REQUIRE(h_C, "%s: a null pointer", who);
    *h_C = 0;
    float r2 = 0.0f;
    if (const int rc = check_args(who, d_points, stride, N, radius, cell, d_comp, d_ws, ws_bytes, &r2)) return rc;
    const Plan p = carve(d_ws, ws_bytes, N);
    if (!p.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_radius_grid_ws_bytes(N));
    hipStream_t st = sg::as_stream(stream);
    const int counting = t_ses.times.timing ? 1 : 0;
    sgos::StageClock<kStages> clock(st, t_ses.times.timing, t_ses.times.us);
    Index ix{};
    if (const int rc = build_index(who, d_points, stride, N, radius, r2, cell, p, clock, st, &ix)) return rc;
    const int nb = sg::cdiv(N, sgcc::kBlock);
    sgcc::k_cc_init<<<nb, sgcc::kBlock, 0, st>>>(p.parent, p.count, N, p.misc);
    clock.tick();
    k_radius_search<HookVisitor><<<sg::cdiv(N, kWave), kWave, 0, st>>>(p.grid.spts, ix.sidx, ix.skey, p.grid.start, ix.g, N, r2,
                                                                      HookVisitor{p.parent, d_label, p.misc, N}, p.tally, counting);
    clock.tick();
    sgcc::k_cc_flatten<<<nb, sgcc::kBlock, 0, st>>>(p.parent, N, d_comp, d_size ? p.count : nullptr, p.misc);
    if (d_size) sgcc::k_cc_sizes<<<nb, sgcc::kBlock, 0, st>>>(d_comp, p.count, N, d_size);
    sggrid::Misc hm{};
    sgcc::Misc hc{};
    Tally ht{};
    SG_HIP(hipMemcpyAsync(&hm, p.grid.misc, sizeof(hm), hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&hc, p.misc, sizeof(hc), hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&ht, p.tally, sizeof(ht), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    clock.tick();
    SG_LAUNCH_CHECK();
    if (hc.flag & sgcc::kFlagBudget) return sg::fail(SG_EINTERNAL, "%s: a chase ran out of its %d steps", who, 2 * N + 4);
    if (hc.roots < 1 || hc.roots > N) return sg::fail(SG_EINTERNAL, "%s: %d components from %d points", who, hc.roots, N);
    *h_C = hc.roots;
    leave_stats(ix.g, hm, ht);
    return SG_OK;
}

}  // extern "C"
