// The exact grid index that the grid kNN, the two-cloud nearest point (8i) and the radius graph (8k) share, and everything
// round it that does not depend on who searches:
//   kernels   the box and the finite check (overseg_device.h's box pieces), the cells on 8g's formula, the gather, the dense table, its stats
//   host      measure (box, read-back, finite check, extents and slack), check_cell (the refusals of a caller's cell edge), bin and
//             sort_cells (cells and the stable sort at one edge), finish_index (gather, table, stats), index_stats
//   device    the search skeleton: pending_lanes and pick_group (the wave's next cell), stage_tile (a sorted range through LDS),
//             wave_sum, search_epilogue
// The entry points decide the cell edge and drive the stages: "measure, choose the edge, index".  Every file that includes this gets its
// own copy of the kernels (internal linkage).
#pragma once
#include <cmath>
#include <cstring>

#include "sg_common.h"
#include "sort_device.h"
#include "cloud_knn_device.h"
#include "overseg_device.h"

namespace sggrid {
namespace {

using sgos::bits_for_cells;
using sgos::kCellLimit;

constexpr int kBlock = sgos::kBoxBlock;
constexpr int kWave = 64;                       // queries per block of the search: one wave
constexpr int kGTile = 256;                     // candidates staged per LDS tile of the search
constexpr int kMinCells = 1 << 22;              // the dense table holds max(2^22, 4 N) cells
constexpr int kTargetOccupancy = 48;            // points per occupied cell the library aims at
constexpr int kRingLimit = 8;
constexpr int kMaxRingLimit = 64;
constexpr float kShrink = 0.998046875f;         // 1 - 2^-9: swallows every rounding of the settled test
constexpr int kNumStats = 9;

struct Misc {
    unsigned long long evals;       // pair scores evaluated (timed calls only)
    int flag;                       // |= 1: a coordinate is not finite
    int nq;                         // queued queries
    int maxring;                    // the largest ring count of a settled query
    int heads;                      // occupied cells of the probe
    int occupied, maxcell;          // of the grid in use
    unsigned int m2;                // bits of max |p|^2 (non-negative: ascending as unsigned)
    unsigned int lo[3], hi[3];      // the bounding box as sgos::weight_key words
};

struct Grid {
    float lo[3];
    float h;
    int nc[3];
    int ncells;
    float delta, slack;
    int rmax;
};

__global__ void k_grid_init(Misc* __restrict__ m) {
    m->evals = 0ull;
    m->flag = 0; m->nq = 0; m->maxring = 0; m->heads = 0; m->occupied = 0; m->maxcell = 0; m->m2 = 0u;
    for (int a = 0; a < 3; ++a) { m->lo[a] = 0xffffffffu; m->hi[a] = 0u; }
}

// the box reduction of overseg_device.h with k_pc_pack's output: cand[i] = (x, y, z, |p|^2), and a seventh atomic per block for M2
__global__ __launch_bounds__(kBlock) void k_grid_box(const float* __restrict__ p, int stride, int N, float4* __restrict__ cand,
                                                     Misc* __restrict__ m) {
    __shared__ unsigned int s_lo[3][sgos::kBoxWaves], s_hi[3][sgos::kBoxWaves], s_m2[sgos::kBoxWaves];
    sgos::Box box;
    unsigned int m2 = 0u;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * kBlock) {
        const float c[3] = {p[i * stride], p[i * stride + 1], p[i * stride + 2]};
        sgos::box_take(box, c);
        const float4 v = sgcloud::with_norm(c[0], c[1], c[2]);
        cand[i] = v;
        m2 = max(m2, __float_as_uint(v.w));
    }
    sgos::box_stage(box, &m->flag, s_lo, s_hi);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m2 = max(m2, (unsigned int)__shfl_xor((int)m2, off));
    if ((threadIdx.x & 63) == 0) s_m2[threadIdx.x >> 6] = m2;
    __syncthreads();
    sgos::box_commit(s_lo, s_hi, m->lo, m->hi);
    if (threadIdx.x == 3) {
        unsigned int v = s_m2[0];
#pragma unroll
        for (int w = 1; w < sgos::kBoxWaves; ++w) v = max(v, s_m2[w]);
        atomicMax(&m->m2, v);
    }
}

// the cell of point i on 8g's formula; the host derived nc[] with the same operations from the box's maximum and the cell is monotone in
// the coordinate, so 0 <= f < nc -- the clamp never acts, it only keeps a table index in range whatever happens
__global__ __launch_bounds__(kBlock) void k_grid_cells(const float4* __restrict__ cand, int N, Grid g, unsigned long long* __restrict__ key,
                                                       int* __restrict__ idx) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float4 p = cand[i];
    const float q0 = (p.x - g.lo[0]) / g.h, q1 = (p.y - g.lo[1]) / g.h, q2 = (p.z - g.lo[2]) / g.h;
    const int c0 = min(max((int)__builtin_floorf(q0), 0), g.nc[0] - 1);
    const int c1 = min(max((int)__builtin_floorf(q1), 0), g.nc[1] - 1);
    const int c2 = min(max((int)__builtin_floorf(q2), 0), g.nc[2] - 1);
    key[i] = (unsigned long long)((c2 * g.nc[1] + c1) * g.nc[0] + c0);
    idx[i] = i;
}

// occupied cells = run heads of the sorted keys: one atomic per block
__global__ __launch_bounds__(kBlock) void k_grid_heads(const unsigned long long* __restrict__ skey, int N, int* __restrict__ heads) {
    __shared__ int part[kBlock / 64];
    const int s = blockIdx.x * kBlock + threadIdx.x;
    const bool head = s < N && (s == 0 || skey[s] != skey[s - 1]);
    const int n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(head));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += part[w];
        if (t) atomicAdd(heads, t);
    }
}

__global__ __launch_bounds__(kBlock) void k_grid_gather(const float4* __restrict__ cand, const int* __restrict__ sidx, int N,
                                                        float4* __restrict__ spts) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s < N) spts[s] = cand[sidx[s]];
}

// start[c] = the number of sorted keys below c, c = 0 .. ncells (start[ncells] = N)
__global__ __launch_bounds__(kBlock) void k_grid_table(const unsigned long long* __restrict__ skey, int N, int ncells, int* __restrict__ start) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c > ncells) return;
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < (unsigned long long)c) lo = mid + 1; else hi = mid;
    }
    start[c] = lo;
}

__global__ __launch_bounds__(kBlock) void k_grid_cellstats(const int* __restrict__ start, int ncells, Misc* __restrict__ m) {
    __shared__ int s_occ[kBlock / 64], s_max[kBlock / 64];
    const int c = blockIdx.x * kBlock + threadIdx.x;
    int n = c < ncells ? start[c + 1] - start[c] : 0;
    const int occ = __builtin_popcountll(__builtin_amdgcn_ballot_w64(n > 0));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n = max(n, __shfl_xor(n, off));
    if ((threadIdx.x & 63) == 0) { s_occ[threadIdx.x >> 6] = occ; s_max[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0, mx = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) { t += s_occ[w]; mx = max(mx, s_max[w]); }
        if (t) { atomicAdd(&m->occupied, t); atomicMax(&m->maxcell, mx); }
    }
}

// ---- the search skeleton: one wave per 64 queries in the order of their cell keys ----

// The wave's next group: the lanes of the first pending lane's cell, and that cell's coordinates (wave-uniform).  A search loops
//     while (const unsigned long long pending = pending_lanes(done)) { const Group grp = pick_group(g, pending, done, mycell); ... }
// The group is returned by value and picked in one place of the loop: outputs through references cost the self-kNN's search at 21 entries its occupancy, a
// second inlined copy a hundred instructions (profiles/grid_builder_resources.md).
struct Group {
    bool in;                        // this lane belongs to the group
    int x, y, z;
};

__device__ __forceinline__ unsigned long long pending_lanes(bool done) { return __builtin_amdgcn_ballot_w64(!done); }

__device__ __forceinline__ Group pick_group(const Grid& g, unsigned long long pending, bool done, int mycell) {
    const int leader = __builtin_ctzll(pending);
    const int gcell = __builtin_amdgcn_readfirstlane(__shfl(mycell, leader));
    const int nx = g.nc[0], ny = g.nc[1];
    return Group{!done && mycell == gcell, gcell % nx, (gcell / nx) % ny, gcell / (nx * ny)};
}

// The sorted points [c0, min(c0 + kGTile, b)) into tile / tidx (float4 + original index) -> their number.  c0 and b are wave-uniform, so
// every lane of the block (one wave) reaches both barriers: the first keeps the previous tile's readers apart from these stores, the
// second the stores from the readers that follow.
__device__ __forceinline__ int stage_tile(int c0, int b, const float4* __restrict__ spts, const int* __restrict__ sidx, float4* tile, int* tidx) {
    const int lane = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kGTile / kWave; ++u) {
        const int e = c0 + u * kWave + lane;
        if (e < b) { tile[u * kWave + lane] = spts[e]; tidx[u * kWave + lane] = sidx[e]; }
    }
    __syncthreads();
    return min(kGTile, b - c0);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// a ring search's leave: the wave's largest ring count of a settled query, and (timed calls) its pair scores
__device__ __forceinline__ void search_epilogue(int myr, unsigned int evals, int counting, Misc* __restrict__ m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) myr = max(myr, __shfl_xor(myr, off));
    if (threadIdx.x == 0 && myr > 0) atomicMax(&m->maxring, myr);
    if (counting) {
        const unsigned long long e = wave_sum(evals);
        if (threadIdx.x == 0) atomicAdd(&m->evals, e);
    }
}

// ---- the host side ----

long long cell_cap(int N) { return std::max<long long>(kMinCells, 4ll * N); }

struct Plan {
    Misc* misc;
    float4 *cand, *spts;            // [N] original order, sorted order
    unsigned long long *k0, *k1;
    int *v0, *v1;
    int* hist;
    int* start;                     // [cell_cap + 1]
    int* queue;                     // [N]
    bool ok;
};

void carve(sg::Carver& cv, Plan& p, int N) {
    const size_t n = (size_t)std::max(N, 1);
    p.misc = cv.take<Misc>(1);
    p.cand = cv.take<float4>(n);
    p.spts = cv.take<float4>(n);
    p.k0 = cv.take<unsigned long long>(n);
    p.k1 = cv.take<unsigned long long>(n);
    p.v0 = cv.take<int>(n);
    p.v1 = cv.take<int>(n);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    p.start = cv.take<int>((size_t)cell_cap(N) + 1);
    p.queue = cv.take<int>(n);
    p.ok = cv.ok;
}

Plan carve(void* d_ws, size_t ws_bytes, int N) {
    Plan p{};
    sg::Carver cv(d_ws, ws_bytes);
    carve(cv, p, N);
    return p;
}

size_t plan_bytes(int N) {
    const size_t n = (size_t)N;
    return sg::align_up(sizeof(Misc)) + 2 * sg::align_up(n * 16) + 2 * sg::align_up(n * 8) + 3 * sg::align_up(n * 4) +
           sg::align_up(sgsort::hist_ints((long long)n) * 4) + sg::align_up(((size_t)cell_cap(N) + 1) * 4);
}

// the cells per axis of edge h, in the device's arithmetic (the cell of the box's maximum + 1); false: an axis reaches 2^21 cells
bool cells_of(const float ext[3], float h, int nc[3], long long* total) {
    *total = 1;
    for (int a = 0; a < 3; ++a) {
        const float q = ext[a] / h;
        if (!(q < kCellLimit)) return false;
        nc[a] = (int)std::floor(q) + 1;
        *total *= nc[a];
    }
    return true;
}

struct Measured {
    Misc hm;                        // as the box left it
    float ext[3], emax;             // the box's extents and the largest of them, E
};

struct Sorted {
    const unsigned long long* key;
    const int* idx;
};

struct Index {
    Grid g;
    const unsigned long long* skey;     // the candidates' sorted keys
    const int* sidx;                    // and their original indices
};

// The stage "box" over the N candidates of `d_points`: the finite check, p.cand, the bounding box and M2.  With queries (d_q, U > 0)
// they run over the UNION of the two clouds and q_pts receives the queries' (x, y, z, |q|^2).  Synchronises the stream once.
// -> a fresh g with lo and slack; the caller chooses h and the rings.
int measure(const char* who, const float* d_points, int stride, int N, const float* d_q, int qstride, int U, float4* q_pts, const Plan& p,
            hipStream_t st, Grid* g, Measured* out) {
    k_grid_init<<<1, 1, 0, st>>>(p.misc);
    k_grid_box<<<std::min(sg::cdiv(N, kBlock), sgos::kBoxBlocks), kBlock, 0, st>>>(d_points, stride, N, p.cand, p.misc);
    if (U > 0) k_grid_box<<<std::min(sg::cdiv(U, kBlock), sgos::kBoxBlocks), kBlock, 0, st>>>(d_q, qstride, U, q_pts, p.misc);
    out->hm = Misc{};
    SG_HIP(hipMemcpyAsync(&out->hm, p.misc, sizeof(Misc), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (out->hm.flag & 1) return sg::fail(SG_EINVAL, "%s: a coordinate is not finite", who);
    *g = Grid{};
    out->emax = 0.0f;
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = sgos::unkey_host(out->hm.lo[a]);
        out->ext[a] = sgos::unkey_host(out->hm.hi[a]) - g->lo[a];
        out->emax = std::max(out->emax, out->ext[a]);
    }
    g->slack = std::ldexp(out->emax, -21);              // 8 u E, u = 2^-24
    return SG_OK;
}

// a cell edge the caller chose: g.nc and the number of cells, or the refusal
int check_cell(const char* who, const Measured& ms, float cell, int N, Grid* g, long long* total) {
    if (!cells_of(ms.ext, cell, g->nc, total))
        return sg::fail(SG_EUNSUP, "%s: cell too small for the cloud's extent (%g / %g is not below %g cells on an axis)", who, (double)ms.emax,
                        (double)cell, (double)kCellLimit);
    if (*total > cell_cap(N))
        return sg::fail(SG_EUNSUP, "%s: a cell of %g gives %lld cells; the table of %d points holds %lld", who, (double)cell, *total, N,
                        cell_cap(N));
    return SG_OK;
}

// the cells at edge h (one that cells_of accepts): g.h, g.nc, g.ncells, and p.k0 / p.v0 = every candidate's key and index
void bin(const Measured& ms, float h, const Plan& p, int N, hipStream_t st, Grid* g) {
    long long total = 0;
    g->h = h;
    cells_of(ms.ext, h, g->nc, &total);
    g->ncells = (int)total;
    k_grid_cells<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(p.cand, N, *g, p.k0, p.v0);
}

// (key, index) of n points, stable by key over the bits a table of ncells uses -> where the sorted lists are
Sorted sort_cells(unsigned long long* k0, unsigned long long* k1, int* v0, int* v1, int* hist, int n, int ncells, hipStream_t st) {
    auto L = sgsort::one_list<unsigned long long, int>(k0, k1, v0, v1, hist, n);
    sgsort::radix_sort<unsigned long long, int, true>(L, 1, 0, bits_for_cells(ncells), st);
    return Sorted{L.kin[0], L.vin[0]};
}

// the rest of the stage "sort" (the points in sorted order) and the stage "table"
template <class Clock>
void finish_index(const Plan& p, const Sorted& s, int N, Clock& clock, hipStream_t st, Index* ix) {
    const Grid& g = ix->g;
    ix->skey = s.key;
    ix->sidx = s.idx;
    k_grid_gather<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(p.cand, s.idx, N, p.spts);
    clock.tick();
    k_grid_table<<<sg::cdiv((long long)g.ncells + 1, kBlock), kBlock, 0, st>>>(s.key, N, g.ncells, p.start);
    k_grid_cellstats<<<sg::cdiv(g.ncells, kBlock), kBlock, 0, st>>>(p.start, g.ncells, p.misc);
    clock.tick();
}

// the stats words every grid entry starts with: nc[0..2], occupied cells, the largest cell, the bits of h
void index_stats(int64_t* s, const Grid& g, const Misc& hm) {
    unsigned int hbits;
    std::memcpy(&hbits, &g.h, 4);
    s[0] = g.nc[0]; s[1] = g.nc[1]; s[2] = g.nc[2];
    s[3] = hm.occupied; s[4] = hm.maxcell; s[5] = (int64_t)hbits;
}

}  // namespace
}  // namespace sggrid
