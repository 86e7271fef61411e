// The exact grid index that the grid kNN, the two-cloud nearest point (8i) and the radius graph (8k) share: the box and the
// finite check, the cells on 8g's formula, the sorted order, the dense table.  Every file that includes this gets its own copy of the
// kernels (internal linkage); the entry points decide the cell edge and drive the stages.
#pragma once
#include <cmath>
#include <cstring>

#include "sg_common.h"
#include "sort_device.h"
#include "cloud_knn_device.h"
#include "overseg_device.h"

namespace sggrid {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;                       // queries per block of the search: one wave
constexpr int kGTile = 256;                     // candidates staged per LDS tile of the search
constexpr int kBoxBlocks = 1024;
constexpr float kCellLimit = 2097152.0f;        // 2^21 cells per axis, as in 8g
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

inline float unkey_host(unsigned int k) {
    const unsigned int b = k & 0x80000000u ? k ^ 0x80000000u : ~k;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

__global__ void k_grid_init(Misc* __restrict__ m) {
    m->evals = 0ull;
    m->flag = 0; m->nq = 0; m->maxring = 0; m->heads = 0; m->occupied = 0; m->maxcell = 0; m->m2 = 0u;
    for (int a = 0; a < 3; ++a) { m->lo[a] = 0xffffffffu; m->hi[a] = 0u; }
}

// k_thin_box's shape (a fixed number of blocks, 7 atomics per block) with k_pc_pack's output
__global__ __launch_bounds__(kBlock) void k_grid_box(const float* __restrict__ p, int stride, int N, float4* __restrict__ cand,
                                                     Misc* __restrict__ m) {
    __shared__ unsigned int s_lo[3][kBlock / 64], s_hi[3][kBlock / 64], s_m2[kBlock / 64];
    unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, m2 = 0u;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * kBlock) {
        float c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = p[i * stride + a];
            bad |= !sgos::finite_f32(c[a]);
            const unsigned int key = sgos::weight_key(c[a]);
            lo[a] = min(lo[a], key);
            hi[a] = max(hi[a], key);
        }
        const float4 v = sgcloud::with_norm(c[0], c[1], c[2]);
        cand[i] = v;
        m2 = max(m2, __float_as_uint(v.w));
    }
    if (bad) atomicOr(&m->flag, 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], (unsigned int)__shfl_xor((int)lo[a], off));
            hi[a] = max(hi[a], (unsigned int)__shfl_xor((int)hi[a], off));
        }
        m2 = max(m2, (unsigned int)__shfl_xor((int)m2, off));
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_lo[a][wave] = lo[a]; s_hi[a][wave] = hi[a]; }
        s_m2[wave] = m2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        unsigned int l = s_lo[a][0], h = s_hi[a][0];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) { l = min(l, s_lo[a][w]); h = max(h, s_hi[a][w]); }
        atomicMin(&m->lo[a], l);
        atomicMax(&m->hi[a], h);
    } else if (threadIdx.x == 3) {
        unsigned int v = s_m2[0];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) v = max(v, s_m2[w]);
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

int bits_for_cells(long long cells) {           // bits that hold 0..cells-1; none for one cell
    int b = 0;
    while (b < 62 && (1ll << b) < cells) ++b;
    return b;
}

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

}  // namespace
}  // namespace sggrid
