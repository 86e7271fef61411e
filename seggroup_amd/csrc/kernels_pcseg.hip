// Point-cloud over-segmentation, device side: the twin of kernels_overseg.hip for a scan that has no faces.  The graph is
// the kNN graph of the cloud, the normals come from the neighbourhoods' covariance; the edge order and the host chain are 8d's.
//
//   k_pc_pack           coordinates finite (one flag word), (x, y, z, |p|^2) per point, the cloud's bounding box (order-free min / max)
//   k_pc_knn            the complete top-(k+1) list of every point against the whole cloud: cloud_knn_device.h, the score and the tie
//                       rule of sg_pointcloud_adjacency's k_nearest_k; with index = SG_KNN_GRID the same table comes from the exact grid
//                       index instead (kernels_knn_grid.hip) and every later stage is unchanged
//   k_pc_normals        one thread per point: mean and the six covariance sums over its list in list order, a cyclic Jacobi iteration
//                       with the rotations written out for the pairs (0,1), (0,2), (1,2) on scalars (nothing is indexed at run time),
//                       the eigenvector of the smallest eigenvalue, turned towards the viewpoint
//   edges               (i, L[i][t]), t = 1..k, without the self pairs, as sorted unique pair keys: a < b in lexicographic order
//   k_pc_weights        8d's weight after the two normals have been aligned (the viewpoint test may have fallen either way)
//   sort + gather       8d's, the same code (overseg_device.h)
//   radius graph        DESIGN.md 8l, sg_pcseg_edges_radius: the lists of sg_radius_neighbours_grid in place of the kNN table; k_pc_normals_csr
//                       (neighbourhoods of variable length, the same Jacobi code: pcseg_normals_device.h), the upper halves of the rows as the
//                       lexicographic edge list (k_pc_upper_counts, scan64_device.h, k_pc_edges_csr); weights, sort and gather as above
//
// Every fp32 operation is written op by op and rounded once (-ffp-contract=off; only + - * / sqrt and comparisons, the explicit FMAs of
// pair_score aside), which tests/test_gpu_pcseg.py holds to the NumPy statement of the specification (tests/pcseg_ref.py) bit for bit.
#include <cmath>

#include "sg_common.h"
#include "sort_device.h"
#include "cloud_knn_device.h"
#include "overseg_device.h"
#include "pcseg_normals_device.h"
#include "scan64_device.h"

namespace {

constexpr int kBlock = 256;
using sgpc::kSweeps;
using sgcloud::kTile;

struct Misc {
    int flag;                       // |= 1: a coordinate is not finite; |= 2: a list has an unfilled entry (scores not finite); |= 4: a
                                    // caller's list names a point outside 0..N-1; |= 8: the offsets of a caller's rows do not ascend from 0
    int count;                      // unique pair keys
    unsigned int lo[3], hi[3];      // the bounding box as sgos::weight_key words
    float view[3];
};

__device__ __forceinline__ float unkey(unsigned int k) { return __uint_as_float(k & 0x80000000u ? k ^ 0x80000000u : ~k); }

__global__ void k_pc_init(Misc* __restrict__ m, int has_view, float vx, float vy, float vz) {
    m->flag = 0;
    m->count = 0;
    for (int a = 0; a < 3; ++a) { m->lo[a] = 0xffffffffu; m->hi[a] = 0u; }
    m->view[0] = has_view ? vx : 0.0f; m->view[1] = has_view ? vy : 0.0f; m->view[2] = has_view ? vz : 0.0f;
}

__global__ __launch_bounds__(kBlock) void k_pc_pack(const float* __restrict__ p, int stride, int N, float4* __restrict__ cand,
                                                    Misc* __restrict__ m) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < N;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = p[(size_t)i * stride + a];
        cand[i] = sgcloud::with_norm(c[0], c[1], c[2]);
        if (!(sgos::finite_f32(c[0]) && sgos::finite_f32(c[1]) && sgos::finite_f32(c[2]))) atomicOr(&m->flag, 1);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        unsigned int lo = live ? sgos::weight_key(c[a]) : 0xffffffffu, hi = live ? lo : 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo = min(lo, (unsigned int)__shfl_xor((int)lo, off));
            hi = max(hi, (unsigned int)__shfl_xor((int)hi, off));
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&m->lo[a], lo); atomicMax(&m->hi[a], hi); }
    }
}

// the default viewpoint: the centre of the bounding box, (min + max) * 0.5 per axis
__global__ void k_pc_view(Misc* __restrict__ m) {
    for (int a = 0; a < 3; ++a) m->view[a] = (unkey(m->lo[a]) + unkey(m->hi[a])) * 0.5f;
}

template <int KK>
__global__ __launch_bounds__(kTile) void k_pc_knn(const float4* __restrict__ cand, int N, int32_t* __restrict__ table, Misc* __restrict__ m) {
    __shared__ float4 tile[kTile];
    const int u = blockIdx.x * kTile + threadIdx.x;
    const bool live = u < N;
    const float4 me = cand[live ? u : 0];
    float bs[KK];
    int bi[KK];
    sgcloud::top_scores<KK>(cand, N, me, tile, bs, bi);
    if (!live) return;
    bool unfilled = false;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        unfilled |= bi[t] >= N;                                // fewer than KK finite scores: the coordinates overflow the score
        table[(size_t)u * KK + t] = bi[t] < N ? bi[t] : u;     // nothing downstream reads through an index that is not a point
    }
    if (unfilled) atomicOr(&m->flag, 2);
}

// p: rows of `stride` floats, xyz first.  table [N,KK]: every point's list; an entry outside 0..N-1 (a caller's table) raises flag 4 and
// counts as the point itself.
template <int KK>
__global__ __launch_bounds__(kBlock) void k_pc_normals(const float* __restrict__ p, int stride, int N, const int32_t* __restrict__ table,
                                                       Misc* __restrict__ m, float* __restrict__ nrm) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int32_t* L = table + (size_t)i * KK;
    // 2. the mean: the sum in list order from +0, divided by (float)(k + 1)
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    bool bad = false;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        int j = L[t];
        if ((unsigned)j >= (unsigned)N) { bad = true; j = i; }
        sx = sx + p[(size_t)j * stride]; sy = sy + p[(size_t)j * stride + 1]; sz = sz + p[(size_t)j * stride + 2];
    }
    if (bad) atomicOr(&m->flag, 4);
    const float kk = (float)KK;
    const float mx = sx / kk, my = sy / kk, mz = sz / kk;
    // 3. the six covariance sums in list order from +0, not normalised
    float a00 = 0.0f, a01 = 0.0f, a02 = 0.0f, a11 = 0.0f, a12 = 0.0f, a22 = 0.0f;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        int j = L[t];
        if ((unsigned)j >= (unsigned)N) j = i;
        const float qx = p[(size_t)j * stride] - mx, qy = p[(size_t)j * stride + 1] - my, qz = p[(size_t)j * stride + 2] - mz;
        a00 = a00 + qx * qx; a01 = a01 + qx * qy; a02 = a02 + qx * qz;
        a11 = a11 + qy * qy; a12 = a12 + qy * qz; a22 = a22 + qz * qz;
    }
    // 4. cyclic Jacobi and the column of the smallest diagonal entry (pcseg_normals_device.h)
    float nx, ny, nz;
    sgpc::smallest_eigenvector(a00, a01, a02, a11, a12, a22, nx, ny, nz);
    // 5. towards the viewpoint
    const float dx = m->view[0] - p[(size_t)i * stride], dy = m->view[1] - p[(size_t)i * stride + 1], dz = m->view[2] - p[(size_t)i * stride + 2];
    const float s = (nx * dx + ny * dy) + nz * dz;
    if (s < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    nrm[(size_t)i * 3] = nx; nrm[(size_t)i * 3 + 1] = ny; nrm[(size_t)i * 3 + 2] = nz;
}


// The normals over neighbourhoods of variable length: the neighbourhood of i is i itself, then its row
// idx[off[i] .. off[i+1]) in stored order.  One thread per point, two passes over the row, every point gathered as the packed 16-byte
// record of k_pc_pack; the sums are sequential by the statement.  The table is checked here: a row outside 0 <= lo <= hi <= off[N] (or
// off[0] != 0) raises flag 8 and counts as empty, an entry outside 0..N-1 raises flag 4 and counts as the point itself -- nothing is
// read through either.
__global__ __launch_bounds__(kBlock) void k_pc_normals_csr(const float4* __restrict__ cand, int N, const int64_t* __restrict__ off,
                                                           const int32_t* __restrict__ idx, Misc* __restrict__ m, float* __restrict__ nrm) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t T = off[N];
    int64_t lo = off[i], hi = off[i + 1];
    if (!(lo >= 0 && lo <= hi && hi <= T) || (i == 0 && lo != 0)) { atomicOr(&m->flag, 8); lo = 0; hi = 0; }
    const float4 me = cand[i];
    // the mean: the sum in neighbourhood order from +0, divided by (float)m
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    sx = sx + me.x; sy = sy + me.y; sz = sz + me.z;
    bool bad = false;
    for (int64_t e = lo; e < hi; ++e) {
        int j = idx[e];
        if ((unsigned)j >= (unsigned)N) { bad = true; j = i; }
        const float4 q = cand[j];
        sx = sx + q.x; sy = sy + q.y; sz = sz + q.z;
    }
    if (bad) atomicOr(&m->flag, 4);
    const float mm = (float)(hi - lo + 1);
    const float mx = sx / mm, my = sy / mm, mz = sz / mm;
    // the six covariance sums in the same order from +0, not normalised
    float a00 = 0.0f, a01 = 0.0f, a02 = 0.0f, a11 = 0.0f, a12 = 0.0f, a22 = 0.0f;
    {
        const float qx = me.x - mx, qy = me.y - my, qz = me.z - mz;
        a00 = a00 + qx * qx; a01 = a01 + qx * qy; a02 = a02 + qx * qz;
        a11 = a11 + qy * qy; a12 = a12 + qy * qz; a22 = a22 + qz * qz;
    }
    for (int64_t e = lo; e < hi; ++e) {
        int j = idx[e];
        if ((unsigned)j >= (unsigned)N) j = i;
        const float4 q = cand[j];
        const float qx = q.x - mx, qy = q.y - my, qz = q.z - mz;
        a00 = a00 + qx * qx; a01 = a01 + qx * qy; a02 = a02 + qx * qz;
        a11 = a11 + qy * qy; a12 = a12 + qy * qz; a22 = a22 + qz * qz;
    }
    float nx, ny, nz;
    sgpc::smallest_eigenvector(a00, a01, a02, a11, a12, a22, nx, ny, nz);
    // towards the viewpoint
    const float dx = m->view[0] - me.x, dy = m->view[1] - me.y, dz = m->view[2] - me.z;
    const float s = (nx * dx + ny * dy) + nz * dz;
    if (s < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    nrm[(size_t)i * 3] = nx; nrm[(size_t)i * 3 + 1] = ny; nrm[(size_t)i * 3 + 2] = nz;
}

// where the upper half of row i begins: the first entry above i of a row in ascending index (the library's own rows)
__device__ __forceinline__ int64_t upper_begin(const int32_t* __restrict__ idx, int64_t lo, int64_t hi, int i) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// up[i] = the entries of row i above i
__global__ __launch_bounds__(kBlock) void k_pc_upper_counts(const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int N,
                                                            int32_t* __restrict__ up) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t hi = off[i + 1];
    up[i] = (int32_t)(hi - upper_begin(idx, off[i], hi, i));
}

// the pairs a < b in lexicographic order: one wave per row copies the row's upper half to adj [E,2] at eoff[i]; E: the room of adj
__global__ __launch_bounds__(kBlock) void k_pc_edges_csr(const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int N,
                                                         const int64_t* __restrict__ eoff, int64_t E, int64_t* __restrict__ adj) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const int64_t hi = off[i + 1];
    const int64_t from = upper_begin(idx, off[i], hi, i);
    const int64_t dst = eoff[i];
    for (int64_t t = lane; t < hi - from; t += 64) {
        if (dst + t >= E) break;
        adj[(size_t)(dst + t) * 2] = (int64_t)i;
        adj[(size_t)(dst + t) * 2 + 1] = (int64_t)idx[from + t];
    }
}

// 6. pair key of (i, L[i][t]), t = 1..k, at i * k + t - 1: lo << 32 | hi; a self pair (coincident points) becomes ~0 and sorts to the end
__global__ __launch_bounds__(kBlock) void k_pc_edge_keys(const int32_t* __restrict__ table, int N, int k, unsigned long long* __restrict__ keys) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (size_t)N * k) return;
    const int i = (int)(e / (unsigned)k), t = (int)(e % (unsigned)k) + 1;
    const int j = table[(size_t)i * (k + 1) + t];
    keys[e] = j == i ? ~0ull : ((unsigned long long)(unsigned)min(i, j) << 32) | (unsigned)max(i, j);
}

__global__ __launch_bounds__(kBlock) void k_pc_unpack(const unsigned long long* __restrict__ keys, int n, int64_t* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[(size_t)i * 2] = (int64_t)(keys[i] >> 32);
    out[(size_t)i * 2 + 1] = (int64_t)(keys[i] & 0xffffffffull);
}

// 7. weight and sort key of edge e = (a, b) of the lexicographic list; idx[e] = e
__global__ __launch_bounds__(kBlock) void k_pc_weights(const int64_t* __restrict__ adj, int E, const float4* __restrict__ cand,
                                                       const float* __restrict__ vn, float* __restrict__ w_out,
                                                       unsigned int* __restrict__ key, int* __restrict__ idx) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const size_t a = (size_t)adj[(size_t)e * 2], b = (size_t)adj[(size_t)e * 2 + 1];
    const float nax = vn[a * 3], nay = vn[a * 3 + 1], naz = vn[a * 3 + 2];
    const float nbx = vn[b * 3], nby = vn[b * 3 + 1], nbz = vn[b * 3 + 2];
    float d = (nax * nbx + nay * nby) + naz * nbz;
    const float4 pa = cand[a], pb = cand[b];
    const float dx = pb.x - pa.x, dy = pb.y - pa.y, dz = pb.z - pa.z;
    float c = (nbx * dx + nby * dy) + nbz * dz;
    if (d < 0.0f) { d = -d; c = -c; }                                     // the same surface seen from the other side
    float w = 1.0f - d;
    if (c > 0.0f) w = w * w;
    w_out[e] = w;
    key[e] = sgos::weight_key(w);
    idx[e] = e;
}

int bits_for(long long n) {
    int b = 1;
    while ((1ll << b) < n) ++b;
    return b;
}

struct Plan {                       // the workspace of one cloud; n = N * k
    size_t n;
    float4* cand;                   // [N]
    Misc* misc;
    int32_t* knn;                   // [N, k+1]
    unsigned long long *p0, *p1, *p2;       // pair keys
    int* hist;
    int* scratch;
    int64_t* adj;                   // [n,2] the lexicographic list
    float* w;                       // [E] weights in that order
    unsigned int *k0, *k1;          // weight keys
    int *v0, *v1;                   // edge indices
    // outputs of sg_pcseg_scan, which has no caller's buffers for them
    float* vn;
    int32_t* edges;
    float* w_sorted;
    char* grid;                     // sg_pointcloud_knn_grid's workspace (index = SG_KNN_GRID only)
    size_t grid_bytes;
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, int N, int k, int index) {
    Plan p{};
    p.n = (size_t)std::max(N, 1) * std::max(k, 1);
    const size_t np = (size_t)std::max(N, 1);
    sg::Carver cv(d_ws, ws_bytes);
    p.cand = cv.take<float4>(np);
    p.misc = cv.take<Misc>(1);
    p.knn = cv.take<int32_t>(np * (std::max(k, 1) + 1));
    p.p0 = cv.take<unsigned long long>(p.n);
    p.p1 = cv.take<unsigned long long>(p.n);
    p.p2 = cv.take<unsigned long long>(p.n);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)p.n));
    p.scratch = cv.take<int>(sgsort::unique_ints((long long)p.n));
    p.adj = cv.take<int64_t>(p.n * 2);
    p.w = cv.take<float>(p.n);
    p.k0 = cv.take<unsigned int>(p.n);
    p.k1 = cv.take<unsigned int>(p.n);
    p.v0 = cv.take<int>(p.n);
    p.v1 = cv.take<int>(p.n);
    p.vn = cv.take<float>(np * 3);
    p.edges = cv.take<int32_t>(p.n * 2);
    p.w_sorted = cv.take<float>(p.n);
    if (index == SG_KNN_GRID) {
        p.grid_bytes = sg_pointcloud_knn_grid_ws_bytes(N, k);
        p.grid = cv.take<char>(p.grid_bytes);
    }
    p.ok = cv.ok;
    return p;
}

// index: SG_KNN_BRUTE scores every pair (k_pc_knn), SG_KNN_GRID takes the lists from the grid (kernels_knn_grid.hip)
int check_k(const char* who, int N, int k, int index = SG_KNN_BRUTE) {
    if (index != SG_KNN_BRUTE && index != SG_KNN_GRID) return sg::fail(SG_EINVAL, "%s: index = %d (SG_KNN_BRUTE or SG_KNN_GRID)", who, index);
    const int cap = index == SG_KNN_GRID ? SG_MAX_GRID_POINTS : SG_MAX_POINTS;
    if (k != 5 && k != 10 && k != 20) return sg::fail(SG_EUNSUP, "%s: k = %d is not built (5, 10 = the reference's default, 20)", who, k);
    if (N <= k) return sg::fail(SG_EINVAL, "%s: %d points for k = %d (topk(k + 1) raises in the reference)", who, N, k);
    if (N > cap) return sg::fail(SG_EUNSUP, "%s: %d points; a cloud holds at most %d", who, N, cap);
    return SG_OK;
}

void launch_knn(const float4* cand, int N, int k, int32_t* table, Misc* m, hipStream_t st) {
    if (k == 5) k_pc_knn<6><<<sg::cdiv(N, kTile), kTile, 0, st>>>(cand, N, table, m);
    else if (k == 10) k_pc_knn<11><<<sg::cdiv(N, kTile), kTile, 0, st>>>(cand, N, table, m);
    else k_pc_knn<21><<<sg::cdiv(N, kTile), kTile, 0, st>>>(cand, N, table, m);
}

void launch_normals(const float* p, int stride, int N, int k, const int32_t* table, Misc* m, float* nrm, hipStream_t st) {
    if (k == 5) k_pc_normals<6><<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(p, stride, N, table, m, nrm);
    else if (k == 10) k_pc_normals<11><<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(p, stride, N, table, m, nrm);
    else k_pc_normals<21><<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(p, stride, N, table, m, nrm);
}

int viewpoint_ok(const char* who, const float* v) {
    if (v && !(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))) return sg::fail(SG_EINVAL, "%s: the viewpoint is not finite", who);
    return SG_OK;
}

// sg_pcseg_set_timing(1): the calling thread's next sg_pcseg_edges calls bracket their stages with events (tools/time_pcseg.py)
constexpr int kStages = 7;
const char* const kStageNames[kStages] = {"check", "knn", "normals", "edges", "weights", "weight_sort", "gather"};
thread_local sgos::StageTimes<kStages> t_times;


size_t pcseg_ws_bytes(int N, int k, int index) {
    const size_t np = (size_t)std::max(N, 1), kk = (size_t)std::max(k, 1), n = np * kk;
    return sg::align_up(np * 16) + sg::align_up(sizeof(Misc)) + sg::align_up(np * (kk + 1) * 4) + 3 * sg::align_up(n * 8) +
           sg::align_up(sgsort::hist_ints((long long)n) * 4) + sg::align_up(sgsort::unique_ints((long long)n) * 4) + sg::align_up(n * 16) +
           5 * sg::align_up(n * 4) + sg::align_up(np * 12) + sg::align_up(n * 8) + sg::align_up(n * 4) +
           (index == SG_KNN_GRID ? sg::align_up(sg_pointcloud_knn_grid_ws_bytes(N, k)) : 0);
}

// sg_pcseg_edges and its indexed twin: only stage 1, the lists, knows the index
int pcseg_edges(const char* who, const float* d_xyz, int N, int k, const float* h_viewpoint, int index, float cell, int32_t* d_knn,
                float* d_normals, int32_t* d_edges, float* d_w, int* h_E, void* d_ws, size_t ws_bytes, void* stream) {
    if (!(N > 0 && d_xyz && d_normals && d_edges && d_w && h_E && d_ws)) return sg::fail(SG_EINVAL, "%s: bad arguments", who);
    *h_E = 0;
    int rc = check_k(who, N, k, index);
    if (rc < 0) return rc;
    if ((rc = viewpoint_ok(who, h_viewpoint)) < 0) return rc;
    const Plan p = carve(d_ws, ws_bytes, N, k, index);
    if (!p.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, pcseg_ws_bytes(N, k, index));
    hipStream_t st = sg::as_stream(stream);
    const int n = N * k;                                                       // N <= 2^24, k <= 20: below 2^31
    sgos::StageClock<kStages> clock(st, t_times.timing, t_times.us);
    // 0. the coordinates are the caller's
    k_pc_init<<<1, 1, 0, st>>>(p.misc, h_viewpoint != nullptr, h_viewpoint ? h_viewpoint[0] : 0.0f, h_viewpoint ? h_viewpoint[1] : 0.0f,
                               h_viewpoint ? h_viewpoint[2] : 0.0f);
    k_pc_pack<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_xyz, 3, N, p.cand, p.misc);
    int flag = 0;
    SG_HIP(hipMemcpyAsync(&flag, &p.misc->flag, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (flag & 1) return sg::fail(SG_EINVAL, "%s: a coordinate is not finite", who);
    clock.tick();
    // 1. the lists
    int32_t* table = d_knn ? d_knn : p.knn;
    if (index == SG_KNN_GRID) {
        if ((rc = sg_pointcloud_knn_grid(d_xyz, 3, N, k, cell, table, p.grid, p.grid_bytes, stream)) < 0) return rc;
    } else {
        launch_knn(p.cand, N, k, table, p.misc, st);
    }
    clock.tick();
    // 2-5. normals
    if (!h_viewpoint) k_pc_view<<<1, 1, 0, st>>>(p.misc);
    launch_normals(reinterpret_cast<const float*>(p.cand), 4, N, k, table, p.misc, d_normals, st);
    clock.tick();
    // 6. the unique undirected pairs a < b in lexicographic order
    k_pc_edge_keys<<<sg::cdiv(n, kBlock), kBlock, 0, st>>>(table, N, k, p.p0);
    auto L = sgsort::one_list<unsigned long long, int>(p.p0, p.p1, nullptr, nullptr, p.hist, n);
    const int field = std::min(32, bits_for((long long)N + 1) + 1);           // one bit more than an id carries: ~0 must come out last
    sgsort::radix_sort<unsigned long long, int, false>(L, 1, 0, field, st);
    sgsort::radix_sort<unsigned long long, int, false>(L, 1, 32, field, st);
    unsigned long long* uniq = p.p2;
    sgsort::unique_sorted<unsigned long long>(L.kin[0], n, uniq, nullptr, &p.misc->count, p.scratch, st);
    int fc[2] = {0, 0};
    SG_HIP(hipMemcpyAsync(fc, p.misc, 8, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (fc[0] & 2) return sg::fail(SG_EINVAL, "%s: the coordinates are too large for the fp32 pair score", who);
    int E = fc[1];
    if (E < 1 || E > n) return sg::fail(SG_EHIP, "%s: %d pair keys from %d points", who, E, N);
    unsigned long long tail = 0;
    SG_HIP(hipMemcpyAsync(&tail, uniq + E - 1, 8, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (tail == ~0ull) --E;                                                    // the self pairs, if any, collapsed into one trailing key
    if (E > 0) k_pc_unpack<<<sg::cdiv(E, kBlock), kBlock, 0, st>>>(uniq, E, p.adj);
    clock.tick();
    if (E == 0) { SG_LAUNCH_CHECK(); return SG_OK; }
    // 7. weights and keys, 8. ascending (w, a, b) and the gather: 8d's stages
    k_pc_weights<<<sg::cdiv(E, kBlock), kBlock, 0, st>>>(p.adj, E, p.cand, d_normals, p.w, p.k0, p.v0);
    clock.tick();
    const int* order = sgos::sort_by_weight(p.k0, p.k1, p.v0, p.v1, p.hist, E, st);
    clock.tick();
    sgos::gather_edges(order, E, p.adj, p.w, d_edges, d_w, st);
    clock.tick();
    SG_LAUNCH_CHECK();
    *h_E = E;
    return SG_OK;
}

int pcseg_scan(const char* who, const float* d_xyz, int N, int k, const float* h_viewpoint, int index, float cell, float k_thresh,
               int seg_min_verts, int32_t* h_seg_indices, void* d_ws, size_t ws_bytes, void* stream) {
    if (!(N > 0 && d_xyz && h_seg_indices && d_ws)) return sg::fail(SG_EINVAL, "%s: bad arguments", who);
    const int rc0 = check_k(who, N, k, index);
    if (rc0 < 0) return rc0;
    const Plan p = carve(d_ws, ws_bytes, N, k, index);
    if (!p.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, pcseg_ws_bytes(N, k, index));
    int E = 0;
    const int rc = pcseg_edges(index == SG_KNN_GRID ? "sg_pcseg_edges_indexed" : "sg_pcseg_edges", d_xyz, N, k, h_viewpoint, index, cell, nullptr,
                               p.vn, p.edges, p.w_sorted, &E, d_ws, ws_bytes, stream);
    if (rc < 0) return rc;
    std::vector<int32_t> h_edges((size_t)E * 2);
    std::vector<float> h_w((size_t)E);
    if (E > 0) {
        hipStream_t st = sg::as_stream(stream);
        SG_HIP(hipMemcpyAsync(h_edges.data(), p.edges, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        SG_HIP(hipMemcpyAsync(h_w.data(), p.w_sorted, (size_t)E * 4, hipMemcpyDeviceToHost, st));
        SG_HIP(hipStreamSynchronize(st));
    }
    return sg_overseg_merge(h_edges.data(), h_w.data(), E, N, k_thresh, seg_min_verts, h_seg_indices);
}

// ---- the radius graph instead of the kNN graph ------------------------------------------------------------------------
struct RPlan {                      // the workspace of one cloud at room for T pairs; E = T / 2
    float4* cand;
    Misc* misc;
    int64_t *off, *eoff;            // [N + 1]
    int32_t* idx;                   // [T]
    int32_t* up;                    // [N]
    long long* tsum;
    int64_t* adj;                   // [E,2]
    float* w;
    unsigned int *k0, *k1;
    int *v0, *v1;
    int* hist;
    float* vn;
    int32_t* edges;
    float* w_sorted;
    char* lists;                    // sg_radius_neighbours_grid's workspace
    size_t lists_bytes;
    bool ok;
};

RPlan carve_radius(void* d_ws, size_t ws_bytes, int N, int64_t T) {
    RPlan p{};
    const size_t np = (size_t)std::max(N, 1), t = (size_t)std::max<int64_t>(T, 0), e = std::max<size_t>(t / 2, 1);
    sg::Carver cv(d_ws, ws_bytes);
    p.cand = cv.take<float4>(np);
    p.misc = cv.take<Misc>(1);
    p.off = cv.take<int64_t>(np + 1);
    p.eoff = cv.take<int64_t>(np + 1);
    p.idx = cv.take<int32_t>(std::max<size_t>(t, 1));
    p.up = cv.take<int32_t>(np);
    p.tsum = cv.take<long long>((size_t)sgscan::tiles_of((int)np) + 1);
    p.adj = cv.take<int64_t>(e * 2);
    p.w = cv.take<float>(e);
    p.k0 = cv.take<unsigned int>(e);
    p.k1 = cv.take<unsigned int>(e);
    p.v0 = cv.take<int>(e);
    p.v1 = cv.take<int>(e);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)e));
    p.vn = cv.take<float>(np * 3);
    p.edges = cv.take<int32_t>(e * 2);
    p.w_sorted = cv.take<float>(e);
    p.lists_bytes = sg_radius_neighbours_ws_bytes(N, T);
    p.lists = cv.take<char>(p.lists_bytes);
    p.ok = cv.ok && p.lists_bytes > 0;
    return p;
}

size_t pcseg_ws_bytes_radius(int N, int64_t T) {
    const size_t np = (size_t)N, t = (size_t)T, e = std::max<size_t>(t / 2, 1);
    return sg::align_up(np * 16) + sg::align_up(sizeof(Misc)) + 2 * sg::align_up((np + 1) * 8) + sg::align_up(std::max<size_t>(t, 1) * 4) +
           sg::align_up(np * 4) + sg::align_up(((size_t)sgscan::tiles_of(N) + 1) * 8) + sg::align_up(e * 16) + 5 * sg::align_up(e * 4) +
           sg::align_up(sgsort::hist_ints((long long)e) * 4) + sg::align_up(np * 12) + sg::align_up(e * 8) + sg::align_up(e * 4) +
           sg::align_up(sg_radius_neighbours_ws_bytes(N, T));
}

constexpr int kListStages = 8;      // box, cells, sort, table, count, scan, fill, rows: the lists' own (kernels_radius.hip)
constexpr int kOwnStages = 5;
constexpr int kRStages = kListStages + kOwnStages;
const char* const kOwnStageNames[kOwnStages] = {"normals", "edges", "weights", "weight_sort", "gather"};
thread_local sgos::StageTimes<kRStages> t_rtimes;       // the lists' stages in front, then this file's own

struct ListTiming {                 // the lists report their stages to this thread while one of these lives
    bool on;
    explicit ListTiming(bool o) : on(o) { if (on) sg::radius_lists_timing(true); }
    ~ListTiming() { if (on) sg::radius_lists_timing(false); }
};

int pcseg_edges_radius(const char* who, const float* d_xyz, int N, float radius, float cell, int64_t capacity, const float* h_viewpoint,
                       int64_t* d_off, int32_t* d_idx, float* d_normals, int32_t* d_edges, float* d_w, int* h_E, int64_t* h_T, void* d_ws,
                       size_t ws_bytes, void* stream) {
    if (!(d_xyz && d_normals && h_E && h_T && d_ws)) return sg::fail(SG_EINVAL, "%s: a null pointer", who);
    *h_E = 0;
    *h_T = 0;
    SG_REQUIRE(N >= 1, "%s: %d points", who, N);
    if (N > SG_MAX_GRID_POINTS) return sg::fail(SG_EUNSUP, "%s: %d points; the grid path holds at most %d", who, N, SG_MAX_GRID_POINTS);
    if (capacity > SG_MAX_RADIUS_PAIRS)
        return sg::fail(SG_EUNSUP, "%s: room for %lld pairs; the lists hold at most %lld: take a smaller radius, or thin the cloud first", who,
                        (long long)capacity, (long long)SG_MAX_RADIUS_PAIRS);
    SG_REQUIRE(capacity >= 0 && (capacity < 2 || (d_edges && d_w)), "%s: room for %lld pairs at a null pointer", who, (long long)capacity);
    SG_REQUIRE((d_off == nullptr) == (d_idx == nullptr) || capacity == 0, "%s: the caller's lists are both offsets and indices", who);
    int rc = viewpoint_ok(who, h_viewpoint);
    if (rc < 0) return rc;
    const RPlan p = carve_radius(d_ws, ws_bytes, N, capacity);
    if (!p.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, pcseg_ws_bytes_radius(N, capacity));
    hipStream_t st = sg::as_stream(stream);
    int64_t* off = d_off ? d_off : p.off;
    int32_t* idx = d_idx ? d_idx : p.idx;
    if (t_rtimes.timing) for (int i = 0; i < kRStages; ++i) t_rtimes.us[i] = 0.0f;
    // the lists: every refusal of 8k and the pair cap are theirs
    {
        const ListTiming lt(t_rtimes.timing);
        rc = sg::radius_lists(who, d_xyz, 3, N, radius, cell, capacity, off, idx, h_T, p.lists, p.lists_bytes, stream);
        if (t_rtimes.timing) for (int i = 0; i < kListStages; ++i) t_rtimes.us[i] = sg::radius_lists_stage_us()[i];
    }
    if (rc < 0) return rc;
    const int64_t T = *h_T;
    sgos::StageClock<kOwnStages> clock(st, t_rtimes.timing, t_rtimes.us + kListStages);
    // normals over the rows
    k_pc_init<<<1, 1, 0, st>>>(p.misc, h_viewpoint != nullptr, h_viewpoint ? h_viewpoint[0] : 0.0f, h_viewpoint ? h_viewpoint[1] : 0.0f,
                               h_viewpoint ? h_viewpoint[2] : 0.0f);
    k_pc_pack<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_xyz, 3, N, p.cand, p.misc);
    if (!h_viewpoint) k_pc_view<<<1, 1, 0, st>>>(p.misc);
    k_pc_normals_csr<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(p.cand, N, off, idx, p.misc, d_normals);
    clock.tick();
    // the pairs a < b in lexicographic order: the upper halves of the rows
    k_pc_upper_counts<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(off, idx, N, p.up);
    sgscan::exclusive_scan64(p.up, N, p.tsum, p.eoff, st);
    int64_t E64 = 0;
    int flag = 0;
    SG_HIP(hipMemcpyAsync(&E64, p.eoff + N, 8, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&flag, &p.misc->flag, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (flag & 1) return sg::fail(SG_EINVAL, "%s: a coordinate is not finite", who);
    if (flag & (4 | 8)) return sg::fail(SG_EINTERNAL, "%s: the lists do not hold together (flag %d)", who, flag);
    if (E64 * 2 != T) return sg::fail(SG_EINTERNAL, "%s: %lld upper entries in rows of %lld", who, (long long)E64, (long long)T);
    const int E = (int)E64;                                  // T <= SG_MAX_RADIUS_PAIRS = 2^30: E <= 2^29
    if (E > 0) k_pc_edges_csr<<<sg::cdiv(N, kBlock / 64), kBlock, 0, st>>>(off, idx, N, p.eoff, E64, p.adj);
    clock.tick();
    if (E == 0) { SG_LAUNCH_CHECK(); return SG_OK; }
    k_pc_weights<<<sg::cdiv(E, kBlock), kBlock, 0, st>>>(p.adj, E, p.cand, d_normals, p.w, p.k0, p.v0);
    clock.tick();
    const int* order = sgos::sort_by_weight(p.k0, p.k1, p.v0, p.v1, p.hist, E, st);
    clock.tick();
    sgos::gather_edges(order, E, p.adj, p.w, d_edges, d_w, st);
    clock.tick();
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    *h_E = E;
    return SG_OK;
}

int pcseg_scan_radius(const char* who, const float* d_xyz, int N, float radius, float cell, int64_t capacity, const float* h_viewpoint,
                      float k_thresh, int seg_min_verts, int32_t* h_seg_indices, int64_t* h_T, void* d_ws, size_t ws_bytes, void* stream) {
    if (!(d_xyz && h_seg_indices && h_T && d_ws)) return sg::fail(SG_EINVAL, "%s: a null pointer", who);
    const RPlan p = carve_radius(d_ws, ws_bytes, std::max(N, 1), std::max<int64_t>(std::min<int64_t>(capacity, SG_MAX_RADIUS_PAIRS), 0));
    if (N >= 1 && N <= SG_MAX_GRID_POINTS && capacity >= 0 && capacity <= SG_MAX_RADIUS_PAIRS && !p.ok)
        return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, pcseg_ws_bytes_radius(N, capacity));
    int E = 0;
    const int rc = pcseg_edges_radius(who, d_xyz, N, radius, cell, capacity, h_viewpoint, nullptr, nullptr, p.vn, p.edges, p.w_sorted, &E, h_T,
                                      d_ws, ws_bytes, stream);
    if (rc < 0) return rc;
    std::vector<int32_t> h_edges((size_t)E * 2);
    std::vector<float> h_w((size_t)E);
    if (E > 0) {
        hipStream_t st = sg::as_stream(stream);
        SG_HIP(hipMemcpyAsync(h_edges.data(), p.edges, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        SG_HIP(hipMemcpyAsync(h_w.data(), p.w_sorted, (size_t)E * 4, hipMemcpyDeviceToHost, st));
        SG_HIP(hipStreamSynchronize(st));
    }
    return sg_overseg_merge(h_edges.data(), h_w.data(), E, N, k_thresh, seg_min_verts, h_seg_indices);
}

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(pcseg, t_times, kStageNames)

size_t sg_pointcloud_knn_ws_bytes(int N) { return sg::align_up((size_t)std::max(N, 1) * 16) + sg::align_up(sizeof(Misc)); }

int sg_pointcloud_knn(const float* d_points, int stride, int N, int k, int32_t* d_knn, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_points && stride >= 3 && N > 0 && d_knn && d_ws, "sg_pointcloud_knn: bad arguments");
    const int rc = check_k("sg_pointcloud_knn", N, k);
    if (rc < 0) return rc;
    sg::Carver cv(d_ws, ws_bytes);
    float4* cand = cv.take<float4>(N);
    Misc* misc = cv.take<Misc>(1);
    if (!cv.ok) return sg::fail(SG_ENOMEM, "sg_pointcloud_knn: workspace too small (%zu < %zu)", ws_bytes, sg_pointcloud_knn_ws_bytes(N));
    hipStream_t st = sg::as_stream(stream);
    k_pc_init<<<1, 1, 0, st>>>(misc, 1, 0.0f, 0.0f, 0.0f);
    k_pc_pack<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_points, stride, N, cand, misc);
    launch_knn(cand, N, k, d_knn, misc, st);
    int flag = 0;
    SG_HIP(hipMemcpyAsync(&flag, &misc->flag, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (flag & 1) return sg::fail(SG_EINVAL, "sg_pointcloud_knn: a coordinate is not finite");
    if (flag & 2) return sg::fail(SG_EINVAL, "sg_pointcloud_knn: the coordinates are too large for the fp32 pair score");
    return SG_OK;
}

int sg_pointcloud_normals(const float* d_xyz, int N, const int32_t* d_knn, int k, const float* h_viewpoint, float* d_normals, void* d_ws,
                          size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_xyz && N > 0 && d_knn && d_normals && d_ws, "sg_pointcloud_normals: bad arguments");
    int rc = check_k("sg_pointcloud_normals", N, k);
    if (rc < 0) return rc;
    if ((rc = viewpoint_ok("sg_pointcloud_normals", h_viewpoint)) < 0) return rc;
    sg::Carver cv(d_ws, ws_bytes);
    float4* cand = cv.take<float4>(N);
    Misc* misc = cv.take<Misc>(1);
    if (!cv.ok) return sg::fail(SG_ENOMEM, "sg_pointcloud_normals: workspace too small (%zu < %zu)", ws_bytes, sg_pointcloud_knn_ws_bytes(N));
    hipStream_t st = sg::as_stream(stream);
    k_pc_init<<<1, 1, 0, st>>>(misc, h_viewpoint != nullptr, h_viewpoint ? h_viewpoint[0] : 0.0f, h_viewpoint ? h_viewpoint[1] : 0.0f,
                               h_viewpoint ? h_viewpoint[2] : 0.0f);
    k_pc_pack<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_xyz, 3, N, cand, misc);
    if (!h_viewpoint) k_pc_view<<<1, 1, 0, st>>>(misc);
    launch_normals(d_xyz, 3, N, k, d_knn, misc, d_normals, st);
    int flag = 0;
    SG_HIP(hipMemcpyAsync(&flag, &misc->flag, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (flag & 1) return sg::fail(SG_EINVAL, "sg_pointcloud_normals: a coordinate is not finite");
    if (flag & 4) return sg::fail(SG_EINVAL, "sg_pointcloud_normals: a list names a point outside 0..%d", N - 1);
    return SG_OK;
}

size_t sg_pcseg_ws_bytes(int N, int k) { return pcseg_ws_bytes(N, k, SG_KNN_BRUTE); }

size_t sg_pcseg_ws_bytes_indexed(int N, int k, int index) {
    if (index == SG_KNN_GRID) return sg_pointcloud_knn_grid_ws_bytes(N, k) ? pcseg_ws_bytes(N, k, index) : 0;
    return index == SG_KNN_BRUTE ? pcseg_ws_bytes(N, k, index) : 0;
}

int sg_pcseg_edges(const float* d_xyz, int N, int k, const float* h_viewpoint, int32_t* d_knn, float* d_normals, int32_t* d_edges, float* d_w,
                   int* h_E, void* d_ws, size_t ws_bytes, void* stream) {
    return pcseg_edges("sg_pcseg_edges", d_xyz, N, k, h_viewpoint, SG_KNN_BRUTE, 0.0f, d_knn, d_normals, d_edges, d_w, h_E, d_ws, ws_bytes, stream);
}

int sg_pcseg_edges_indexed(const float* d_xyz, int N, int k, const float* h_viewpoint, int index, float cell, int32_t* d_knn, float* d_normals,
                           int32_t* d_edges, float* d_w, int* h_E, void* d_ws, size_t ws_bytes, void* stream) {
    return pcseg_edges("sg_pcseg_edges_indexed", d_xyz, N, k, h_viewpoint, index, cell, d_knn, d_normals, d_edges, d_w, h_E, d_ws, ws_bytes,
                       stream);
}

int sg_pcseg_scan(const float* d_xyz, int N, int k, const float* h_viewpoint, float k_thresh, int seg_min_verts, int32_t* h_seg_indices,
                  void* d_ws, size_t ws_bytes, void* stream) {
    return pcseg_scan("sg_pcseg_scan", d_xyz, N, k, h_viewpoint, SG_KNN_BRUTE, 0.0f, k_thresh, seg_min_verts, h_seg_indices, d_ws, ws_bytes, stream);
}

int sg_pcseg_scan_indexed(const float* d_xyz, int N, int k, const float* h_viewpoint, int index, float cell, float k_thresh, int seg_min_verts,
                          int32_t* h_seg_indices, void* d_ws, size_t ws_bytes, void* stream) {
    return pcseg_scan("sg_pcseg_scan_indexed", d_xyz, N, k, h_viewpoint, index, cell, k_thresh, seg_min_verts, h_seg_indices, d_ws, ws_bytes,
                      stream);
}

int sg_pointcloud_normals_csr(const float* d_xyz, int N, const int64_t* d_off, const int32_t* d_idx, const float* h_viewpoint, float* d_normals,
                              void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_pointcloud_normals_csr";
    SG_REQUIRE(d_xyz && N > 0 && d_off && d_normals && d_ws, "%s: bad arguments", who);
    if (N > SG_MAX_GRID_POINTS) return sg::fail(SG_EUNSUP, "%s: %d points; the grid path holds at most %d", who, N, SG_MAX_GRID_POINTS);
    const int rc = viewpoint_ok(who, h_viewpoint);
    if (rc < 0) return rc;
    sg::Carver cv(d_ws, ws_bytes);
    float4* cand = cv.take<float4>(N);
    Misc* misc = cv.take<Misc>(1);
    if (!cv.ok) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_pointcloud_knn_ws_bytes(N));
    hipStream_t st = sg::as_stream(stream);
    k_pc_init<<<1, 1, 0, st>>>(misc, h_viewpoint != nullptr, h_viewpoint ? h_viewpoint[0] : 0.0f, h_viewpoint ? h_viewpoint[1] : 0.0f,
                               h_viewpoint ? h_viewpoint[2] : 0.0f);
    k_pc_pack<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_xyz, 3, N, cand, misc);
    if (!h_viewpoint) k_pc_view<<<1, 1, 0, st>>>(misc);
    // d_idx may be null only where every row is empty; a row that is not then fails the check of its offsets against off[N]
    k_pc_normals_csr<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(cand, N, d_off, d_idx, misc, d_normals);
    int flag = 0;
    SG_HIP(hipMemcpyAsync(&flag, &misc->flag, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (flag & 1) return sg::fail(SG_EINVAL, "%s: a coordinate is not finite", who);
    if (flag & 8) return sg::fail(SG_EINVAL, "%s: the offsets of the rows do not ascend from 0 to off[N]", who);
    if (flag & 4) return sg::fail(SG_EINVAL, "%s: a row names a point outside 0..%d", who, N - 1);
    return SG_OK;
}

size_t sg_pcseg_ws_bytes_radius(int N, int64_t T) {
    if (N < 1 || N > SG_MAX_GRID_POINTS || T < 0 || T > SG_MAX_RADIUS_PAIRS) return 0;
    return pcseg_ws_bytes_radius(N, T);
}

int sg_pcseg_edges_radius(const float* d_xyz, int N, float radius, float cell, int64_t capacity, const float* h_viewpoint, int64_t* d_off,
                          int32_t* d_idx, float* d_normals, int32_t* d_edges, float* d_w, int* h_E, int64_t* h_T, void* d_ws, size_t ws_bytes,
                          void* stream) {
    return pcseg_edges_radius("sg_pcseg_edges_radius", d_xyz, N, radius, cell, capacity, h_viewpoint, d_off, d_idx, d_normals, d_edges, d_w, h_E,
                              h_T, d_ws, ws_bytes, stream);
}

int sg_pcseg_scan_radius(const float* d_xyz, int N, float radius, float cell, int64_t capacity, const float* h_viewpoint, float k_thresh,
                         int seg_min_verts, int32_t* h_seg_indices, int64_t* h_T, void* d_ws, size_t ws_bytes, void* stream) {
    return pcseg_scan_radius("sg_pcseg_scan_radius", d_xyz, N, radius, cell, capacity, h_viewpoint, k_thresh, seg_min_verts, h_seg_indices, h_T,
                             d_ws, ws_bytes, stream);
}

int sg_pcseg_radius_set_timing(int on) { t_rtimes.timing = on != 0; return SG_OK; }
int sg_pcseg_radius_stage_times(float* h_us, int cap) { return t_rtimes.copy("sg_pcseg_radius_stage_times", h_us, cap); }
const char* sg_pcseg_radius_stage_name(int i) {
    return i < kListStages ? sg::radius_lists_stage_name(i) : sgos::stage_name(kOwnStageNames, i - kListStages);
}

}  // extern "C"
