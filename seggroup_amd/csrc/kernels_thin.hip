// Voxel thinning of a large point cloud: one input point per occupied voxel, and for every point the thinned point that
// stands for it.  The front end of the point-cloud over-segmenter for clouds above SG_MAX_POINTS: the segmenter works on the thinned cloud,
// its ids go back to every point through the map.
//
//   k_thin_box          coordinates finite (one flag word), the cloud's bounding box (order-free min / max on k_pc_pack's integer keys):
//                       the box pieces of overseg_device.h, which k_grid_box (grid_index_device.h) is made of as well
//   k_thin_keys         per point its cell, the voxel key (c2, c1, c0 packed over exactly the bits the box needs) and the bits of d2
//   sort                stable radix sort of (key, index) over the key's bits in use (sort_device.h)
//   k_thin_argmin       run heads -> voxel numbers (sort_device.h's head flags and scan); per voxel a 64-bit atomicMin of
//                       (d2 bits << 32 | index): the smallest d2, the lowest index among equals, whatever the order of the atomics
//   flags, scan, rep    1 at every representative in raw order, exclusive scan, rep[] in ascending raw index
//   k_thin_map          thin_of_point[i] = the rank of the representative of i's voxel
//
// Every fp32 operation is written op by op and rounded once (-ffp-contract=off; only - / * + floor and comparisons), which
// tests/test_gpu_thin.py holds to the NumPy statement of the specification (tests/thin_ref.py) bit for bit.  Results are integers.
#include <cmath>

#include "sg_common.h"
#include "sort_device.h"
#include "overseg_device.h"

namespace {

using sgos::bits_for_cells;
using sgos::kBoxBlocks;
using sgos::kCellLimit;
using sgos::unkey_host;

constexpr int kBlock = sgos::kBoxBlock;

struct Misc {
    int flag;                       // |= 1: a coordinate is not finite
    int count;                      // occupied voxels
    unsigned int lo[3], hi[3];      // the bounding box as sgos::weight_key words
};

struct Grid {                       // what the host derives from the box
    float lo[3];
    float h;
    int shift1, shift2;             // key = c0 | c1 << shift1 | c2 << shift2
};

__global__ void k_thin_init(Misc* __restrict__ m) {
    m->flag = 0;
    m->count = 0;
    for (int a = 0; a < 3; ++a) { m->lo[a] = 0xffffffffu; m->hi[a] = 0u; }
}

// the box reduction of overseg_device.h as it is: kBoxBlocks blocks, 6 atomics per block
__global__ __launch_bounds__(kBlock) void k_thin_box(const float* __restrict__ p, int stride, int N, Misc* __restrict__ m) {
    __shared__ unsigned int s_lo[3][sgos::kBoxWaves], s_hi[3][sgos::kBoxWaves];
    sgos::Box box;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * kBlock) {
        const float c[3] = {p[i * stride], p[i * stride + 1], p[i * stride + 2]};
        sgos::box_take(box, c);
    }
    sgos::box_stage(box, &m->flag, s_lo, s_hi);
    __syncthreads();
    sgos::box_commit(s_lo, s_hi, m->lo, m->hi);
}

// 8g steps 2-4 for point i: key[i], idx[i] = i, d2[i] (the bits of a non-negative float or +inf: ascending as unsigned)
__global__ __launch_bounds__(kBlock) void k_thin_keys(const float* __restrict__ p, int stride, int N, Grid g, unsigned long long* __restrict__ key,
                                                      int* __restrict__ idx, unsigned int* __restrict__ d2) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float x = p[(size_t)i * stride], y = p[(size_t)i * stride + 1], z = p[(size_t)i * stride + 2];
    const float q0 = (x - g.lo[0]) / g.h, q1 = (y - g.lo[1]) / g.h, q2 = (z - g.lo[2]) / g.h;
    const float f0 = __builtin_floorf(q0), f1 = __builtin_floorf(q1), f2 = __builtin_floorf(q2);
    const float t0 = g.lo[0] + (f0 + 0.5f) * g.h, t1 = g.lo[1] + (f1 + 0.5f) * g.h, t2 = g.lo[2] + (f2 + 0.5f) * g.h;
    const float e0 = x - t0, e1 = y - t1, e2 = z - t2;
    const float dd = (e0 * e0 + e1 * e1) + e2 * e2;
    // the host checked the box's largest cell, and the cell is monotone in the coordinate: 0 <= f < 2^21
    key[i] = (unsigned long long)(unsigned int)f0 | ((unsigned long long)(unsigned int)f1 << g.shift1) |
             ((unsigned long long)(unsigned int)f2 << g.shift2);
    idx[i] = i;
    d2[i] = __float_as_uint(dd);
}

__global__ __launch_bounds__(kBlock) void k_thin_fill(unsigned long long* __restrict__ best, int N) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < N) best[i] = ~0ull;
}

// sorted position s: its voxel number (heads before it, itself included, minus one) -> vox[point], best[voxel] = min(d2 << 32 | point).
// The lanes of a wave that share a voxel are neighbours (the keys are sorted): a segmented min-scan along the wave leaves each segment's
// minimum in its last lane, which alone goes to memory -- a voxel of thousands of points costs an atomic per wave, not per point.
__global__ __launch_bounds__(kBlock) void k_thin_argmin(const unsigned long long* __restrict__ key, const int* __restrict__ idx,
                                                        const int* __restrict__ pos, const int* __restrict__ tile_sum, int N,
                                                        const unsigned int* __restrict__ d2, int* __restrict__ vox,
                                                        unsigned long long* __restrict__ best) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = s < N;
    int v = -1;
    unsigned long long val = ~0ull;
    if (live) {
        const int head = (s == 0 || key[s] != key[s - 1]) ? 1 : 0;
        v = pos[s] + tile_sum[s / sgsort::kTile] + head - 1;
        const int i = idx[s];
        vox[i] = v;
        val = ((unsigned long long)d2[i] << 32) | (unsigned int)i;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long ov = __shfl_up(val, off);
        const int vv = __shfl_up(v, off);
        if (lane >= off && vv == v) val = min(val, ov);
    }
    const int next = __shfl_down(v, 1);
    if (live && (lane == 63 || next != v)) atomicMin(&best[v], val);
}

__global__ __launch_bounds__(kBlock) void k_thin_flags(const int* __restrict__ vox, const unsigned long long* __restrict__ best, int N,
                                                       int* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < N) flag[i] = (int)(best[vox[i]] & 0xffffffffull) == i ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_thin_rep(const int* __restrict__ vox, const unsigned long long* __restrict__ best,
                                                     const int* __restrict__ pos, const int* __restrict__ tile_sum, int N,
                                                     int32_t* __restrict__ rep) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    if ((int)(best[vox[i]] & 0xffffffffull) == i) rep[pos[i] + tile_sum[i / sgsort::kTile]] = i;
}

__global__ __launch_bounds__(kBlock) void k_thin_map(const int* __restrict__ vox, const unsigned long long* __restrict__ best,
                                                     const int* __restrict__ pos, const int* __restrict__ tile_sum, int N,
                                                     int32_t* __restrict__ thin_of_point) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int r = (int)(best[vox[i]] & 0xffffffffull);
    thin_of_point[i] = pos[r] + tile_sum[r / sgsort::kTile];
}

struct Plan {
    Misc* misc;
    unsigned long long *k0, *k1;    // voxel keys
    int *v0, *v1;                   // point indices
    int* hist;
    unsigned int* d2;               // [N] raw order
    int* vox;                       // [N] raw order: the point's voxel number
    unsigned long long* best;       // [N] per voxel
    int* heads;                     // unique_ints(N): head flags of the sorted keys -> their exclusive scan
    int* flags;                     // unique_ints(N): representative flags in raw order -> their exclusive scan
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, int N) {
    Plan p{};
    const size_t n = (size_t)std::max(N, 1);
    sg::Carver cv(d_ws, ws_bytes);
    p.misc = cv.take<Misc>(1);
    p.k0 = cv.take<unsigned long long>(n);
    p.k1 = cv.take<unsigned long long>(n);
    p.v0 = cv.take<int>(n);
    p.v1 = cv.take<int>(n);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    p.d2 = cv.take<unsigned int>(n);
    p.vox = cv.take<int>(n);
    p.best = cv.take<unsigned long long>(n);
    p.heads = cv.take<int>(sgsort::unique_ints((long long)n));
    p.flags = cv.take<int>(sgsort::unique_ints((long long)n));
    p.ok = cv.ok;
    return p;
}

// sg_cloud_thin_set_timing(1): the calling thread's next sg_cloud_thin calls bracket their stages with events (tools/time_thin.py)
constexpr int kStages = 6;
const char* const kStageNames[kStages] = {"check_box", "keys", "sort", "representatives", "compact", "map"};
thread_local sgos::StageTimes<kStages> t_times;

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(cloud_thin, t_times, kStageNames)

size_t sg_cloud_thin_ws_bytes(int N) {
    if (N < 1 || N > SG_MAX_CLOUD_POINTS) return 0;
    const size_t n = (size_t)N;
    return sg::align_up(sizeof(Misc)) + 3 * sg::align_up(n * 8) + 4 * sg::align_up(n * 4) + sg::align_up(sgsort::hist_ints((long long)n) * 4) +
           2 * sg::align_up(sgsort::unique_ints((long long)n) * 4);
}

int sg_cloud_thin(const float* d_points, int stride, int N, float voxel, int32_t* d_rep, int32_t* d_thin_of_point, int* h_M, float* h_lo3,
                  void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_points && d_rep && d_thin_of_point && h_M && d_ws, "sg_cloud_thin: a null pointer");
    *h_M = 0;
    SG_REQUIRE(stride >= 3 && N >= 1, "sg_cloud_thin: %d points in rows of %d floats", N, stride);
    SG_REQUIRE(std::isfinite(voxel) && voxel > 0.0f, "sg_cloud_thin: the voxel edge must be finite and positive (%g)", (double)voxel);
    if (N > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "sg_cloud_thin: %d points; a cloud holds at most %d", N, SG_MAX_CLOUD_POINTS);
    const Plan p = carve(d_ws, ws_bytes, N);
    SG_REQUIRE(p.ok, "sg_cloud_thin: workspace too small (%zu < %zu)", ws_bytes, sg_cloud_thin_ws_bytes(N));
    hipStream_t st = sg::as_stream(stream);
    const int nb = sg::cdiv(N, kBlock);
    sgos::StageClock<kStages> clock(st, t_times.timing, t_times.us);
    // 1. the coordinates are the caller's; the box
    k_thin_init<<<1, 1, 0, st>>>(p.misc);
    k_thin_box<<<std::min(nb, kBoxBlocks), kBlock, 0, st>>>(d_points, stride, N, p.misc);
    Misc hm{};
    SG_HIP(hipMemcpyAsync(&hm, p.misc, sizeof(Misc), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (hm.flag & 1) return sg::fail(SG_EINVAL, "sg_cloud_thin: a coordinate is not finite");
    clock.tick();
    // 2. the largest cell per axis is the cell of the box's maximum: decided here, in the device's arithmetic
    Grid g{};
    g.h = voxel;
    int bits[3];
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = unkey_host(hm.lo[a]);
        const float span = unkey_host(hm.hi[a]) - g.lo[a];
        const float q = span / voxel;
        if (!(q < kCellLimit))
            return sg::fail(SG_EUNSUP, "sg_cloud_thin: voxel too small for the cloud's extent (axis %d: %g / %g is not below %g cells)", a,
                            (double)span, (double)voxel, (double)kCellLimit);
        bits[a] = bits_for_cells((unsigned int)std::floor(q) + 1u);
    }
    g.shift1 = bits[0];
    g.shift2 = bits[0] + bits[1];
    const int key_bits = bits[0] + bits[1] + bits[2];
    if (h_lo3) for (int a = 0; a < 3; ++a) h_lo3[a] = g.lo[a];
    k_thin_keys<<<nb, kBlock, 0, st>>>(d_points, stride, N, g, p.k0, p.v0, p.d2);
    clock.tick();
    // 3. stable by voxel key: inside a run the indices ascend
    auto L = sgsort::one_list<unsigned long long, int>(p.k0, p.k1, p.v0, p.v1, p.hist, N);
    sgsort::radix_sort<unsigned long long, int, true>(L, 1, 0, key_bits, st);
    clock.tick();
    // 5. the representatives
    int* htile = p.heads + N;
    sgsort::k_head_flags<unsigned long long><<<nb, kBlock, 0, st>>>(L.kin[0], N, p.heads);
    sgsort::k_scan_tiles<><<<sgsort::tiles_of(N), sgsort::kThreads, 0, st>>>(p.heads, N, htile);
    sgsort::k_scan_tile_sums<><<<1, 1024, 0, st>>>(htile, sgsort::tiles_of(N), &p.misc->count);
    k_thin_fill<<<nb, kBlock, 0, st>>>(p.best, N);
    k_thin_argmin<<<nb, kBlock, 0, st>>>(L.kin[0], L.vin[0], p.heads, htile, N, p.d2, p.vox, p.best);
    clock.tick();
    // 6. rep in ascending raw index
    int* ftile = p.flags + N;
    k_thin_flags<<<nb, kBlock, 0, st>>>(p.vox, p.best, N, p.flags);
    sgsort::k_scan_tiles<><<<sgsort::tiles_of(N), sgsort::kThreads, 0, st>>>(p.flags, N, ftile);
    sgsort::k_scan_tile_sums<><<<1, 1024, 0, st>>>(ftile, sgsort::tiles_of(N), nullptr);
    k_thin_rep<<<nb, kBlock, 0, st>>>(p.vox, p.best, p.flags, ftile, N, d_rep);
    clock.tick();
    k_thin_map<<<nb, kBlock, 0, st>>>(p.vox, p.best, p.flags, ftile, N, d_thin_of_point);
    clock.tick();
    int M = 0;
    SG_HIP(hipMemcpyAsync(&M, &p.misc->count, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (M < 1 || M > N) return sg::fail(SG_EHIP, "sg_cloud_thin: %d voxels from %d points", M, N);
    *h_M = M;
    return SG_OK;
}

}  // extern "C"
