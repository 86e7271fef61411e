// The deterministic moment sums, written once: the launch shape, both reduction trees and the host sequence
// around them.  A moment kernel (k_align_moments, k_plane_moments, k_pl_moments, k_lb_moments) runs kBlock threads that take kPer items
// each -- thread t the items t, t + 256, .. of its workgroup's kItems, in order -- and hands its accumulators to block_row, the FIRST tree:
// one row of kM doubles per workgroup.  k_fold, the SECOND tree, is one workgroup that adds those rows.  Grid, block and both trees are
// functions of the item count alone, so the sums do not depend on the device or the stream.  No floating-point atomics.
// (In a header because three kernel files use it; each gets its own copy.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "sg_common.h"
#include "wave_ops.h"

namespace sgmom {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPer = 4;                       // items per thread: four independent gathers in flight
constexpr int kItems = kBlock * kPer;         // items per workgroup = per partial row

// The first tree.  EVERY thread of the workgroup must reach this call (wave_sum needs all 64 lanes, and there is a barrier inside): an
// item that does not count adds 0 to acc.  A wave sums each slot on the DPP network of wave_ops.h, lane 0 leaves it in the wave's LDS
// row, and after the barrier threads 0..kM-1 add the waves' rows in the order 0, 1, 2, 3 and store row[0..kM).
template <int kM>
__device__ __forceinline__ void block_row(const double (&acc)[kM], double* __restrict__ row) {
    static_assert(kM <= kBlock, "one thread per slot");
    __shared__ double s_rows[kWaves][kM];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
    for (int m = 0; m < kM; ++m) {
        const double s = sgw::wave_sum(acc[m]);
        if (lane == 0) s_rows[wave][m] = s;
    }
    __syncthreads();
    if (threadIdx.x < kM) {
        double s = s_rows[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += s_rows[w][threadIdx.x];
        row[threadIdx.x] = s;
    }
}

// The second tree: thread t adds rows t, t + 256, .. in order, a wave sums on the same network, the four waves' sums are added in order.
template <int kM>
__global__ __launch_bounds__(kBlock) void k_fold(const double* __restrict__ partial, int rows, double* __restrict__ out) {
    __shared__ double s_rows[kWaves][kM];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll 1
    for (int m = 0; m < kM; ++m) {
        double acc = 0.0;
        for (int r = threadIdx.x; r < rows; r += kBlock) acc += partial[(size_t)r * kM + m];
        const double s = sgw::wave_sum(acc);
        if (lane == 0) s_rows[wave][m] = s;
    }
    __syncthreads();
    if (threadIdx.x < kM) {
        double s = s_rows[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += s_rows[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
template <int kM> struct Landing { double m[kM]; int flag; int pad; };   // what one copy brings back: the sums and the flag word

template <int kM>
inline size_t ws_bytes(int items) {
    return sg::align_up(sizeof(Landing<kM>)) + sg::align_up((size_t)std::max(sg::cdiv(items, kItems), 1) * kM * sizeof(double));
}

struct Nothing { void operator()() const {} };

// kM sums over `items` >= 1 items into h_out, and the flag word into *h_flag; a flag word that is not 0 leaves h_out alone.
// first(rows, d_partial, d_flag) launches the moment kernel on `st`: `rows` workgroups of kBlock threads, one partial row each; it may
// raise bits in *d_flag, which starts at 0.  h_flag == nullptr: a kernel that raises none -- d_flag is NULL and the memset that clears the
// word (3 us of a 23 us call, measured) is left out.  queued() runs when everything is on the stream, before the host waits (a stage
// clock's tick).
template <int kM, class First, class Queued = Nothing>
int reduce(const char* who, int items, void* d_ws, size_t bytes, hipStream_t st, First&& first, double* h_out, int* h_flag,
           Queued&& queued = Queued()) {
    const size_t need = ws_bytes<kM>(items);
    SG_REQUIRE(bytes >= need, "%s: workspace too small (%zu < %zu)", who, bytes, need);
    const int rows = sg::cdiv(items, kItems);
    sg::Carver cv(d_ws, bytes);
    Landing<kM>* d_land = cv.take<Landing<kM>>(1);
    double* d_partial = cv.take<double>((size_t)rows * kM);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, bytes, need);
    if (h_flag) SG_HIP(hipMemsetAsync(d_land, 0, sizeof(Landing<kM>), st));
    first(rows, d_partial, h_flag ? &d_land->flag : nullptr);
    k_fold<kM><<<1, kBlock, 0, st>>>(d_partial, rows, d_land->m);
    Landing<kM> land{};
    SG_HIP(hipMemcpyAsync(&land, d_land, sizeof(Landing<kM>), hipMemcpyDeviceToHost, st));
    queued();
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (h_flag) *h_flag = land.flag;
    if (!h_flag || !land.flag)
        for (int m = 0; m < kM; ++m) h_out[m] = land.m[m];
    return SG_OK;
}

// what the entry points of the moment kernels take from the host, checked
struct Rigid { double m[12]; };               // row-major 3x4 [R|t]
struct Origin { double c[3]; };

template <int kN>
inline bool finite_n(const double* v) {
    for (int i = 0; i < kN; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline int read_rigid(const char* who, const double* h_T, Rigid* T) {
    for (int i = 0; i < 12; ++i) {
        SG_REQUIRE(std::isfinite(h_T[i]), "%s: entry %d of the transform is not finite", who, i);
        T->m[i] = h_T[i];
    }
    return SG_OK;
}

inline Origin origin_of(const double* h) { return Origin{{h[0], h[1], h[2]}}; }

}  // namespace sgmom
