// The second tree of the deterministic moment sums: one workgroup folds the partial rows that the moment kernels
// of kernels_align.hip and kernels_planes.hip leave, one row of kM doubles per workgroup of theirs.  Thread t adds rows t, t + 256, .. in
// order, a wave sums on the DPP network of wave_ops.h, the four waves' sums are added in order: a function of `rows` alone.  (In a
// header because two kernel files launch it; each gets its own copy.)
#pragma once
#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace sgmom {

constexpr int kFoldBlock = 256;
constexpr int kFoldWaves = kFoldBlock / 64;

template <int kM>
__global__ __launch_bounds__(kFoldBlock) void k_align_fold(const double* __restrict__ partial, int rows, double* __restrict__ out) {
    __shared__ double s_rows[kFoldWaves][kM];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll 1
    for (int m = 0; m < kM; ++m) {
        double acc = 0.0;
        for (int r = threadIdx.x; r < rows; r += kFoldBlock) acc += partial[(size_t)r * kM + m];
        const double s = sgw::wave_sum(acc);
        if (lane == 0) s_rows[wave][m] = s;
    }
    __syncthreads();
    if (threadIdx.x < kM) {
        double s = s_rows[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kFoldWaves; ++w) s += s_rows[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

}  // namespace sgmom
