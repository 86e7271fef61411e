// A 64-bit exclusive sum over int32 counts: off[0..N] from count[0..N), off[N] = the total.  The radius lists' row
// offsets (kernels_radius.hip) and the offsets of their upper halves (kernels_pcseg.hip) are made with it; sort_device.h's scan is 32-bit.
// Three launches: the sums of tiles of 2048 counts, one block over those sums, the tiles again.  (Templates although nothing varies: the
// header is included by more than one kernel file.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sgscan {

constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanBlock * kScanItems;          // counts per block of the two tile kernels
constexpr int kSumBlock = 1024;                             // the one block that scans the tile sums: at most 2^24 / 2048 = 8192 of them

// exclusive scan of one long long per thread over the block, through LDS; *total = the block's sum (every thread)
template <int kT>
__device__ __forceinline__ long long block_exclusive(long long v, long long* __restrict__ part, long long* total) {
    const int t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (int o = 1; o < kT; o <<= 1) {
        const long long x = t >= o ? part[t - o] : 0ll;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    *total = part[kT - 1];
    return part[t] - v;
}

template <int kUnused = 0>
__global__ __launch_bounds__(kScanBlock) void k_scan64_tile_sums(const int32_t* __restrict__ count, int N, long long* __restrict__ tsum) {
    __shared__ long long part[kScanBlock];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    long long s = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) s += base + i < (size_t)N ? (long long)count[base + i] : 0ll;
    long long total;
    block_exclusive<kScanBlock>(s, part, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one block: tsum[0..ntiles) -> its exclusive scan in place; off[N] = the grand total T
template <int kUnused = 0>
__global__ __launch_bounds__(kSumBlock) void k_scan64_sums(long long* __restrict__ tsum, int ntiles, int64_t* __restrict__ off, int N) {
    __shared__ long long part[kSumBlock];
    const int per = (ntiles + kSumBlock - 1) / kSumBlock;
    const int lo = min((int)threadIdx.x * per, ntiles), hi = min(lo + per, ntiles);
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += tsum[i];
    long long total;
    long long run = block_exclusive<kSumBlock>(s, part, &total);
    for (int i = lo; i < hi; ++i) { const long long v = tsum[i]; tsum[i] = run; run += v; }
    if (threadIdx.x == 0) off[N] = (int64_t)total;
}

template <int kUnused = 0>
__global__ __launch_bounds__(kScanBlock) void k_scan64_offsets(const int32_t* __restrict__ count, int N, const long long* __restrict__ tsum,
                                                           int64_t* __restrict__ off) {
    __shared__ long long part[kScanBlock];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    long long s = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) s += base + i < (size_t)N ? (long long)count[base + i] : 0ll;
    long long total;
    long long run = tsum[blockIdx.x] + block_exclusive<kScanBlock>(s, part, &total);
#pragma unroll
    for (int i = 0; i < kScanItems; ++i)
        if (base + i < (size_t)N) { off[base + i] = (int64_t)run; run += (long long)count[base + i]; }
}

inline int tiles_of(int N) { return (N + kScanTile - 1) / kScanTile; }

// tsum: tiles_of(N) + 1 words of scratch
inline void exclusive_scan64(const int32_t* count, int N, long long* tsum, int64_t* off, hipStream_t st) {
    const int nt = tiles_of(N);
    k_scan64_tile_sums<><<<nt, kScanBlock, 0, st>>>(count, N, tsum);
    k_scan64_sums<><<<1, kSumBlock, 0, st>>>(tsum, nt, off, N);
    k_scan64_offsets<><<<nt, kScanBlock, 0, st>>>(count, N, tsum, off);
}

}  // namespace sgscan
