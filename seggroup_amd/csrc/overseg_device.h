// What the two over-segmenters share on the device: the mesh one (kernels_overseg.hip) and the point-cloud one
// (kernels_pcseg.hip) differ in where normals and edges come from; the order of the edges -- the stable sort by (w, a, b) and the gather --
// is one piece of code, defined in kernels_overseg.hip.
//
// Also here, for every cloud tool: weight_key and its inverse, the pieces of the bounding-box reduction that k_thin_box (kernels_thin.hip)
// and k_grid_box (grid_index_device.h) are made of, and the stage timer -- StageClock, and StageTimes behind every sg_*_set_timing /
// sg_*_stage_times / sg_*_stage_name.
#pragma once
#include <cstring>

#include "sg_common.h"

namespace sgos {

using sg::finite_f32;

// ascending as unsigned <=> ascending as fp32, negatives included (w may be slightly negative)
__device__ __forceinline__ unsigned int weight_key(float w) {
    const unsigned bits = __float_as_uint(w);
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

// weight_key's inverse on the host
inline float unkey_host(unsigned int k) {
    const unsigned int b = k & 0x80000000u ? k ^ 0x80000000u : ~k;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

constexpr float kCellLimit = 2097152.0f;        // 2^21 cells per axis: three axes share a 63-bit key

// bits that hold 0..cells-1; none for one cell.  The cells of one axis (at most 2^21) or of a whole table: both widen to long long exactly.
inline int bits_for_cells(long long cells) {
    int b = 0;
    while (b < 62 && (1ll << b) < cells) ++b;
    return b;
}

// ---- The bounding box of a cloud as weight_key words, order-free.  A fixed number of blocks walks the cloud: every thread keeps its own
// minima and maxima, a wave folds them by shuffles, the block's waves meet in LDS, and three threads of the block go to memory -- 6
// atomics per block, 6 * kBoxBlocks per call whatever N is.  (One atomic per wave and axis, as k_pc_pack has them, was 85 % of
// sg_cloud_thin at 1 M points: 100,000 atomics on six words.)  A kernel declares s_lo / s_hi, calls box_take per point, box_stage once,
// __syncthreads(), box_commit.
constexpr int kBoxBlock = 256;
constexpr int kBoxBlocks = 1024;                // blocks of a box kernel: four per CU
constexpr int kBoxWaves = kBoxBlock / 64;

struct Box {
    unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    bool bad = false;                           // a coordinate is not finite
};

__device__ __forceinline__ void box_take(Box& b, const float (&c)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.bad |= !finite_f32(c[a]);
        const unsigned int key = weight_key(c[a]);
        b.lo[a] = min(b.lo[a], key);
        b.hi[a] = max(b.hi[a], key);
    }
}

// the flag word, the wave's fold, its lane 0 into LDS; the caller's barrier follows
__device__ __forceinline__ void box_stage(Box& b, int* __restrict__ flag, unsigned int (*s_lo)[kBoxWaves], unsigned int (*s_hi)[kBoxWaves]) {
    if (b.bad) atomicOr(flag, 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            b.lo[a] = min(b.lo[a], (unsigned int)__shfl_xor((int)b.lo[a], off));
            b.hi[a] = max(b.hi[a], (unsigned int)__shfl_xor((int)b.hi[a], off));
        }
        if (lane == 0) { s_lo[a][wave] = b.lo[a]; s_hi[a][wave] = b.hi[a]; }
    }
}

// after the barrier: thread a < 3 folds the waves of axis a and goes to memory
__device__ __forceinline__ void box_commit(const unsigned int (*s_lo)[kBoxWaves], const unsigned int (*s_hi)[kBoxWaves],
                                           unsigned int* __restrict__ lo, unsigned int* __restrict__ hi) {
    if (threadIdx.x >= 3) return;
    const int a = threadIdx.x;
    unsigned int l = s_lo[a][0], h = s_hi[a][0];
#pragma unroll
    for (int w = 1; w < kBoxWaves; ++w) { l = min(l, s_lo[a][w]); h = max(h, s_hi[a][w]); }
    atomicMin(&lo[a], l);
    atomicMax(&hi[a], h);
}

// 8d step 5 on the device.  k0 / v0 hold the keys (weight_key) and the indices 0..E-1 of the lexicographic edge list; k1 / v1 are second
// buffers of the same size, hist holds sgsort::hist_ints(E) ints.  -> the edge indices in ascending (w, a, b): a stable sort over the
// key's 32 bits.
const int* sort_by_weight(unsigned int* k0, unsigned int* k1, int* v0, int* v1, int* hist, int E, hipStream_t st);
// (a, b, w) of the lexicographic list adj [E,2] int64 / w [E] in the order idx names
void gather_edges(const int* idx, int E, const int64_t* adj, const float* w, int32_t* edges, float* w_sorted, hipStream_t st);

// Stage times by events: a call that is timed (the thread asked through sg_*_set_timing) brackets its stages with tick(); the
// destructor leaves the microseconds in us[0..kStages).
template <int kStages>
struct StageClock {
    hipEvent_t ev[kStages + 1];
    int made = 0, next = 0;
    hipStream_t st;
    float* us;
    StageClock(hipStream_t s, bool on, float* out) : st(s), us(out) {
        if (!on) return;
        for (int i = 0; i < kStages; ++i) us[i] = 0.0f;
        for (; made <= kStages; ++made)
            if (hipEventCreate(&ev[made]) != hipSuccess) break;
        if (made <= kStages) { drop(); return; }
        tick();
    }
    void tick() { if (made && next <= kStages) (void)hipEventRecord(ev[next++], st); }     // the end of stage next - 1
    void drop() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]); made = 0; }
    ~StageClock() {
        if (!made) return;
        if (next > 1 && hipEventSynchronize(ev[next - 1]) == hipSuccess)
            for (int i = 1; i < next; ++i) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, ev[i - 1], ev[i]) == hipSuccess) us[i - 1] = ms * 1000.0f;
            }
        drop();
    }
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
};

// What a thread asked for through sg_*_set_timing and what its last timed call left: one per family, thread_local
template <int kStages>
struct StageTimes {
    bool timing = false;
    float us[kStages];
    int copy(const char* who, float* h_us, int cap) const {        // sg_*_stage_times -> the number of stages
        SG_REQUIRE(h_us && cap >= kStages, "%s: room for %d floats is needed", who, kStages);
        for (int i = 0; i < kStages; ++i) h_us[i] = us[i];
        return kStages;
    }
};

template <int kStages>
const char* stage_name(const char* const (&names)[kStages], int i) { return i >= 0 && i < kStages ? names[i] : nullptr; }

// sg_<family>_set_timing / _stage_times / _stage_name over the family's StageTimes object and its names, inside an extern "C" block; a
// refusal names the symbol it came from by construction
#define SG_STAGE_TIMER_API(family, times, names)                                                                              \
    int sg_##family##_set_timing(int on) { (times).timing = on != 0; return SG_OK; }                                         \
    int sg_##family##_stage_times(float* h_us, int cap) { return (times).copy("sg_" #family "_stage_times", h_us, cap); }    \
    const char* sg_##family##_stage_name(int i) { return sgos::stage_name(names, i); }

}  // namespace sgos
