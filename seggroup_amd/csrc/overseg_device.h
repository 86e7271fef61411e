// What the two over-segmenters share on the device: the mesh one (kernels_overseg.hip) and the point-cloud one
// (kernels_pcseg.hip) differ in where normals and edges come from; the order of the edges -- the stable sort by (w, a, b) and the gather --
// is one piece of code, defined in kernels_overseg.hip.
#pragma once
#include "sg_common.h"

namespace sgos {

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ascending as unsigned <=> ascending as fp32, negatives included (w may be slightly negative)
__device__ __forceinline__ unsigned int weight_key(float w) {
    const unsigned bits = __float_as_uint(w);
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
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

}  // namespace sgos
