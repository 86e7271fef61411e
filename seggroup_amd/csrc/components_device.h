// What the connected-components entry points (kernels_components.hip) and the radius graph (kernels_radius.hip, 8k) share on
// the device: the parent array's hook with its step budget and flag word, and the init, flatten and sizes launches.  The invariant and the
// proof that one pass over the pairs is enough are written out at the head of kernels_components.hip; only the source of the pairs differs.
#pragma once
#include "sg_common.h"

namespace sgcc {
namespace {

constexpr int kBlock = 256;

enum : int { kFlagIndex = 1, kFlagCoord = 2, kFlagBudget = 4 };

struct Misc {
    int flag;                       // kFlag* bits
    int roots;                      // #{v : comp[v] == v}
};

__device__ __forceinline__ int load_parent(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x's root as far as this thread can see it, halving the path on the way.  Every step goes to a lower index; `budget` counts them.
__device__ __forceinline__ int find_halving(int* parent, int x, int& budget) {
    while (budget > 0) {
        const int p = load_parent(parent, x);
        if (p == x) return x;
        const int g = load_parent(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // x is not a root: g < p < x
        x = g;
        --budget;
    }
    return x;
}

__device__ __forceinline__ void hook(int* parent, int a, int b, int V, Misc* m) {
    int budget = 2 * V + 4;                      // V <= 2^27
    a = find_halving(parent, a, budget);
    b = find_halving(parent, b, budget);
    while (a != b && budget > 0) {
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        --budget;                                // hi was hooked by somebody else: old < hi is its parent now
        a = find_halving(parent, old, budget);
        b = find_halving(parent, lo, budget);
    }
    if (a != b) atomicOr(&m->flag, kFlagBudget);
}

__global__ __launch_bounds__(kBlock) void k_cc_init(int* __restrict__ parent, int* __restrict__ count, int V, Misc* __restrict__ m) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v == 0) { m->flag = 0; m->roots = 0; }
    if (v < V) { parent[v] = v; count[v] = 0; }
}

// After the hooks: parent is final, plain loads.  The lanes of a wave that share a root add once, through the lowest of them.
__global__ __launch_bounds__(kBlock) void k_cc_flatten(const int* __restrict__ parent, int V, int32_t* __restrict__ comp, int* __restrict__ count,
                                                       Misc* __restrict__ m) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = v < V;
    int r = -1;
    if (live) {
        r = v;
        int budget = V;
        for (int p = parent[r]; p != r && budget > 0; p = parent[r], --budget) r = p;
        if (parent[r] != r) atomicOr(&m->flag, kFlagBudget);
        comp[v] = r;
        if (r == v) atomicAdd(&m->roots, 1);
    }
    if (!count) return;
    bool todo = live;
    for (int it = 0; it < 64; ++it) {            // at most 64 different roots in a wave
        const unsigned long long open = __ballot(todo);
        if (!open) break;
        const int leader = __ffsll((long long)open) - 1;
        const int lr = __shfl(r, leader);
        const bool same = todo && r == lr;
        const int n = __popcll(__ballot(same));
        if (lane == leader) atomicAdd(count + lr, n);
        if (same) todo = false;
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_sizes(const int32_t* __restrict__ comp, const int* __restrict__ count, int V,
                                                     int32_t* __restrict__ size) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v < V) size[v] = count[comp[v]];
}

}  // namespace
}  // namespace sgcc
