// The triple of a RANSAC hypothesis, written once for k_ransac_filter / k_ransac_count (kernels_register.hip) and
// k_pl_generate (kernels_planes.hip).  register.py restates the draw on the host, independently.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sgdraw {

// t[0..3) of hypothesis h over C candidates, 3 <= C <= 2^24: the caller's row, or index e = ((z >> 32) * C) >> 32 of
// z = splitmix64(seed + (3h + e + 1) * golden).  false: a caller's entry outside 0..C-1 -- nothing may be read through t.
// *distinct: the three indices differ.
__device__ __forceinline__ bool triple_of(int h, const int32_t* __restrict__ triples, unsigned long long seed, int C, int* t, bool* distinct) {
    bool ok = true;
    if (triples) {
        for (int e = 0; e < 3; ++e) {
            t[e] = triples[(size_t)h * 3 + e];
            ok = ok && (unsigned)t[e] < (unsigned)C;
        }
    } else {
        for (int e = 0; e < 3; ++e) {
            unsigned long long z = seed + (3ull * (unsigned long long)h + (unsigned long long)e + 1ull) * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            t[e] = (int)(((z >> 32) * (unsigned long long)C) >> 32);
        }
    }
    *distinct = t[0] != t[1] && t[1] != t[2] && t[0] != t[2];
    return ok;
}

}  // namespace sgdraw
