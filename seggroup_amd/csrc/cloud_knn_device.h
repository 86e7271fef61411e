// Whole-cloud brute-force kNN, the part that kernels_prepare.hip (sg_nearest_point, sg_pointcloud_adjacency) and kernels_pcseg.hip
// (sg_pointcloud_knn) share: the reference's exact fp32 score and the top-KK selection with its tie rule.  One definition, so the kNN
// graph that get_adj_from_pointcloud writes and the table the point-cloud segmenter walks cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

namespace sgcloud {

constexpr int kTile = 256;      // candidates staged per LDS tile = queries per block

// score of candidate c = (x, y, z, yy) for the query (qx, qy, qz) with squared norm qq, in the reference's order
__device__ inline float pair_score(float qx, float qy, float qz, float qq, const float4& c) {
    const float tt = __builtin_fmaf(qz, c.z, __builtin_fmaf(qy, c.y, qx * c.x));      // MKL's K=3 dot product
    const float inner = -2.0f * tt;
    return ((-qq) - inner) - c.w;
}

// (x, y, z) -> (x, y, z, (x*x + y*y) + z*z): torch.sum(y**2, dim=1)
__device__ inline float4 with_norm(float x, float y, float z) { return make_float4(x, y, z, (x * x + y * y) + z * z); }

// The KK best-scoring candidates of the query `me` among cand[0..N): descending score, the lower index first among equal scores
// (candidates arrive in ascending index and `>` keeps the earlier one).  Every thread of the block takes part (the tile is staged by all
// of them); bs / bi are the caller's registers: the loops over them are unrolled, nothing is indexed at run time.
template <int KK>
__device__ __forceinline__ void top_scores(const float4* __restrict__ cand, int N, const float4 me, float4* tile, float (&bs)[KK],
                                           int (&bi)[KK]) {
#pragma unroll
    for (int t = 0; t < KK; ++t) { bs[t] = -INFINITY; bi[t] = 0x7fffffff; }
    for (int c0 = 0; c0 < N; c0 += kTile) {
        __syncthreads();
        tile[threadIdx.x] = c0 + threadIdx.x < N ? cand[c0 + threadIdx.x] : make_float4(0.f, 0.f, 0.f, INFINITY);
        __syncthreads();
        const int m = min(kTile, N - c0);
        for (int j = 0; j < m; ++j) {
            const float sc = pair_score(me.x, me.y, me.z, me.w, tile[j]);
            if (sc > bs[KK - 1]) {                             // candidates arrive in ascending index: `>` keeps the earlier one of a tie
                float v = sc;
                int id = c0 + j;
                bool placed = false;
#pragma unroll
                for (int t = 0; t < KK; ++t) {
                    if (placed || v > bs[t]) {
                        placed = true;
                        const float tv = bs[t]; const int ti = bi[t];
                        bs[t] = v; bi[t] = id; v = tv; id = ti;
                    }
                }
            }
        }
    }
}

// kernels_prepare.hip: sg_nearest_point's kernel for the queries qid[0..U) (rows of qxyz; the identity when qid is null) against
// cand[0..N) = with_norm(y); out[scatter ? row : u] = the best-scoring candidate, the lowest index among equal scores
void launch_nearest(const float* qxyz, int qstride, const int32_t* qid, int U, const float4* cand, int N, int64_t* out, int scatter,
                    hipStream_t st);

}  // namespace sgcloud
