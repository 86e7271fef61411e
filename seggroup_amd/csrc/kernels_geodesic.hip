// Geodesic distances over a scan's graph, device side: multi-source shortest paths in double and the owning seed, by the
// two rules of include/seggroup_hip.h.  Both rules are fixed points of a monotone relaxation (fl(d + w) is monotone in d and never below d
// for w >= 0; the owner rule is a minimum of integers), so any schedule, stale reads included, ends at the same bytes.
//
//   k_gd_keys      one thread an edge row: the row is refused through the flag word (an index outside 0..V-1, a weight that is negative or
//                  not finite, a coordinate of an end that is not finite) or it gives two arcs keyed by their SOURCE vertex.  A refused row
//                  and a self loop get the key V: they sort behind every vertex and are never read again, so nothing that was refused
//                  is ever used as an index or a weight.
//   (sort_device.h) the 2E (key, arc number) pairs through the stable radix sort, over the bits of V only
//   k_gd_rows      one thread a vertex: row start = the lower bound of the vertex in the sorted keys (V + 1 entries; the last is the number
//                  of arcs kept)
//   k_gd_arcs      one thread a kept arc: its target, and its weight computed once (from the coordinates, from d_weight, or none for hops)
//   k_gd_init      D = 0 at a seed, +inf elsewhere (owner phase: O = v at a seed, INT_MAX elsewhere)
//   k_gd_relax     PULL-based, owner-writes: a workgroup of 256 threads owns a tile of 256 consecutive vertices, a thread a vertex.  The
//                  tile's values sit in LDS; up to `sweeps` inner sweeps, each a compute step (reads only: a neighbour inside the tile from
//                  LDS, one outside with a relaxed agent-scope load), a barrier, a write step, and a barrier that also says whether the tile
//                  is quiet.  A workgroup writes back only after its sweeps, so within a launch a value from another tile is new only if
//                  that workgroup has finished: the inner sweeps carry values INSIDE a tile, across tiles about one hop a launch.  A row longer than kLongRow arcs is taken by a wave with a lane minimum.  What fell is written back with
//                  a relaxed agent-scope store, and a workgroup that changed anything stores the LAUNCH NUMBER into the phase's word (a
//                  plain vector store of the same value from every such workgroup).
//   k_gd_tight     one thread a kept arc (t -> v): tight iff D(v) is finite and D(t) + w == D(v), the same double addition; the target of a
//                  tight arc stays, any other becomes -1.  The owner phase is k_gd_relax over these, on int32.
//   k_gd_finish    owner INT_MAX -> -1; the reached vertices counted (integer adds)
//
// The host enqueues `batch` launches of k_gd_relax, reads the phase's word with one 4-byte copy and repeats while the word holds the number
// of the batch's last launch.  A launch that changed nothing read nothing newer than the kernel boundary before it: a true fixed point.
// Every launch holds at least one full sweep over values no older than its start, so V + 1 launches always suffice (SG_EINTERNAL beyond).
// No cooperative launch, no device-wide barrier, no workgroup waits for another.  Double arithmetic, nothing contracted, no floating-point
// atomics; the integer atomics are the OR into the flag word and the two counters.
#include <climits>
#include <cmath>
#include <cstdlib>

#include "sg_common.h"
#include "sort_device.h"
#include "box_iou_device.h"
#include "overseg_device.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = kBlock;                  // vertices a workgroup owns: one a thread (seggroup_amd/geodesic.py TILE names it for the tests; tests/test_geodesic_ref.py holds the two together)
constexpr int kWave = 64;
constexpr int kLongRow = 128;                  // a row of more arcs is walked by a wave, not by a lane
constexpr int kSweeps = 1;                     // inner sweeps of a launch at most (a quiet tile stops earlier).  MEASURED: values cross
                                               // tiles one hop a launch, so on meshes more sweeps only cost: 1 beat 2, 4, 8, 32 and 256 on every shape
constexpr int kBatch = 8;                      // launches per host wait (measured against 1 and 32 at one sweep a launch: DESIGN.md 8x.6)
constexpr long long kMaxEdges = 1ll << 26;
constexpr int kFlagIndex = 1, kFlagWeight = 2, kFlagCoord = 4;
constexpr int kMisc = 64;                      // int32 words: flag | tight arcs | reached | arcs kept | distance word | owner word
enum { mFlag = 0, mTight = 1, mReached = 2, mArcs = 3, mDistWord = 4, mOwnerWord = 5 };

typedef unsigned int u32;

struct Edges {
    const int32_t* pairs;           // [E,2]
    long long E;
    int V;
    const float* xyz;               // rows of `stride` floats, or NULL
    int stride;
    const double* weight;           // [E], or NULL
};

__global__ __launch_bounds__(kBlock) void k_gd_keys(Edges g, u32* __restrict__ key, int32_t* __restrict__ arc, int* __restrict__ misc) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= g.E) return;
    const int a = g.pairs[2 * e], b = g.pairs[2 * e + 1];
    int bad = 0;
    if ((unsigned)a >= (unsigned)g.V || (unsigned)b >= (unsigned)g.V) bad = kFlagIndex;
    if (!bad && g.xyz) {
        const float *pa = g.xyz + (size_t)a * g.stride, *pb = g.xyz + (size_t)b * g.stride;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (!sgos::finite_f32(pa[c]) || !sgos::finite_f32(pb[c])) bad = kFlagCoord;
    }
    if (g.weight) {
        const double w = g.weight[e];
        if (!sg_box::finite_f64(w) || w < 0.0) bad |= kFlagWeight;
    }
    if (bad) atomicOr(&misc[mFlag], bad);
    const bool keep = !bad && a != b;
    key[2 * e] = keep ? (u32)a : (u32)g.V;
    key[2 * e + 1] = keep ? (u32)b : (u32)g.V;
    arc[2 * e] = (int32_t)(2 * e);              // 2E <= 2^27
    arc[2 * e + 1] = (int32_t)(2 * e + 1);
}

__global__ __launch_bounds__(kBlock) void k_gd_rows(const u32* __restrict__ key, int A, int V, int32_t* __restrict__ row, int* __restrict__ misc) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v > V) return;
    int lo = 0, hi = A;                          // the first position whose key is >= v
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < (u32)v) lo = mid + 1; else hi = mid;
    }
    row[v] = lo;
    if (v == V) misc[mArcs] = lo;
}

// position i of the sorted arcs, i < row[V]: arc number n = 2e + side leaves the row's end `side` and arrives at the other
__global__ __launch_bounds__(kBlock) void k_gd_arcs(Edges g, const int32_t* __restrict__ arc, const int32_t* __restrict__ row, int32_t* __restrict__ tgt,
                                                    double* __restrict__ w) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= row[g.V]) return;
    const int n = arc[i];
    const long long e = n >> 1;
    const int a = g.pairs[2 * e], b = g.pairs[2 * e + 1];      // both inside 0..V-1: the row was kept
    tgt[i] = (n & 1) ? a : b;
    if (g.xyz) {
        const float *pa = g.xyz + (size_t)a * g.stride, *pb = g.xyz + (size_t)b * g.stride;
        const double d0 = (double)pa[0] - (double)pb[0], d1 = (double)pa[1] - (double)pb[1], d2 = (double)pa[2] - (double)pb[2];
        w[i] = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    } else if (g.weight) {
        w[i] = g.weight[e];
    }
}

__global__ __launch_bounds__(kBlock) void k_gd_init(const int32_t* __restrict__ seed, int V, double* __restrict__ dist, int32_t* __restrict__ owner) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const bool s = seed[v] >= 0;
    dist[v] = s ? 0.0 : INFINITY;
    owner[v] = s ? v : INT_MAX;
}

template <class T>
__device__ __forceinline__ T lesser(T a, T b) { return b < a ? b : a; }

template <class T>
__device__ __forceinline__ T peer(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ double lane_min(double v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v = fmin(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ int lane_min(int v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m, kWave));
    return v;
}

// kDist: T = double, a candidate is D(t) + w (w = 1.0 without weights), taken when it is not above `limit`.
// else:  T = int32, a candidate is O(t) over the arcs whose target is not -1 (the tight ones).
template <bool kDist, class T>
__device__ __forceinline__ T candidate(const T* __restrict__ val, const T* tile, int base, int V, const int32_t* __restrict__ tgt,
                                       const double* __restrict__ w, int i, double limit, T none) {
    const int t = tgt[i];
    if constexpr (!kDist)
        if (t < 0) return none;
    const unsigned l = (unsigned)(t - base);
    const T x = l < (unsigned)kTile ? tile[l] : peer(val + t);          // 0 <= t < V: k_gd_arcs wrote ends of kept rows only
    if constexpr (kDist) {
        const double c = x + (w ? w[i] : 1.0);
        return c <= limit ? c : none;                                    // +inf stays +inf: never below what a vertex holds
    } else {
        return x;
    }
}

template <bool kDist, class T>
__global__ __launch_bounds__(kBlock) void k_gd_relax(const int32_t* __restrict__ row, const int32_t* __restrict__ tgt, const double* __restrict__ w, int V,
                                                     T* __restrict__ val, double limit, T none, int sweeps, int* __restrict__ word, int launch) {
    __shared__ T tile[kTile];
    __shared__ T lbest[kTile];                   // what a wave found for a long row
    __shared__ int longs[kTile];
    __shared__ int nlong;
    const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    const int base = blockIdx.x * kTile;
    const int v = base + t;
    const bool live = v < V;
    if (t == 0) nlong = 0;
    const T first = live ? peer(val + v) : none;
    T mine = first;
    tile[t] = mine;
    const int lo = live ? row[v] : 0, hi = live ? row[v + 1] : 0;
    const bool is_long = hi - lo > kLongRow;
    __syncthreads();
    if (is_long) longs[atomicAdd(&nlong, 1)] = t;          // < kTile entries: a thread enters once
    __syncthreads();
    const int nl = nlong;
    for (int s = 0; s < sweeps; ++s) {
        // compute: reads of the tile and of other tiles only
        T best = mine;
        if (!is_long)
            for (int i = lo; i < hi; ++i) best = lesser(best, candidate<kDist, T>(val, tile, base, V, tgt, w, i, limit, none));
        for (int k = wave; k < nl; k += kBlock / kWave) {   // uniform over the wave
            const int lt = longs[k];
            const int l0 = row[base + lt], l1 = row[base + lt + 1];
            T b = none;
            for (int i = l0 + lane; i < l1; i += kWave) b = lesser(b, candidate<kDist, T>(val, tile, base, V, tgt, w, i, limit, none));
            b = lane_min(b);
            if (lane == 0) lbest[lt] = b;
        }
        __syncthreads();
        // write: a thread its own entry
        if (is_long) best = lesser(best, lbest[t]);
        const bool fell = best < mine;
        if (fell) { mine = best; tile[t] = best; }
        if (!__syncthreads_or(fell)) break;
    }
    const bool changed = live && mine < first;
    if (changed) __hip_atomic_store(val + v, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__syncthreads_or(changed) && t == 0) *word = launch;
}

// in place over the sorted keys: position i holds its SOURCE v = key[i] (the row it lies in) and leaves the target of a tight arc, or -1
__global__ __launch_bounds__(kBlock) void k_gd_tight(const int32_t* __restrict__ row, int V, const int32_t* __restrict__ tgt, const double* __restrict__ w,
                                                     const double* __restrict__ dist, int32_t* __restrict__ key_then_tight, int* __restrict__ misc) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool tight = false;
    if (i < row[V]) {
        const int v = key_then_tight[i], t = tgt[i];         // v < V: the position lies before row[V]
        const double dv = dist[v];
        tight = dv != INFINITY && dist[t] + (w ? w[i] : 1.0) == dv;
        key_then_tight[i] = tight ? t : -1;
    }
    const int n = __popcll(__ballot(tight));
    if (n && threadIdx.x % kWave == 0) atomicAdd(&misc[mTight], n);
}

__global__ __launch_bounds__(kBlock) void k_gd_finish(int V, int32_t* __restrict__ owner, int* __restrict__ misc) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    bool reached = false;
    if (v < V) {
        reached = owner[v] != INT_MAX;
        if (!reached) owner[v] = -1;
    }
    const int n = __popcll(__ballot(reached));
    if (n && threadIdx.x % kWave == 0) atomicAdd(&misc[mReached], n);
}

bool sizes_ok(int V, long long E) { return V >= 1 && V <= SG_MAX_CLOUD_POINTS && E >= 0 && E <= kMaxEdges; }

int key_bits(int V) {                            // the keys are 0..V
    int b = 1;
    while ((1ll << b) <= (long long)V) ++b;
    return b;
}

// misc | row starts | keys x 2 | arc numbers x 2 | sort histograms | targets | weights
size_t need_bytes(int V, long long E) {
    const size_t A = (size_t)std::max(2 * E, 1ll);
    return sg::align_up(kMisc * sizeof(int)) + sg::align_up(((size_t)V + 1) * sizeof(int32_t)) + 4 * sg::align_up(A * sizeof(int32_t)) +
           sg::align_up(sgsort::hist_ints((long long)A) * sizeof(int)) + sg::align_up(A * sizeof(int32_t)) + sg::align_up(A * sizeof(double));
}

// SG_GEODESIC_SCHEDULE=S,R (read once): at most S inner sweeps a launch and R launches a host wait instead of the build's; "1,1" is the
// plain schedule, the yardstick of tools/time_geodesic.py.  The outputs do not depend on it.
struct Schedule { int sweeps, batch; };
Schedule schedule() {
    static const Schedule chosen = [] {
        Schedule s{kSweeps, kBatch};
        const char* e = std::getenv("SG_GEODESIC_SCHEDULE");
        int a = 0, b = 0;
        if (e && std::sscanf(e, "%d,%d", &a, &b) == 2 && a >= 1 && a <= 4096 && b >= 1 && b <= 256) s = Schedule{a, b};
        return s;
    }();
    return chosen;
}

thread_local int64_t t_stats[5] = {0, 0, 0, 0, 0};

// launches of k_gd_relax until one changes nothing -> the number ENQUEUED (whole batches: the launch that first changed nothing may be up to
// batch - 1 earlier), or -1 past V + 1 (and a HIP error code through *rc)
template <bool kDist, class T>
int relax_phase(const int32_t* row, const int32_t* tgt, const double* w, int V, T* val, double limit, T none, int* d_word, hipStream_t st, hipError_t* rc) {
    const int sweeps = schedule().sweeps, batch = schedule().batch;
    const int nb = sg::cdiv(V, kTile);
    const long long budget = (long long)V + 1;
    long long launches = 0;
    *rc = hipSuccess;
    for (;;) {
        const int n = (int)std::min<long long>(batch, budget - launches);
        if (n <= 0) return -1;
        for (int k = 0; k < n; ++k) {
            ++launches;
            k_gd_relax<kDist, T><<<nb, kBlock, 0, st>>>(row, tgt, w, V, val, limit, none, sweeps, d_word, (int)launches);
        }
        int word = 0;
        *rc = hipMemcpyAsync(&word, d_word, sizeof(int), hipMemcpyDeviceToHost, st);
        if (*rc != hipSuccess) return 0;
        *rc = hipStreamSynchronize(st);
        if (*rc != hipSuccess) return 0;
        if (word != (int)launches) return (int)launches;       // the batch's last launch changed nothing
    }
}

}  // namespace

extern "C" {

size_t sg_graph_geodesic_ws_bytes(int V, long long E) { return sizes_ok(V, E) ? need_bytes(V, E) : 0; }

int sg_graph_geodesic_stats(int64_t* h, int cap) {
    SG_REQUIRE(h && cap >= 5, "sg_graph_geodesic_stats: room for 5 values is needed (%d at %p)", cap, (const void*)h);
    for (int i = 0; i < 5; ++i) h[i] = t_stats[i];
    return 5;
}

int sg_graph_geodesic(const int32_t* d_edges, long long E, int V, const float* d_xyz, int stride, const double* d_weight, const int32_t* d_seed,
                      double max_dist, double* d_dist, int32_t* d_owner, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_graph_geodesic";
    SG_REQUIRE(V >= 1 && E >= 0, "%s: %d vertices and %lld edge rows", who, V, E);
    if (V > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d vertices; a graph holds at most %d", who, V, SG_MAX_CLOUD_POINTS);
    if (E > kMaxEdges) return sg::fail(SG_EUNSUP, "%s: %lld edge rows; a call takes at most 2^26", who, E);
    SG_REQUIRE(d_seed && d_dist && d_owner && d_ws && (E == 0 || d_edges), "%s: a null pointer", who);
    SG_REQUIRE(!(d_xyz && d_weight), "%s: both coordinates and weights are given; a call takes at most one of them", who);
    SG_REQUIRE(!d_xyz || stride >= 3, "%s: rows of %d floats; a point is at least 3", who, stride);
    SG_REQUIRE(max_dist >= 0.0, "%s: max_dist must be +inf or finite and >= 0 (%g)", who, max_dist);       // NaN fails the comparison
    const size_t need = need_bytes(V, E);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const size_t A = (size_t)(2 * E);
    sg::Carver cv(d_ws, ws_bytes);
    int* misc = cv.take<int>(kMisc);
    int32_t* row = cv.take<int32_t>((size_t)V + 1);
    u32* key0 = cv.take<u32>(std::max<size_t>(A, 1));
    u32* key1 = cv.take<u32>(std::max<size_t>(A, 1));
    int32_t* arc0 = cv.take<int32_t>(std::max<size_t>(A, 1));
    int32_t* arc1 = cv.take<int32_t>(std::max<size_t>(A, 1));
    int* hist = cv.take<int>(sgsort::hist_ints((long long)std::max<size_t>(A, 1)));
    int32_t* tgt = cv.take<int32_t>(std::max<size_t>(A, 1));
    double* w = cv.take<double>(std::max<size_t>(A, 1));
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    if (!d_xyz && !d_weight) w = nullptr;        // hops: every arc weighs 1.0
    for (int i = 0; i < 5; ++i) t_stats[i] = 0;

    hipStream_t st = sg::as_stream(stream);
    const int nbv = sg::cdiv(V, kBlock);
    SG_HIP(hipMemsetAsync(misc, 0, kMisc * sizeof(int), st));       // the flag word, the counters and the two phase words: one clear
    k_gd_init<<<nbv, kBlock, 0, st>>>(d_seed, V, d_dist, d_owner);
    int dist_launches = 0, owner_launches = 0;
    if (E > 0) {
        Edges g{d_edges, E, V, d_xyz, stride, d_weight};
        k_gd_keys<<<sg::cdiv(E, kBlock), kBlock, 0, st>>>(g, key0, arc0, misc);
        auto L = sgsort::one_list<u32, int32_t>(key0, key1, arc0, arc1, hist, (int)A);
        sgsort::radix_sort<u32, int32_t, true>(L, 1, 0, key_bits(V), st);
        const u32* key = L.kin[0];
        const int32_t* arc = L.vin[0];
        k_gd_rows<<<sg::cdiv((long long)V + 1, kBlock), kBlock, 0, st>>>(key, (int)A, V, row, misc);
        const int nba = sg::cdiv((long long)A, kBlock);
        k_gd_arcs<<<nba, kBlock, 0, st>>>(g, arc, row, tgt, w);
        SG_LAUNCH_CHECK();
        hipError_t rc = hipSuccess;
        dist_launches = relax_phase<true, double>(row, tgt, w, V, d_dist, max_dist, (double)INFINITY, misc + mDistWord, st, &rc);
        SG_HIP(rc);
        if (dist_launches < 0) return sg::fail(SG_EINTERNAL, "%s: the distances did not settle in %d launches", who, V + 1);
        int32_t* tight = const_cast<int32_t*>(reinterpret_cast<const int32_t*>(key));      // the sorted keys are done with after this pass
        k_gd_tight<<<nba, kBlock, 0, st>>>(row, V, tgt, w, d_dist, tight, misc);
        owner_launches = relax_phase<false, int32_t>(row, tight, nullptr, V, d_owner, 0.0, INT_MAX, misc + mOwnerWord, st, &rc);
        SG_HIP(rc);
        if (owner_launches < 0) return sg::fail(SG_EINTERNAL, "%s: the owners did not settle in %d launches", who, V + 1);
    }
    k_gd_finish<<<nbv, kBlock, 0, st>>>(V, d_owner, misc);
    int land[4] = {0, 0, 0, 0};
    SG_HIP(hipMemcpyAsync(land, misc, sizeof(land), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land[mFlag] & kFlagIndex) return sg::fail(SG_EINVAL, "%s: a vertex index outside 0..%d", who, V - 1);
    if (land[mFlag] & kFlagWeight) return sg::fail(SG_EINVAL, "%s: a weight that is negative or not finite", who);
    if (land[mFlag] & kFlagCoord) return sg::fail(SG_EINVAL, "%s: a coordinate of an edge's end is not finite", who);
    t_stats[0] = land[mArcs];
    t_stats[1] = dist_launches;
    t_stats[2] = owner_launches;
    t_stats[3] = land[mTight];
    t_stats[4] = land[mReached];
    return SG_OK;
}

}  // extern "C"
