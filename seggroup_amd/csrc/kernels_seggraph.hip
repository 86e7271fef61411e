// Segment graph of a scan: the scan's [E,2] edge list contracted through the per-vertex segment number -- the distinct
// (lo, hi) segment pairs in ascending order and, per pair, the number of scan edges behind it.  sg_contract_point_edges (kernels_graph.hip)
// answers "which pairs" with a bitmap of S * S bits (S <= 46,340, no counts, the model's first layer); this one sorts, so S goes up to
// 2^20 and memory is O(E).
//
//   k_sgg_keys        one pass over the rows: bounds of both vertices and both segment numbers (one flag word), key = lo << bits(S) | hi of
//                     every crossing row, compacted to the front of the key buffer.  On a real scan nine rows in ten lie inside one
//                     segment, so what is sorted is a tenth of the list.  A block of 256 threads takes 2,048 rows, scans its threads'
//                     counts through LDS and claims its stretch of the buffer with ONE atomic; the order the blocks land in is whatever
//                     the atomics give -- the sort and the counts below do not depend on it.
//   sort              sort_device.h's radix sort over exactly the 2 * bits(S) key bits: 32-bit keys when they fit, 64-bit otherwise
//   unique            run heads + scan (sort_device.h): the distinct keys and where their runs start
//   k_sgg_emit        pair i = (key >> bits, key & mask), cross i = the length of its run
//
// Integers only: the same bytes on every run and every stream.  The host reads the flag word and the number of crossing rows after the
// key pass (the sort's launches are sized by it) and the number of pairs at the end: two synchronisations.
#include "sg_common.h"
#include "sort_device.h"
#include "overseg_device.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 8;                        // rows per thread of the key pass
constexpr int kKeyTile = kBlock * kRows;        // 2048 rows per block
constexpr int kMaxSegments = 1 << 20;
constexpr long long kMaxRows = 1ll << 31;       // exclusive
typedef unsigned long long u64;

// flag[0] |= 1: a vertex index is outside 0..V-1; |= 2: a segment number is >= S.  flag[1] = the crossing rows so far.
template <class K>
__global__ __launch_bounds__(kBlock) void k_sgg_keys(const longlong2* __restrict__ adj, long long E, const int32_t* __restrict__ seg, int V, int S,
                                                     int bits, K* __restrict__ key, int* __restrict__ flag) {
    __shared__ int part[kBlock];
    __shared__ int s_base;
    const long long base = (long long)blockIdx.x * kKeyTile;
    K mine[kRows];
    int n = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
        const long long r = base + (long long)i * kBlock + threadIdx.x;
        mine[i] = ~(K)0;                                            // lo = hi: no crossing row makes this key
        if (r < E) {
            const longlong2 uv = adj[r];
            if (uv.x < 0 || uv.x >= V || uv.y < 0 || uv.y >= V) { bad |= 1; continue; }
            const int a = seg[uv.x], b = seg[uv.y];                 // nothing is read through an index that failed the check
            if (a >= S || b >= S) { bad |= 2; continue; }
            if (a >= 0 && b >= 0 && a != b) {
                mine[i] = ((K)(unsigned)min(a, b) << bits) | (K)(unsigned)max(a, b);
                ++n;
            }
        }
    }
    if (bad) atomicOr(flag, bad);
    part[threadIdx.x] = n;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int x = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
    if (threadIdx.x == kBlock - 1) s_base = part[kBlock - 1] ? atomicAdd(flag + 1, part[kBlock - 1]) : 0;
    __syncthreads();
    // at most E keys are written in all: one per row that crossed
    int dst = s_base + part[threadIdx.x] - n;
#pragma unroll
    for (int i = 0; i < kRows; ++i)
        if (mine[i] != ~(K)0) key[dst++] = mine[i];
}

// pair p of *d_P: its two segments and the length of its run among the M sorted keys
template <class K>
__global__ __launch_bounds__(kBlock) void k_sgg_emit(const K* __restrict__ ukey, const int* __restrict__ head, const int* __restrict__ d_P, int M,
                                                     int bits, int32_t* __restrict__ pairs, int32_t* __restrict__ cross) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int P = *d_P;
    if (p >= P) return;
    const K k = ukey[p];
    pairs[2 * (size_t)p] = (int32_t)(k >> bits);
    pairs[2 * (size_t)p + 1] = (int32_t)(k & (((K)1 << bits) - 1));
    cross[p] = (p + 1 < P ? head[p + 1] : M) - head[p];
}

// bits that hold the values 0..n-1
int bits_for(long long n) {
    int b = 0;
    while ((1ll << b) < n) ++b;
    return b;
}

size_t key_bytes(int S) { return 2 * bits_for(S) > 32 ? 8 : 4; }

struct Plan {                       // the workspace of one call
    void *k0, *k1;                  // the keys and the sort's second buffer
    int* hist;
    int* uniq;                      // unique_sorted's scratch
    int* head;                      // [E + 1] where each pair's run starts
    int* flag;                      // check flag | crossing rows | pairs
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, long long E, int S) {
    Plan p{};
    const size_t n = (size_t)std::max(E, 1ll), kb = key_bytes(S);
    sg::Carver cv(d_ws, ws_bytes);
    p.k0 = cv.take<char>(n * kb);
    p.k1 = cv.take<char>(n * kb);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    p.uniq = cv.take<int>(sgsort::unique_ints((long long)n));
    p.head = cv.take<int>(n + 1);
    p.flag = cv.take<int>(4);
    p.ok = cv.ok;
    return p;
}

constexpr int kStages = 4;
const char* const kStageNames[kStages] = {"keys", "sort", "unique", "emit"};
thread_local sgos::StageTimes<kStages> t_times;
using StageClock = sgos::StageClock<kStages>;

template <class K>
int run(const Plan& p, const int64_t* d_adj, long long E, const int32_t* d_seg, int V, int S, int32_t* d_pairs, int32_t* d_cross,
        long long* h_P, StageClock& clock, hipStream_t st) {
    const int bits = bits_for(S);
    K* k0 = static_cast<K*>(p.k0);
    K* k1 = static_cast<K*>(p.k1);
    SG_HIP(hipMemsetAsync(p.flag, 0, 16, st));
    k_sgg_keys<K><<<sg::cdiv(E, kKeyTile), kBlock, 0, st>>>(reinterpret_cast<const longlong2*>(d_adj), E, d_seg, V, S, bits, k0, p.flag);
    int flag[2] = {0, 0};
    SG_HIP(hipMemcpyAsync(flag, p.flag, 8, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (flag[0] & 1) return sg::fail(SG_EINVAL, "sg_segment_graph: a vertex index is outside 0..%d", V - 1);
    if (flag[0] & 2) return sg::fail(SG_EINVAL, "sg_segment_graph: a segment number is outside 0..%d", S - 1);
    const int M = flag[1];
    if (M < 0 || (long long)M > E) return sg::fail(SG_EHIP, "sg_segment_graph: %d crossing rows from %lld rows", M, E);
    if (M > (1 << 30)) return sg::fail(SG_EUNSUP, "sg_segment_graph: %d crossing rows; at most %d are sorted", M, 1 << 30);
    clock.tick();
    if (M == 0) {
        SG_LAUNCH_CHECK();
        return SG_OK;
    }
    auto L = sgsort::one_list<K, int>(k0, k1, nullptr, nullptr, p.hist, M);
    sgsort::radix_sort<K, int, false>(L, 1, 0, 2 * bits, st);
    clock.tick();
    K* ukey = L.kout[0];                                            // the buffer the sorted keys are not in
    sgsort::unique_sorted<K>(L.kin[0], M, ukey, p.head, p.flag + 2, p.uniq, st);
    clock.tick();
    k_sgg_emit<K><<<sg::cdiv(M, kBlock), kBlock, 0, st>>>(ukey, p.head, p.flag + 2, M, bits, d_pairs, d_cross);
    int P = 0;
    SG_HIP(hipMemcpyAsync(&P, p.flag + 2, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    clock.tick();
    SG_LAUNCH_CHECK();
    if (P < 1 || P > M) return sg::fail(SG_EHIP, "sg_segment_graph: %d pairs from %d crossing rows", P, M);
    *h_P = P;
    return SG_OK;
}

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(segment_graph, t_times, kStageNames)

size_t sg_segment_graph_ws_bytes(long long E, int S) {
    if (E < 0 || E >= kMaxRows || S < 1 || S > kMaxSegments) return 0;
    const size_t n = (size_t)std::max(E, 1ll);
    return 2 * sg::align_up(n * key_bytes(S)) + sg::align_up(sgsort::hist_ints((long long)n) * 4) +
           sg::align_up(sgsort::unique_ints((long long)n) * 4) + sg::align_up((n + 1) * 4) + 256;
}

int sg_segment_graph(const int64_t* d_adj, long long E, const int32_t* d_seg, int V, int S, int32_t* d_pairs, int32_t* d_cross, long long* h_P,
                     void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_adj && d_seg && d_pairs && d_cross && h_P && d_ws, "sg_segment_graph: null pointer");
    SG_REQUIRE((reinterpret_cast<uintptr_t>(d_adj) & 15) == 0, "sg_segment_graph: d_adj must be 16-byte aligned");
    SG_REQUIRE(E >= 0 && S >= 1 && V >= 1, "sg_segment_graph: E >= 0, S >= 1 and V >= 1 are needed (E = %lld, S = %d, V = %d)", E, S, V);
    *h_P = 0;
    if (S > kMaxSegments) return sg::fail(SG_EUNSUP, "sg_segment_graph: S = %d; at most %d segments", S, kMaxSegments);
    if (E >= kMaxRows) return sg::fail(SG_EUNSUP, "sg_segment_graph: E = %lld; fewer than %lld rows", E, kMaxRows);
    const Plan p = carve(d_ws, ws_bytes, E, S);
    if (!p.ok) return sg::fail(SG_ENOMEM, "sg_segment_graph: workspace too small (%zu < %zu)", ws_bytes, sg_segment_graph_ws_bytes(E, S));
    if (E == 0) {
        if (t_times.timing) std::fill(t_times.us, t_times.us + kStages, 0.0f);
        return SG_OK;
    }
    hipStream_t st = sg::as_stream(stream);
    StageClock clock(st, t_times.timing, t_times.us);
    return key_bytes(S) == 4 ? run<unsigned int>(p, d_adj, E, d_seg, V, S, d_pairs, d_cross, h_P, clock, st)
                             : run<u64>(p, d_adj, E, d_seg, V, S, d_pairs, d_cross, h_P, clock, st);
}

}  // extern "C"
