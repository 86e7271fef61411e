// Segment vote: every vertex carries a row id (any non-negative int32) and a column (0..n_cols-1); per distinct row id
// the column held by the most of its vertices, ties to the lowest column.  Re-keying a scan's annotations onto another over-segmentation
// is two such votes (rekey.py): rows = new segments, columns = annotation groups; rows = source segments, columns = new segments.
//
//   k_rk_check        ids >= 0, columns inside 0..n_cols-1 (one flag word), the largest id (one atomic per wave)
//   rank              stable radix sort of (id, vertex) over exactly the id bits in use (sort_device.h), run heads + scan:
//                     the distinct ids ascending, their vertex counts, rank[v] = position of v's id among them
//   pairs             key = rank << column bits | column, value = vertex, stable sort over rank bits + column bits -- 32-bit keys when
//                     they fit, 64-bit keys otherwise; run heads + scan: the distinct (row, column) pairs and their run lengths
//   arg-max           one thread per pair: atomicMax of (run length << 32 | ~pair index) on its row's word -- the longest run, the lowest
//                     column among equals (pairs ascend with the column inside a row); integers only, the result is the same whatever the
//                     order the atomics land in.  Then per row: winner, its count, the number of pairs, the lowest vertex of the winning
//                     run (the sort is stable, values ascend inside a run); per pair: the tied flag
//   k_rk_vertex       winner of every vertex's row
//
// Memory is O(V): there is no rows x columns table anywhere (seg_min_verts = 1 gives rows ~ V, and the second vote's columns are segments).
#include "sg_common.h"
#include "sort_device.h"
#include "overseg_device.h"

namespace {

constexpr int kBlock = 256;
typedef unsigned long long u64;

// flag[0] |= 1: an id is negative; |= 2: a column is outside 0..n_cols-1; flag[1] = the largest id
__global__ __launch_bounds__(kBlock) void k_rk_check(const int32_t* __restrict__ ids, const int32_t* __restrict__ cols, int V, int n_cols,
                                                     int* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int bad = 0, id = 0;
    if (i < V) {
        id = ids[i];
        if (id < 0) { bad |= 1; id = 0; }
        if (cols) {
            const int c = cols[i];
            if (c < 0 || c >= n_cols) bad |= 2;
        }
    }
    for (int off = 32; off > 0; off >>= 1) id = max(id, __shfl_xor(id, off));      // every lane of the block is here
    if ((threadIdx.x & 63) == 0 && id > 0) atomicMax(flag + 1, id);
    if (bad) atomicOr(flag, bad);
}

__global__ __launch_bounds__(kBlock) void k_rk_id_keys(const int32_t* __restrict__ ids, int V, unsigned int* __restrict__ key,
                                                       int* __restrict__ val) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    key[i] = (unsigned)ids[i];
    val[i] = i;
}

// sorted position i -> the rank of its id: the scanned head flags count the heads in front of i (unique_sorted's scratch layout)
__global__ __launch_bounds__(kBlock) void k_rk_rank(const unsigned int* __restrict__ skey, const int* __restrict__ sval, const int* __restrict__ pos,
                                                    const int* __restrict__ tile_sum, int V, int32_t* __restrict__ rank) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    const bool head = i == 0 || skey[i] != skey[i - 1];
    rank[sval[i]] = pos[i] + tile_sum[i / sgsort::kTile] - (head ? 0 : 1);
}

__global__ __launch_bounds__(kBlock) void k_rk_row_counts(const int* __restrict__ head, int R, int V, int32_t* __restrict__ count) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= R) return;
    count[r] = (r + 1 < R ? head[r + 1] : V) - head[r];
}

template <class K>
__global__ __launch_bounds__(kBlock) void k_rk_pair_keys(const int32_t* __restrict__ rank, const int32_t* __restrict__ cols, int V, int cbits,
                                                         K* __restrict__ key, int* __restrict__ val) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    key[v] = ((K)(unsigned)rank[v] << cbits) | (K)(unsigned)cols[v];
    val[v] = v;
}

// pair p of *d_P: the first pair of its row notes where the row starts; every pair bids for its row
template <class K>
__global__ __launch_bounds__(kBlock) void k_rk_bid(const K* __restrict__ pkey, const int* __restrict__ phead, const int* __restrict__ d_P, int V,
                                                   int R, int cbits, int* __restrict__ row_start, u64* __restrict__ best) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int P = *d_P;
    if (p >= P) return;
    const int row = (int)(pkey[p] >> cbits);
    if (p == 0 || (int)(pkey[p - 1] >> cbits) != row) row_start[row] = p;
    if (p == 0) row_start[R] = P;
    const int len = (p + 1 < P ? phead[p + 1] : V) - phead[p];
    atomicMax(&best[row], ((u64)(unsigned)len << 32) | (u64)(~(unsigned)p));
}

template <class K>
__global__ __launch_bounds__(kBlock) void k_rk_rows(const K* __restrict__ pkey, const int* __restrict__ phead, const int* __restrict__ sval,
                                                    const int* __restrict__ row_start, const u64* __restrict__ best,
                                                    const int* __restrict__ d_P, int R, int cbits, int32_t* __restrict__ winner,
                                                    int32_t* __restrict__ winner_count, int32_t* __restrict__ distinct,
                                                    int32_t* __restrict__ first_vertex) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= R) return;
    const u64 b = best[r];
    const int p = (int)~(unsigned)b;
    if (p < 0 || p >= *d_P) {                                          // cannot happen: every row holds a pair; nothing is read through it
        winner[r] = winner_count[r] = distinct[r] = first_vertex[r] = -1;
        return;
    }
    const K cmask = ((K)1 << cbits) - 1;
    winner[r] = (int32_t)(pkey[p] & cmask);
    winner_count[r] = (int32_t)(b >> 32);
    distinct[r] = row_start[r + 1] - row_start[r];
    first_vertex[r] = sval[phead[p]];
}

// a pair as long as its row's winner that is not the winner: the row is tied (every writer stores the same 1)
template <class K>
__global__ __launch_bounds__(kBlock) void k_rk_tied(const K* __restrict__ pkey, const int* __restrict__ phead, const int* __restrict__ d_P, int V,
                                                    int cbits, const u64* __restrict__ best, int32_t* __restrict__ tied) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int P = *d_P;
    if (p >= P) return;
    const int row = (int)(pkey[p] >> cbits);
    const unsigned len = (unsigned)((p + 1 < P ? phead[p + 1] : V) - phead[p]);
    const u64 b = best[row];
    if (len == (unsigned)(b >> 32) && p != (int)~(unsigned)b) tied[row] = 1;
}

__global__ __launch_bounds__(kBlock) void k_rk_vertex(const int32_t* __restrict__ rank, const int32_t* __restrict__ winner, int V,
                                                      int32_t* __restrict__ vertex_winner) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    vertex_winner[v] = winner[rank[v]];
}

// bits that hold the values 0..n-1
int bits_for(long long n) {
    int b = 0;
    while ((1ll << b) < n) ++b;
    return b;
}

struct Plan {                       // the workspace of one call
    u64 *k0, *k1;                   // sort keys: the ids (as 32-bit words), then the (rank, column) pairs
    int *v0, *v1;                   // the vertices that travel with them
    int* hist;
    int* uniq;                      // unique_sorted's scratch: [V] scanned head flags | tile sums
    int* row_head;                  // [V + 1] where each id's run starts
    u64* pkey;                      // [V] the distinct pairs
    int* phead;                     // [V + 1] where each pair's run starts
    int* row_start;                 // [V + 1] the first pair of each row
    u64* best;                      // [V] run length << 32 | ~pair index
    int* flag;                      // check flag | largest id | rows | pairs
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, int V) {
    Plan p{};
    const size_t n = (size_t)std::max(V, 1);
    sg::Carver cv(d_ws, ws_bytes);
    p.k0 = cv.take<u64>(n);
    p.k1 = cv.take<u64>(n);
    p.v0 = cv.take<int>(n);
    p.v1 = cv.take<int>(n);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    p.uniq = cv.take<int>(sgsort::unique_ints((long long)n));
    p.row_head = cv.take<int>(n + 1);
    p.pkey = cv.take<u64>(n);
    p.phead = cv.take<int>(n + 1);
    p.row_start = cv.take<int>(n + 1);
    p.best = cv.take<u64>(n);
    p.flag = cv.take<int>(4);
    p.ok = cv.ok;
    return p;
}

// sg_segment_vote_set_timing(1): the calling thread's next calls bracket their stages with events (tools/time_rekey.py), through
// overseg_device.h's StageTimes and StageClock
constexpr int kStages = 7;
const char* const kStageNames[kStages] = {"check", "rank_sort", "rank_unique", "pair_sort", "pair_unique", "arg_max", "vertex_gather"};
thread_local sgos::StageTimes<kStages> t_times;
using StageClock = sgos::StageClock<kStages>;

// stages 0-2: the check and the ranks.  -> *h_R rows; p.row_head holds the runs' starts
int rank_stage(const char* who, const Plan& p, const int32_t* d_ids, const int32_t* d_cols, int V, int n_cols, int32_t* d_rank,
               int32_t* d_row_ids, int32_t* d_row_count, int* h_R, StageClock& clock, hipStream_t st) {
    // 0. the arrays are the caller's: nothing is indexed by an id or a column before this check has passed
    SG_HIP(hipMemsetAsync(p.flag, 0, 16, st));
    k_rk_check<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_ids, d_cols, V, n_cols, p.flag);
    int flag[2] = {0, 0};
    SG_HIP(hipMemcpyAsync(flag, p.flag, 8, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (flag[0] & 1) return sg::fail(SG_EINVAL, "%s: a row id is negative", who);
    if (flag[0] & 2) return sg::fail(SG_EINVAL, "%s: a column is outside 0..%d", who, n_cols - 1);
    clock.tick();
    // 1. (id, vertex) sorted by id over the bits the largest id uses
    unsigned int* k0 = reinterpret_cast<unsigned int*>(p.k0);
    unsigned int* k1 = reinterpret_cast<unsigned int*>(p.k1);
    k_rk_id_keys<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_ids, V, k0, p.v0);
    auto L = sgsort::one_list<unsigned int, int>(k0, k1, p.v0, p.v1, p.hist, V);
    sgsort::radix_sort<unsigned int, int, true>(L, 1, 0, bits_for((long long)flag[1] + 1), st);
    clock.tick();
    // 2. the distinct ids, where their runs start, every vertex's rank
    sgsort::unique_sorted<unsigned int>(L.kin[0], V, reinterpret_cast<unsigned int*>(d_row_ids), p.row_head, p.flag + 2, p.uniq, st);
    k_rk_rank<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(L.kin[0], L.vin[0], p.uniq, p.uniq + V, V, d_rank);
    int R = 0;
    SG_HIP(hipMemcpyAsync(&R, p.flag + 2, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (R < 1 || R > V) return sg::fail(SG_EHIP, "%s: %d rows from %d vertices", who, R, V);
    k_rk_row_counts<<<sg::cdiv(R, kBlock), kBlock, 0, st>>>(p.row_head, R, V, d_row_count);
    clock.tick();
    SG_LAUNCH_CHECK();
    *h_R = R;
    return SG_OK;
}

// stages 3-6 with keys of type K
template <class K>
int pair_stages(const Plan& p, const int32_t* d_rank, const int32_t* d_cols, int V, int R, int rbits, int cbits, int32_t* d_winner,
                int32_t* d_winner_count, int32_t* d_distinct, int32_t* d_tied, int32_t* d_first_vertex, int32_t* d_vertex_winner,
                StageClock& clock, hipStream_t st) {
    K* k0 = reinterpret_cast<K*>(p.k0);
    K* k1 = reinterpret_cast<K*>(p.k1);
    K* pkey = reinterpret_cast<K*>(p.pkey);
    k_rk_pair_keys<K><<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_rank, d_cols, V, cbits, k0, p.v0);
    auto L = sgsort::one_list<K, int>(k0, k1, p.v0, p.v1, p.hist, V);
    sgsort::radix_sort<K, int, true>(L, 1, 0, rbits + cbits, st);
    clock.tick();
    sgsort::unique_sorted<K>(L.kin[0], V, pkey, p.phead, p.flag + 3, p.uniq, st);
    clock.tick();
    SG_HIP(hipMemsetAsync(p.best, 0, (size_t)R * 8, st));
    SG_HIP(hipMemsetAsync(d_tied, 0, (size_t)R * 4, st));
    k_rk_bid<K><<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(pkey, p.phead, p.flag + 3, V, R, cbits, p.row_start, p.best);
    k_rk_rows<K><<<sg::cdiv(R, kBlock), kBlock, 0, st>>>(pkey, p.phead, L.vin[0], p.row_start, p.best, p.flag + 3, R, cbits, d_winner,
                                                         d_winner_count, d_distinct, d_first_vertex);
    k_rk_tied<K><<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(pkey, p.phead, p.flag + 3, V, cbits, p.best, d_tied);
    clock.tick();
    k_rk_vertex<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_rank, d_winner, V, d_vertex_winner);
    clock.tick();
    SG_LAUNCH_CHECK();
    return SG_OK;
}

constexpr int kMaxVertices = 1 << 30;

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(segment_vote, t_times, kStageNames)

size_t sg_segment_vote_ws_bytes(int V) {
    const size_t n = (size_t)std::max(V, 1);
    return 4 * sg::align_up(n * 8) + 2 * sg::align_up(n * 4) + 3 * sg::align_up((n + 1) * 4) + sg::align_up(sgsort::hist_ints((long long)n) * 4) +
           sg::align_up(sgsort::unique_ints((long long)n) * 4) + 256;
}

int sg_segment_rank(const int32_t* d_ids, int V, int32_t* d_rank, int32_t* d_row_ids, int32_t* d_row_count, int* h_R, void* d_ws,
                    size_t ws_bytes, void* stream) {
    SG_REQUIRE(V > 0 && V <= kMaxVertices && d_ids && d_rank && d_row_ids && d_row_count && h_R && d_ws, "sg_segment_rank: bad arguments");
    *h_R = 0;
    const Plan p = carve(d_ws, ws_bytes, V);
    if (!p.ok) return sg::fail(SG_ENOMEM, "sg_segment_rank: workspace too small (%zu < %zu)", ws_bytes, sg_segment_vote_ws_bytes(V));
    hipStream_t st = sg::as_stream(stream);
    StageClock clock(st, t_times.timing, t_times.us);
    return rank_stage("sg_segment_rank", p, d_ids, nullptr, V, 1, d_rank, d_row_ids, d_row_count, h_R, clock, st);
}

int sg_segment_vote(const int32_t* d_ids, const int32_t* d_cols, int V, int n_cols, int32_t* d_rank, int32_t* d_vertex_winner,
                    int32_t* d_row_ids, int32_t* d_row_count, int32_t* d_winner, int32_t* d_winner_count, int32_t* d_distinct, int32_t* d_tied,
                    int32_t* d_first_vertex, int* h_R, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(V > 0 && V <= kMaxVertices && n_cols >= 1 && d_ids && d_cols && d_rank && d_vertex_winner && d_row_ids && d_row_count &&
                   d_winner && d_winner_count && d_distinct && d_tied && d_first_vertex && h_R && d_ws,
               "sg_segment_vote: bad arguments");
    *h_R = 0;
    const Plan p = carve(d_ws, ws_bytes, V);
    if (!p.ok) return sg::fail(SG_ENOMEM, "sg_segment_vote: workspace too small (%zu < %zu)", ws_bytes, sg_segment_vote_ws_bytes(V));
    hipStream_t st = sg::as_stream(stream);
    StageClock clock(st, t_times.timing, t_times.us);
    int R = 0;
    const int rc = rank_stage("sg_segment_vote", p, d_ids, d_cols, V, n_cols, d_rank, d_row_ids, d_row_count, &R, clock, st);
    if (rc < 0) return rc;
    const int rbits = bits_for(R), cbits = bits_for(n_cols);
    const int rc2 = rbits + cbits <= 32
                        ? pair_stages<unsigned int>(p, d_rank, d_cols, V, R, rbits, cbits, d_winner, d_winner_count, d_distinct, d_tied,
                                                    d_first_vertex, d_vertex_winner, clock, st)
                        : pair_stages<u64>(p, d_rank, d_cols, V, R, rbits, cbits, d_winner, d_winner_count, d_distinct, d_tied, d_first_vertex,
                                           d_vertex_winner, clock, st);
    if (rc2 < 0) return rc2;
    *h_R = R;
    return SG_OK;
}

}  // extern "C"
