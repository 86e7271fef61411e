// The V-sized part of the ScanNet instance AP evaluation: per scene, the contingency of label slots against ground-truth
// instances, compacted to (slot, g, count) triples.  A vertex's label in every layer is tables[row][seg_of_vertex[v]], so ONE pass over the
// vertices serves every layer; the S-sized arithmetic (instances, matching) is host work (csrc/ap.cpp).
//   k_ap_gt_count     count[gt_id] += 1 over the 41,000 possible ids (gt_id = sem*1000 + ins where ins > 0, else 0); refuses bad labels
//   k_ap_gt_index     the table in place: count -> dense index g (0 = id 0), the scene's sorted (id, count) list (direct-indexed: no sort)
//   k_ap_contingency  C[slot(v)][g(v)] += 1 and first_vertex[slot] = min v; slot = the vertex's segment (S without one), or its instance value
//   k_ap_chunk_count / k_ap_chunk_scan / k_ap_compact   the non-zero cells of C in (slot, g) order
// Integer atomics only: the same bytes on every run.  Mesh order makes neighbouring vertices share (slot, g); equal keys of neighbouring lanes
// are merged (DPP row_shr:1 + ballot) so that one lane of a run issues the atomic with the run's length.
// No pointer is loaded from a descriptor here (descriptors hold offsets; the bases are kernel arguments, which the compiler knows are global).
#include "sg_common.h"

namespace {

constexpr int kApIds = 41000;            // sem 0..40, ins 0..999
constexpr int kApIdsPad = 41984;         // 1024 threads x 41 ids
constexpr int kApBlock = 256;
constexpr int kApChunk = 2048;           // cells of C per block of the compaction kernels (8 per thread)

struct ApScene { long long sov_off, V, gt_off, S, G, c_off, first_off, chunk_off, trip_off, nchunks; };

template <int W>
__device__ __forceinline__ int ap_slot(const void* __restrict__ src, long long i, int S, bool& bad) {
    if constexpr (W == 2) {
        const uint16_t u = reinterpret_cast<const uint16_t*>(src)[i];
        return u < S ? (int)u : S;
    } else if constexpr (W == 4) {
        const int x = reinterpret_cast<const int32_t*>(src)[i];
        return (x >= 0 && x < S) ? x : S;
    } else {                             // an instance vector: values <= 0 share slot 0, S is the largest value
        const int x = reinterpret_cast<const int32_t*>(src)[i];
        bad = x > S;
        return (x > 0 && x <= S) ? x : 0;
    }
}

// a lane is the head of a run when its key differs from the lane below it in its row of 16 (row_shr:1; a row's first lane takes ~key: always
// a head); len = lanes up to the next head.  All 64 lanes must be active.
__device__ __forceinline__ bool run_head(uint32_t key, int lane, int& len) {
    const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)~key, (int)key, 0x111, 0xF, 0xF, false);
    const bool head = prev != key;
    const unsigned long long m = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : (m >> (lane + 1));
    len = above ? __ffsll(above) : 64 - lane;
    return head;
}

__device__ __forceinline__ uint32_t gt_id_of(int2 g, bool& bad) {
    bad = (unsigned)g.x > 40u || g.y >= 1000;
    return (bad || g.y <= 0) ? 0u : (uint32_t)(g.x * 1000 + g.y);
}

template <bool MERGE>
__global__ __launch_bounds__(kApBlock) void k_ap_gt_count(const ApScene* __restrict__ desc, const int32_t* __restrict__ gt_all,
                                                           uint32_t* __restrict__ cnt_all, uint32_t* __restrict__ err) {
    const ApScene d = desc[blockIdx.y];
    const int V = (int)d.V, lane = threadIdx.x & 63;
    const int2* gt = reinterpret_cast<const int2*>(gt_all) + d.gt_off;
    uint32_t* cnt = cnt_all + (size_t)blockIdx.y * kApIdsPad;
    bool any_bad = false;
    for (int v0 = blockIdx.x * kApBlock + (threadIdx.x & ~63); v0 < V; v0 += gridDim.x * kApBlock) {
        const int v = v0 + lane;
        const bool act = v < V;
        uint32_t key = 0xffffffffu;
        if (act) {
            bool bad;
            key = gt_id_of(gt[v], bad);
            any_bad |= bad;
        }
        if constexpr (MERGE) {
            int len;
            if (run_head(key, lane, len) && act) atomicAdd(&cnt[key], (uint32_t)len);
        } else {
            if (act) atomicAdd(&cnt[key], 1u);
        }
    }
    if (any_bad) atomicOr(&err[blockIdx.y], 1u);
}

// exclusive scan over the block's threads (N = blockDim.x), sh [N]
template <int N>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* sh, uint32_t& total) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int o = 1; o < N; o <<= 1) {
        const uint32_t y = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    total = sh[N - 1];
    const uint32_t r = sh[t] - x;
    __syncthreads();
    return r;
}

// one block of 1024 threads per scene, 41 ids per thread.  The count table becomes the index table in place (a thread reads only the ids it
// rewrites); list [gt_cap][2] = (id, count) in ascending id order, entry 0 = id 0 (present or not); n_gt = distinct non-zero ids + 1.
__global__ __launch_bounds__(1024) void k_ap_gt_index(uint32_t* __restrict__ cnt_all, int32_t* __restrict__ list_all, int gt_cap,
                                                       int32_t* __restrict__ n_gt) {
    __shared__ uint32_t sh[1024];
    uint32_t* cnt = cnt_all + (size_t)blockIdx.x * kApIdsPad;
    int32_t* list = list_all + (size_t)blockIdx.x * gt_cap * 2;
    const int base = threadIdx.x * 41;
    uint32_t n = 0;
    for (int i = 0; i < 41; ++i) {
        const int id = base + i;
        n += (id >= 1 && id < kApIds && cnt[id] != 0u) ? 1u : 0u;
    }
    uint32_t total;
    uint32_t k = 1u + block_excl_scan<1024>(n, sh, total);
    for (int i = 0; i < 41; ++i) {
        const int id = base + i;
        if (id >= kApIds) break;
        const uint32_t c = cnt[id];
        if (id == 0) {
            list[0] = 0; list[1] = (int32_t)c;
            cnt[0] = 0u;
        } else if (c) {
            if ((int)k < gt_cap) { list[2 * k] = id; list[2 * k + 1] = (int32_t)c; }
            cnt[id] = k++;
        }
    }
    if (threadIdx.x == 0) n_gt[blockIdx.x] = (int32_t)(total + 1u);
}

template <int W, bool MERGE>
__global__ __launch_bounds__(kApBlock) void k_ap_contingency(const ApScene* __restrict__ desc, const void* __restrict__ src_all,
                                                              const int32_t* __restrict__ gt_all, const uint32_t* __restrict__ idx_all,
                                                              uint32_t* __restrict__ C_all, uint32_t* __restrict__ first_all,
                                                              uint32_t* __restrict__ err) {
    const ApScene d = desc[blockIdx.y];
    const int V = (int)d.V, S = (int)d.S, G = (int)d.G, lane = threadIdx.x & 63;
    const int2* gt = reinterpret_cast<const int2*>(gt_all) + d.gt_off;
    const void* src = (W == 2) ? (const void*)(reinterpret_cast<const uint16_t*>(src_all) + d.sov_off)
                               : (const void*)(reinterpret_cast<const int32_t*>(src_all) + d.sov_off);
    const uint32_t* idx = idx_all + (size_t)blockIdx.y * kApIdsPad;
    uint32_t* Cm = C_all + d.c_off;
    uint32_t* first = first_all + d.first_off;
    bool any_bad = false;
    for (int v0 = blockIdx.x * kApBlock + (threadIdx.x & ~63); v0 < V; v0 += gridDim.x * kApBlock) {
        const int v = v0 + lane;
        const bool act = v < V;
        uint32_t key = 0xffffffffu;
        int slot = 0;
        if (act) {
            bool bad_g, bad_s = false;
            const uint32_t id = gt_id_of(gt[v], bad_g);
            slot = ap_slot<W>(src, v, S, bad_s);
            any_bad |= bad_s;
            uint32_t g = idx[id];
            if (g >= (uint32_t)G) g = 0u;                     // cannot happen after k_ap_gt_index on the same gt; keeps the store in bounds
            key = (uint32_t)slot * (uint32_t)G + g;
        }
        if constexpr (MERGE) {
            int len;
            if (run_head(key, lane, len) && act) {            // a run shares (slot, g); its head holds the lowest vertex
                atomicAdd(&Cm[key], (uint32_t)len);
                atomicMin(&first[slot], (uint32_t)v);
            }
        } else {
            if (act) {
                atomicAdd(&Cm[key], 1u);
                atomicMin(&first[slot], (uint32_t)v);
            }
        }
    }
    if (any_bad) atomicOr(&err[blockIdx.y], 2u);
}

__device__ __forceinline__ uint32_t chunk_cells(const uint32_t* __restrict__ Cm, long long cells, long long c0, uint32_t (&val)[8]) {
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        val[i] = c0 + i < cells ? Cm[c0 + i] : 0u;
        n += val[i] != 0u;
    }
    return n;
}

__global__ __launch_bounds__(kApBlock) void k_ap_chunk_count(const ApScene* __restrict__ desc, const uint32_t* __restrict__ C_all,
                                                              uint32_t* __restrict__ chunk_all) {
    __shared__ uint32_t sh[kApBlock];
    const ApScene d = desc[blockIdx.y];
    if (blockIdx.x >= d.nchunks) return;
    const long long cells = (d.S + 1) * d.G;
    uint32_t val[8], total;
    const uint32_t n = chunk_cells(C_all + d.c_off, cells, (long long)blockIdx.x * kApChunk + threadIdx.x * 8, val);
    (void)block_excl_scan<kApBlock>(n, sh, total);
    if (threadIdx.x == 0) chunk_all[d.chunk_off + blockIdx.x] = total;
}

// one block per scene: the chunk counts become their exclusive prefix; entry [nchunks] = the scene's number of triples
__global__ __launch_bounds__(kApBlock) void k_ap_chunk_scan(const ApScene* __restrict__ desc, uint32_t* __restrict__ chunk_all) {
    __shared__ uint32_t sh[kApBlock];
    const ApScene d = desc[blockIdx.x];
    uint32_t* ch = chunk_all + d.chunk_off;
    uint32_t run = 0;
    for (long long c0 = 0; c0 < d.nchunks; c0 += kApBlock) {
        const long long c = c0 + threadIdx.x;
        const uint32_t x = c < d.nchunks ? ch[c] : 0u;
        uint32_t total;
        const uint32_t off = block_excl_scan<kApBlock>(x, sh, total);
        if (c < d.nchunks) ch[c] = run + off;
        run += total;
    }
    if (threadIdx.x == 0) ch[d.nchunks] = run;
}

__global__ __launch_bounds__(kApBlock) void k_ap_compact(const ApScene* __restrict__ desc, const uint32_t* __restrict__ C_all,
                                                          const uint32_t* __restrict__ chunk_all, int32_t* __restrict__ trip_all) {
    __shared__ uint32_t sh[kApBlock];
    const ApScene d = desc[blockIdx.y];
    if (blockIdx.x >= d.nchunks) return;
    const long long cells = (d.S + 1) * d.G, c0 = (long long)blockIdx.x * kApChunk + threadIdx.x * 8;
    const int G = (int)d.G;
    uint32_t val[8], total;
    const uint32_t n = chunk_cells(C_all + d.c_off, cells, c0, val);
    uint32_t k = chunk_all[d.chunk_off + blockIdx.x] + block_excl_scan<kApBlock>(n, sh, total);
    int32_t* trip = trip_all + d.trip_off * 3;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (val[i]) {                                         // at most V non-zero cells: k stays below the scene's triple capacity
            const long long c = c0 + i;
            trip[3 * (size_t)k] = (int32_t)(c / G);
            trip[3 * (size_t)k + 1] = (int32_t)(c % G);
            trip[3 * (size_t)k + 2] = (int32_t)val[i];
            ++k;
        }
}

struct ApLayout {
    size_t desc, cnt, list, ngt, err, first, cells, chunks, trips, total;
};

// every size from the descriptors and gt_cap alone (the contingency of scene b takes (S_b + 1) * gt_cap cells at most)
bool ap_layout(int B, const long long* h_desc, int gt_cap, ApLayout& L) {
    size_t first = 0, cells = 0, chunks = 0, trips = 0;
    for (int b = 0; b < B; ++b) {
        const long long S = h_desc[6 * b + 1], V = h_desc[6 * b + 3];
        if (S < 0 || V < 0 || S > INT32_MAX - 1 || V > INT32_MAX) return false;
        const long long c = (S + 1) * (long long)gt_cap;
        if (c > 0x7fffffffLL) return false;
        first += (size_t)S + 1;
        cells += (size_t)c;
        chunks += (size_t)sg::cdiv(c, kApChunk) + 1;
        trips += (size_t)std::min<long long>(V, c);
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += sg::align_up(bytes); return o; };
    L.desc = take((size_t)B * sizeof(ApScene));
    L.cnt = take((size_t)B * kApIdsPad * 4);
    L.list = take((size_t)B * gt_cap * 8);
    L.ngt = take((size_t)B * 4);
    L.err = take((size_t)B * 4);
    L.first = take(first * 4);
    L.cells = take(cells * 4);
    L.chunks = take(chunks * 4);
    L.trips = take(trips * 12);
    L.total = off;
    return true;
}

template <int W>
int launch_contingency(bool merge, dim3 grid, hipStream_t st, const ApScene* d_desc, const void* d_src, const int32_t* d_gt, const uint32_t* d_idx,
                       uint32_t* d_C, uint32_t* d_first, uint32_t* d_err) {
    if (merge) k_ap_contingency<W, true><<<grid, kApBlock, 0, st>>>(d_desc, d_src, d_gt, d_idx, d_C, d_first, d_err);
    else k_ap_contingency<W, false><<<grid, kApBlock, 0, st>>>(d_desc, d_src, d_gt, d_idx, d_C, d_first, d_err);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

// mode: 2 / 4 = seg_of_vertex width, 0 = an instance vector.  flags bit 0: no in-wave merge (plain per-vertex atomics, for measurement)
int ap_contingency(const char* who, int B, const long long* h_desc, const void* d_src, int mode, const int32_t* d_gt, int gt_cap, int flags,
                   long long* h_counts, int32_t* h_gt, int32_t* h_first, int32_t* h_triples, long long triples_cap, void* d_ws, size_t ws_bytes,
                   void* stream) {
    ApLayout L;
    SG_REQUIRE(gt_cap >= 1 && gt_cap <= kApIds && ap_layout(B, h_desc, gt_cap, L), "%s: bad descriptors or gt_cap", who);
    if (ws_bytes < L.total) return sg::fail(SG_ENOMEM, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    const bool merge = !(flags & 1);
    hipStream_t st = sg::as_stream(stream);
    char* ws = (char*)d_ws;
    ApScene* d_desc = (ApScene*)(ws + L.desc);
    uint32_t* d_cnt = (uint32_t*)(ws + L.cnt);
    int32_t* d_list = (int32_t*)(ws + L.list);
    int32_t* d_ngt = (int32_t*)(ws + L.ngt);
    uint32_t* d_err = (uint32_t*)(ws + L.err);
    uint32_t* d_first = (uint32_t*)(ws + L.first);
    uint32_t* d_C = (uint32_t*)(ws + L.cells);
    uint32_t* d_chunks = (uint32_t*)(ws + L.chunks);
    int32_t* d_trips = (int32_t*)(ws + L.trips);

    std::vector<ApScene> desc(B);
    long long max_V = 0, n_first = 0;
    for (int b = 0; b < B; ++b) {
        const long long* h = h_desc + 6 * b;
        ApScene& d = desc[b];
        d = ApScene{};
        d.S = h[1]; d.sov_off = h[2]; d.V = h[3]; d.gt_off = h[4];
        SG_REQUIRE(d.sov_off >= 0 && d.gt_off >= 0 && (mode != 0 || d.S >= 0) && (mode == 0 || d.S >= 1), "%s: bad descriptor of scene %d", who, b);
        SG_REQUIRE(mode != 2 || d.S < 65535, "%s: scene %d has S >= 65535 with 16-bit seg_of_vertex", who, b);
        d.first_off = n_first;
        n_first += d.S + 1;
        max_V = std::max(max_V, d.V);
    }
    // ground-truth index
    SG_HIP(hipMemcpyAsync(d_desc, desc.data(), (size_t)B * sizeof(ApScene), hipMemcpyHostToDevice, st));
    SG_HIP(hipMemsetAsync(d_cnt, 0, (size_t)B * kApIdsPad * 4, st));
    SG_HIP(hipMemsetAsync(d_err, 0, (size_t)B * 4, st));
    const int bx = std::max(1, std::min(sg::cdiv(max_V, kApBlock * 4), 1024));
    if (merge) k_ap_gt_count<true><<<dim3(bx, B), kApBlock, 0, st>>>(d_desc, d_gt, d_cnt, d_err);
    else k_ap_gt_count<false><<<dim3(bx, B), kApBlock, 0, st>>>(d_desc, d_gt, d_cnt, d_err);
    k_ap_gt_index<<<B, 1024, 0, st>>>(d_cnt, d_list, gt_cap, d_ngt);
    SG_LAUNCH_CHECK();
    std::vector<int32_t> ngt(B);
    std::vector<uint32_t> err(B);
    SG_HIP(hipMemcpyAsync(ngt.data(), d_ngt, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(err.data(), d_err, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    int over = -1;
    for (int b = 0; b < B; ++b) {
        h_counts[2 * b] = ngt[b];
        h_counts[2 * b + 1] = 0;
        SG_REQUIRE(!(err[b] & 1u), "%s: scene %d: a ground-truth label has sem outside 0..40 or ins >= 1000 (gt_id = sem*1000 + ins)", who, b);
        if (ngt[b] > gt_cap && over < 0) over = b;
    }
    if (over >= 0)
        return sg::fail(SG_ENOMEM, "%s: scene %d has %d ground-truth ids, gt_cap is %d (h_counts holds every scene's number)", who, over, ngt[over], gt_cap);
    // contingency and compaction, sized by the scenes' own G
    long long n_cells = 0, n_chunks = 0, n_trips = 0, n_gt = 0, max_chunks = 0;
    for (int b = 0; b < B; ++b) {
        ApScene& d = desc[b];
        d.G = ngt[b];
        const long long cells = (d.S + 1) * d.G;
        d.c_off = n_cells; n_cells += cells;
        d.nchunks = sg::cdiv(cells, kApChunk);
        d.chunk_off = n_chunks; n_chunks += d.nchunks + 1;
        d.trip_off = n_trips; n_trips += std::min(d.V, cells);
        max_chunks = std::max(max_chunks, d.nchunks);
        SG_HIP(hipMemcpyAsync(h_gt + 2 * n_gt, d_list + (size_t)b * gt_cap * 2, (size_t)d.G * 8, hipMemcpyDeviceToHost, st));
        n_gt += d.G;
    }
    SG_HIP(hipMemcpyAsync(d_desc, desc.data(), (size_t)B * sizeof(ApScene), hipMemcpyHostToDevice, st));
    SG_HIP(hipMemsetAsync(d_C, 0, (size_t)n_cells * 4, st));
    SG_HIP(hipMemsetAsync(d_first, 0xff, (size_t)n_first * 4, st));
    int rc = mode == 2 ? launch_contingency<2>(merge, dim3(bx, B), st, d_desc, d_src, d_gt, d_cnt, d_C, d_first, d_err)
           : mode == 4 ? launch_contingency<4>(merge, dim3(bx, B), st, d_desc, d_src, d_gt, d_cnt, d_C, d_first, d_err)
                       : launch_contingency<0>(merge, dim3(bx, B), st, d_desc, d_src, d_gt, d_cnt, d_C, d_first, d_err);
    if (rc < 0) { (void)hipStreamSynchronize(st); return rc; }
    const int cx = (int)std::max(1LL, max_chunks);
    k_ap_chunk_count<<<dim3(cx, B), kApBlock, 0, st>>>(d_desc, d_C, d_chunks);
    k_ap_chunk_scan<<<B, kApBlock, 0, st>>>(d_desc, d_chunks);
    k_ap_compact<<<dim3(cx, B), kApBlock, 0, st>>>(d_desc, d_C, d_chunks, d_trips);
    SG_LAUNCH_CHECK();
    std::vector<uint32_t> ntrip(B);
    for (int b = 0; b < B; ++b)
        SG_HIP(hipMemcpyAsync(&ntrip[b], d_chunks + desc[b].chunk_off + desc[b].nchunks, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(err.data(), d_err, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(h_first, d_first, (size_t)n_first * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    long long total = 0;
    for (int b = 0; b < B; ++b) {
        SG_REQUIRE(!(err[b] & 2u), "%s: scene %d: an instance value is larger than S", who, b);
        h_counts[2 * b + 1] = ntrip[b];
        total += ntrip[b];
    }
    if (total > triples_cap) return sg::fail(SG_ENOMEM, "%s: %lld triples, room for %lld", who, total, triples_cap);
    long long o = 0;
    for (int b = 0; b < B; ++b) {
        if (ntrip[b])
            SG_HIP(hipMemcpyAsync(h_triples + 3 * o, d_trips + 3 * desc[b].trip_off, (size_t)ntrip[b] * 12, hipMemcpyDeviceToHost, st));
        o += ntrip[b];
    }
    SG_HIP(hipStreamSynchronize(st));
    return SG_OK;
}

}  // namespace

extern "C" {

size_t sg_ap_contingency_ws_bytes(int B, const long long* h_desc, int gt_cap) {
    ApLayout L;
    if (B <= 0 || !h_desc || gt_cap < 1 || gt_cap > kApIds || !ap_layout(B, h_desc, gt_cap, L)) return 0;
    return L.total;
}

int sg_ap_contingency(int B, const long long* h_desc, const void* d_seg_of_vertex, int sov_width, const int32_t* d_gt, int gt_cap, int flags,
                      long long* h_counts, int32_t* h_gt, int32_t* h_first_vertex, int32_t* h_triples, long long triples_cap, void* d_ws,
                      size_t ws_bytes, void* stream) {
    SG_REQUIRE(B >= 1 && B <= 65535 && h_desc && d_seg_of_vertex && d_gt && (sov_width == 2 || sov_width == 4) && h_counts && h_gt &&
               h_first_vertex && h_triples && triples_cap >= 0 && d_ws, "sg_ap_contingency: bad arguments");
    return ap_contingency("sg_ap_contingency", B, h_desc, d_seg_of_vertex, sov_width, d_gt, gt_cap, flags, h_counts, h_gt, h_first_vertex,
                          h_triples, triples_cap, d_ws, ws_bytes, stream);
}

int sg_ap_contingency_vectors(const int32_t* d_ins, int V, int S, const int32_t* d_gt, int gt_cap, int flags, long long* h_counts, int32_t* h_gt,
                              int32_t* h_first_vertex, int32_t* h_triples, long long triples_cap, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_ins && V >= 0 && S >= 0 && d_gt && h_counts && h_gt && h_first_vertex && h_triples && triples_cap >= 0 && d_ws,
               "sg_ap_contingency_vectors: bad arguments");
    const long long desc[6] = {0, S, 0, V, 0, 0};
    return ap_contingency("sg_ap_contingency_vectors", 1, desc, d_ins, 0, d_gt, gt_cap, flags, h_counts, h_gt, h_first_vertex, h_triples,
                          triples_cap, d_ws, ws_bytes, stream);
}

}  // extern "C"
