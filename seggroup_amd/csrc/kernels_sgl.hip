// Kernels that work straight from the compact pseudo-label form (`.sgl`, csrc/sgl.cpp): [nvec,S] label tables + one seg_of_vertex
// array per scene, vec[t][v] = tables[t][seg_of_vertex[v]] (-1 where seg_of_vertex[v] < 0; model.py:525-605 via sg_export_labels).
//   sg_expand_labels_device(_batch)  the label vectors on the device (a stage-2 data loader moves ~0.4 MB per scene over PCIe, not 8.4 MB)
//   sg_eval_tables                   evaluate (model.py:608-655) of every layer of many scenes in one pass over each scene's vertices
// Both are gathers: memory-bound, so the tables sit in LDS when they fit and the vector rows leave in 16-byte stores.
#include "sg_common.h"
#include "engine_ctx.h"

namespace {

constexpr int kExpandBlock = 512;
constexpr int kEvalBlock = 512;
constexpr size_t kLdsBudget = 128 * 1024;     // bytes of LDS a block of these kernels may take (160 KiB per CU on gfx950)

template <int W>
__device__ __forceinline__ int load_sov(const void* __restrict__ sov, long long i) {
    if constexpr (W == 2) {
        const uint16_t u = reinterpret_cast<const uint16_t*>(sov)[i];
        return u == 0xFFFF ? -1 : (int)u;
    } else {
        return reinterpret_cast<const int32_t*>(sov)[i];
    }
}

struct ExpandScene { long long tab_off, S, sov_off, V, out_off; };

// one scene's rows: 4 consecutive vertices per thread, every row written with one 16-byte store per 4 (int32) values or two per
// 4 (int64) values where the row position is 16-byte aligned (scalar stores at the edges)
template <int W, typename O>
__device__ __forceinline__ void expand_body(const int32_t* __restrict__ tables, int nvec, int S, const void* __restrict__ sov, int V,
                                            O* __restrict__ out, bool lds_tab, int bid, int nblk) {
    extern __shared__ int32_t tl[];
    if (lds_tab) {
        for (int i = threadIdx.x; i < nvec * S; i += blockDim.x) tl[i] = tables[i];
        __syncthreads();
    }
    const int32_t* T = lds_tab ? tl : tables;
    const int nq = (V + 3) >> 2;
    for (int q = bid * blockDim.x + threadIdx.x; q < nq; q += nblk * blockDim.x) {
        const int v0 = q << 2;
        const int nv = min(4, V - v0);
        int s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = k < nv ? load_sov<W>(sov, v0 + k) : -1;
            s[k] = (x >= 0 && x < S) ? x : -1;
        }
        for (int t = 0; t < nvec; ++t) {
            const int32_t* row = T + (size_t)t * S;
            O val[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = s[k] >= 0 ? (O)row[s[k]] : (O)-1;
            O* o = out + (size_t)t * V + v0;
            if (nv == 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
                if constexpr (sizeof(O) == 4) {
                    *reinterpret_cast<int4*>(o) = make_int4((int)val[0], (int)val[1], (int)val[2], (int)val[3]);
                } else {
                    reinterpret_cast<longlong2*>(o)[0] = make_longlong2((long long)val[0], (long long)val[1]);
                    reinterpret_cast<longlong2*>(o)[1] = make_longlong2((long long)val[2], (long long)val[3]);
                }
            } else {
                for (int k = 0; k < nv; ++k) o[k] = val[k];
            }
        }
    }
}

template <int W, typename O>
__global__ __launch_bounds__(kExpandBlock) void k_expand(const int32_t* __restrict__ tables, int nvec, int S, const void* __restrict__ sov,
                                                         int V, O* __restrict__ out, int lds_tab) {
    expand_body<W, O>(tables, nvec, S, sov, V, out, lds_tab != 0, blockIdx.x, gridDim.x);
}

// scene = blockIdx.y; LDS is sized for the batch's largest table, a scene whose table fits uses it
template <int W, typename O>
__global__ __launch_bounds__(kExpandBlock) void k_expand_b(const ExpandScene* __restrict__ desc, const int32_t* __restrict__ tables, int nvec,
                                                           const void* __restrict__ sov, O* __restrict__ out, int lds_tab) {
    const ExpandScene d = desc[blockIdx.y];
    if ((long long)blockIdx.x * blockDim.x >= (d.V + 3) / 4) return;      // no quad of this scene for the block (it leaves whole: no barrier skipped)
    const void* sv = (W == 2) ? (const void*)(reinterpret_cast<const uint16_t*>(sov) + d.sov_off)
                              : (const void*)(reinterpret_cast<const int32_t*>(sov) + d.sov_off);
    expand_body<W, O>(tables + d.tab_off, nvec, (int)d.S, sv, (int)d.V, out + d.out_off, lds_tab != 0, blockIdx.x, gridDim.x);
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return SG_OK;
    SG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
    return SG_OK;
}

template <int W, typename O>
int launch_expand(const int32_t* d_tables, int nvec, int S, const void* d_sov, int V, void* d_out, hipStream_t st) {
    const size_t tab_bytes = (size_t)nvec * S * 4;
    const bool lds = tab_bytes <= kLdsBudget;
    const size_t dyn = lds ? tab_bytes : 0;
    if (lds) { const int rc = allow_lds(&k_expand<W, O>, dyn); if (rc < 0) return rc; }
    // the grid from V: one quad of vertices per thread, at most 1,024 blocks (4 per CU) striding over the rest -- with the table in LDS every
    // block pays for staging it, so small scenes get few blocks
    const int blocks = std::max(1, std::min(sg::cdiv(sg::cdiv(V, 4), kExpandBlock), 1024));
    k_expand<W, O><<<blocks, kExpandBlock, dyn, st>>>(d_tables, nvec, S, d_sov, V, (O*)d_out, lds ? 1 : 0);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

template <int W, typename O>
int launch_expand_b(int B, const void* d_desc, int max_V, int max_S, const int32_t* d_tables, int nvec, const void* d_sov, void* d_out,
                    hipStream_t st) {
    const size_t tab_bytes = (size_t)nvec * max_S * 4;
    const bool lds = tab_bytes <= kLdsBudget;
    const size_t dyn = lds ? tab_bytes : 0;
    if (lds) { const int rc = allow_lds(&k_expand_b<W, O>, dyn); if (rc < 0) return rc; }
    const int bx = std::max(1, std::min(sg::cdiv(sg::cdiv(max_V, 4), kExpandBlock), std::max(4, 2048 / std::max(B, 1))));
    k_expand_b<W, O><<<dim3(bx, B), kExpandBlock, dyn, st>>>((const ExpandScene*)d_desc, d_tables, nvec, d_sov, (O*)d_out, lds ? 1 : 0);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

// ------------------------------------------------------------------------------------------------
// evaluate, every requested layer in one pass.  Counters of (scene, layer) = the k_eval_counts layout (kernels_graph.hip):
// [0..127] the class histograms and scalars, then ins pred / true / both / first-vertex [max_ins each], then first-sem [max_ins].
// ------------------------------------------------------------------------------------------------
struct EvalScene { long long tab_off, S, sov_off, V, gt_off, cnt_off, max_ins, pad; };
struct LayerRows { int n; int ins[5]; int sem[5]; };

__device__ inline bool sem_valid(int c) {   // SEM_VALID_CLASS_IDS (model.py:27)
    const unsigned long long m = (1ull << 1) | (1ull << 2) | (1ull << 3) | (1ull << 4) | (1ull << 5) | (1ull << 6) | (1ull << 7) |
                                 (1ull << 8) | (1ull << 9) | (1ull << 10) | (1ull << 11) | (1ull << 12) | (1ull << 14) |
                                 (1ull << 16) | (1ull << 24) | (1ull << 28) | (1ull << 33) | (1ull << 34) | (1ull << 36) | (1ull << 39);
    return c >= 0 && c < 64 && ((m >> c) & 1ull);
}
__device__ inline bool ins_valid(int c) { return sem_valid(c) && c != 1 && c != 2; }   // INS_VALID_CLASS_IDS (model.py:28)

__device__ __forceinline__ size_t layer_words(long long max_ins) { return 128 + 5 * (size_t)max_ins; }

__global__ void k_eval_tables_clear(const EvalScene* __restrict__ desc, uint32_t* __restrict__ cnt_all) {
    const EvalScene d = desc[blockIdx.y];
    uint32_t* cnt = cnt_all + d.cnt_off + (size_t)blockIdx.z * layer_words(d.max_ins);
    const long long n0 = 128 + 3 * d.max_ins, n1 = n0 + d.max_ins;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n1; i += (long long)gridDim.x * blockDim.x)
        cnt[i] = i < n0 ? 0u : 0xffffffffu;
}

// LDS: [L][128] histograms | ins arrays [L][4][max_ins] when they fit ins_cap words | the layers' (ins, sem) table rows [2L][S] when they
// fit tab_cap words.  One pass over the scene's vertices: gt and seg_of_vertex are read once, every layer counts through its two rows.
template <int W>
__global__ __launch_bounds__(kEvalBlock) void k_eval_tables(const EvalScene* __restrict__ desc, const int32_t* __restrict__ tables,
                                                            const void* __restrict__ sov_all, const int32_t* __restrict__ gt_all,
                                                            uint32_t* __restrict__ cnt_all, LayerRows lr, int ins_cap, int tab_cap) {
    const EvalScene d = desc[blockIdx.y];
    const int L = lr.n, S = (int)d.S, V = (int)d.V, max_ins = (int)d.max_ins;
    extern __shared__ uint32_t lds[];
    uint32_t* h = lds;                                       // [L][128]
    uint32_t* li = lds + 128 * L;                            // [L][4][max_ins]
    int32_t* lt = reinterpret_cast<int32_t*>(li + ins_cap);  // [2L][S]
    const bool lds_ins = (long long)4 * L * max_ins <= ins_cap;
    const bool lds_tab = (long long)2 * L * S <= tab_cap;
    const int32_t* tab = tables + d.tab_off;
    for (int i = threadIdx.x; i < 128 * L; i += blockDim.x) h[i] = 0;
    if (lds_ins)
        for (int i = threadIdx.x; i < 4 * L * max_ins; i += blockDim.x) li[i] = (i % (4 * max_ins)) < 3 * max_ins ? 0u : 0xffffffffu;
    if (lds_tab)
        for (int i = threadIdx.x; i < 2 * L * S; i += blockDim.x) {
            const int r = i / S, c = i - r * S, l = r >> 1;
            lt[i] = tab[(size_t)((r & 1) ? lr.sem[l] : lr.ins[l]) * S + c];
        }
    __syncthreads();
    const int2* gt = reinterpret_cast<const int2*>(gt_all) + d.gt_off;
    const void* sov = (W == 2) ? (const void*)(reinterpret_cast<const uint16_t*>(sov_all) + d.sov_off)
                               : (const void*)(reinterpret_cast<const int32_t*>(sov_all) + d.sov_off);
    uint32_t sc[5][7];
#pragma unroll
    for (int l = 0; l < 5; ++l)
#pragma unroll
        for (int k = 0; k < 7; ++k) sc[l][k] = 0;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
        const int2 g = gt[v];
        const int st = g.x, it = g.y;
        if (st == 0) continue;                               // valid_idxs (model.py:615)
        int s = load_sov<W>(sov, v);
        if (s < 0 || s >= S) s = -1;
#pragma unroll
        for (int l = 0; l < 5; ++l) {
            if (l >= L) break;
            int ip = -1, sp = -1;
            if (s >= 0) {
                if (lds_tab) { ip = lt[(2 * l) * S + s]; sp = lt[(2 * l + 1) * S + s]; }
                else { ip = tab[(size_t)lr.ins[l] * S + s]; sp = tab[(size_t)lr.sem[l] * S + s]; }
            }
            uint32_t* hl = h + 128 * l;
            sc[l][0] += 1;
            if (sp >= 1 && sp <= 40) atomicAdd(&hl[sp - 1], 1u);
            if (st >= 1 && st <= 40) atomicAdd(&hl[40 + st - 1], 1u);
            if (sp == st) {
                sc[l][1] += 1;
                if (sp >= 1 && sp <= 40) atomicAdd(&hl[80 + sp - 1], 1u);
            }
            sc[l][2] += (ip == it);
            if (sem_valid(st)) { sc[l][3] += 1; sc[l][4] += (sp == st); }
            if (ins_valid(it)) { sc[l][5] += 1; sc[l][6] += (ip == it); }
            uint32_t* base = lds_ins ? li + (size_t)4 * max_ins * l : cnt_all + d.cnt_off + layer_words(max_ins) * l + 128;
            if (ip >= 0 && ip < max_ins) {
                atomicAdd(&base[ip], 1u);
                atomicMin(&base[3 * max_ins + ip], (uint32_t)v);
                if (it == ip) atomicAdd(&base[2 * max_ins + ip], 1u);
            }
            if (it >= 0 && it < max_ins) atomicAdd(&base[max_ins + it], 1u);
        }
    }
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        if (l >= L) break;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            uint32_t x = sc[l][k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            if ((threadIdx.x & 63) == 0 && x) atomicAdd(&h[128 * l + 120 + k], x);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 128 * L; i += blockDim.x) {
        const int l = i >> 7, k = i & 127;
        if (h[i]) atomicAdd(&cnt_all[d.cnt_off + layer_words(max_ins) * l + k], h[i]);
    }
    if (lds_ins)
        for (int i = threadIdx.x; i < L * max_ins; i += blockDim.x) {
            const int l = i / max_ins, j = i - l * max_ins;
            const uint32_t* src = li + (size_t)4 * max_ins * l;
            uint32_t* g = cnt_all + d.cnt_off + layer_words(max_ins) * l + 128;
            if (src[j]) atomicAdd(&g[j], src[j]);
            if (src[max_ins + j]) atomicAdd(&g[max_ins + j], src[max_ins + j]);
            if (src[2 * max_ins + j]) atomicAdd(&g[2 * max_ins + j], src[2 * max_ins + j]);
            if (src[3 * max_ins + j] != 0xffffffffu) atomicMin(&g[3 * max_ins + j], src[3 * max_ins + j]);
        }
}

// the semantic prediction at the first valid vertex of every predicted instance (model.py:636), through the tables; layer = blockIdx.z
template <int W>
__global__ void k_eval_tables_first_sem(const EvalScene* __restrict__ desc, const int32_t* __restrict__ tables, const void* __restrict__ sov_all,
                                        uint32_t* __restrict__ cnt_all, LayerRows lr) {
    const EvalScene d = desc[blockIdx.y];
    const int l = blockIdx.z, max_ins = (int)d.max_ins;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= max_ins) return;
    uint32_t* cnt = cnt_all + d.cnt_off + layer_words(max_ins) * l;
    const uint32_t* ins_p = cnt + 128;
    const uint32_t* first = ins_p + 3 * (size_t)max_ins;
    uint32_t* fsem = cnt + 128 + 4 * (size_t)max_ins;
    if (!ins_p[i]) { fsem[i] = 0xffffffffu; return; }
    const void* sov = (W == 2) ? (const void*)(reinterpret_cast<const uint16_t*>(sov_all) + d.sov_off)
                               : (const void*)(reinterpret_cast<const int32_t*>(sov_all) + d.sov_off);
    const int s = load_sov<W>(sov, first[i]);               // a counted instance has a vertex with a segment
    fsem[i] = (uint32_t)tables[d.tab_off + (size_t)lr.sem[l] * d.S + s];
}

template <int W>
int launch_eval(int B, const EvalScene* d_desc, const int32_t* d_tables, const void* d_sov, const int32_t* d_gt, uint32_t* d_cnt,
                const LayerRows& lr, long long max_V, long long max_S, long long max_ins, hipStream_t st) {
    const int L = lr.n;
    // LDS: the histograms always; then the ins arrays of the batch's largest scene if they fit, then its table rows
    const size_t budget = kLdsBudget / 4 - (size_t)128 * L;
    const size_t need_ins = (size_t)4 * L * max_ins, need_tab = (size_t)2 * L * max_S;
    const size_t ins_cap = need_ins <= budget ? need_ins : 0;
    const size_t tab_cap = need_tab <= budget - ins_cap ? need_tab : 0;
    const size_t dyn = ((size_t)128 * L + ins_cap + tab_cap) * 4;
    int rc = allow_lds(&k_eval_tables<W>, dyn);
    if (rc < 0) return rc;
    k_eval_tables_clear<<<dim3(std::max(1, std::min(sg::cdiv(128 + 4 * max_ins, 256), 64)), B, L), 256, 0, st>>>(d_desc, d_cnt);
    // the grid from the batch's largest V: ~8 vertices per thread and at most 16 blocks per scene (each block flushes its LDS counters once)
    const int bx = std::max(1, std::min(sg::cdiv(max_V, (long long)kEvalBlock * 8), std::max(1, std::min(16, 2048 / std::max(B, 1)))));
    k_eval_tables<W><<<dim3(bx, B), kEvalBlock, dyn, st>>>(d_desc, d_tables, d_sov, d_gt, d_cnt, lr, (int)ins_cap, (int)tab_cap);
    k_eval_tables_first_sem<W><<<dim3(sg::cdiv(std::max(max_ins, 1LL), 256), B, L), 256, 0, st>>>(d_desc, d_tables, d_sov, d_cnt, lr);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_expand_labels_device(const int32_t* d_tables, int nvec, int S, const void* d_seg_of_vertex, int sov_width, int V, void* d_out,
                            int out_elem_bytes, void* stream) {
    SG_REQUIRE(d_tables && nvec >= 1 && S >= 1 && V >= 0 && (V == 0 || (d_seg_of_vertex && d_out)) && (sov_width == 2 || sov_width == 4) &&
               (out_elem_bytes == 4 || out_elem_bytes == 8), "sg_expand_labels_device: bad arguments");
    if (V == 0) return SG_OK;
    hipStream_t st = sg::as_stream(stream);
    if (sov_width == 2) return out_elem_bytes == 4 ? launch_expand<2, int32_t>(d_tables, nvec, S, d_seg_of_vertex, V, d_out, st)
                                                   : launch_expand<2, int64_t>(d_tables, nvec, S, d_seg_of_vertex, V, d_out, st);
    return out_elem_bytes == 4 ? launch_expand<4, int32_t>(d_tables, nvec, S, d_seg_of_vertex, V, d_out, st)
                               : launch_expand<4, int64_t>(d_tables, nvec, S, d_seg_of_vertex, V, d_out, st);
}

int sg_expand_labels_device_batch(int B, const long long* d_desc, int max_V, int max_S, const int32_t* d_tables, int nvec,
                                  const void* d_seg_of_vertex, int sov_width, void* d_out, int out_elem_bytes, void* stream) {
    SG_REQUIRE(B >= 0 && B <= 65535 && d_desc && max_V >= 0 && max_S >= 1 && d_tables && nvec >= 1 && (sov_width == 2 || sov_width == 4) &&
               (out_elem_bytes == 4 || out_elem_bytes == 8), "sg_expand_labels_device_batch: bad arguments");
    if (B == 0 || max_V == 0) return SG_OK;
    SG_REQUIRE(d_seg_of_vertex && d_out, "sg_expand_labels_device_batch: null arrays");
    hipStream_t st = sg::as_stream(stream);
    if (sov_width == 2) return out_elem_bytes == 4 ? launch_expand_b<2, int32_t>(B, d_desc, max_V, max_S, d_tables, nvec, d_seg_of_vertex, d_out, st)
                                                   : launch_expand_b<2, int64_t>(B, d_desc, max_V, max_S, d_tables, nvec, d_seg_of_vertex, d_out, st);
    return out_elem_bytes == 4 ? launch_expand_b<4, int32_t>(B, d_desc, max_V, max_S, d_tables, nvec, d_seg_of_vertex, d_out, st)
                               : launch_expand_b<4, int64_t>(B, d_desc, max_V, max_S, d_tables, nvec, d_seg_of_vertex, d_out, st);
}

size_t sg_eval_tables_ws_bytes(int B, int nlayers, const long long* h_desc) {
    if (B <= 0 || nlayers < 1 || nlayers > 5 || !h_desc) return 0;
    size_t words = 0;
    for (int b = 0; b < B; ++b) words += (size_t)nlayers * (128 + 5 * (size_t)std::max(h_desc[6 * b + 5], 1LL));
    return sg::align_up((size_t)B * sizeof(EvalScene)) + sg::align_up(words * 4);
}

int sg_eval_tables(int B, const long long* h_desc, const int32_t* d_tables, int nvec, const void* d_seg_of_vertex, int sov_width,
                   const int32_t* d_gt, int nlayers, const int* h_layer_rows, float* h_iou_sem, float* h_iou_ins, float* h_acc,
                   void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(B >= 1 && B <= 65535 && h_desc && d_tables && nvec >= 1 && nvec <= SG_NUM_LABEL_VECTORS && d_seg_of_vertex && d_gt &&
               (sov_width == 2 || sov_width == 4) && nlayers >= 1 && nlayers <= 5 && h_layer_rows && h_iou_sem && h_iou_ins && h_acc && d_ws,
               "sg_eval_tables: bad arguments");
    LayerRows lr;
    lr.n = nlayers;
    for (int l = 0; l < 5; ++l) { lr.ins[l] = 0; lr.sem[l] = 0; }
    for (int l = 0; l < nlayers; ++l) {
        lr.ins[l] = h_layer_rows[2 * l];
        lr.sem[l] = h_layer_rows[2 * l + 1];
        SG_REQUIRE(lr.ins[l] >= 0 && lr.ins[l] < nvec && lr.sem[l] >= 0 && lr.sem[l] < nvec, "sg_eval_tables: layer %d names rows outside [0, %d)", l, nvec);
    }
    std::vector<EvalScene> desc(B);
    long long words = 0, max_V = 0, max_S = 1, max_ins = 1;
    for (int b = 0; b < B; ++b) {
        const long long* h = h_desc + 6 * b;
        EvalScene& d = desc[b];
        d.tab_off = h[0]; d.S = h[1]; d.sov_off = h[2]; d.V = h[3]; d.gt_off = h[4]; d.max_ins = std::max(h[5], 1LL); d.pad = 0;
        SG_REQUIRE(d.tab_off >= 0 && d.S >= 1 && d.S <= INT32_MAX && d.sov_off >= 0 && d.V >= 0 && d.V <= INT32_MAX && d.gt_off >= 0 &&
                   d.max_ins <= (1LL << 28), "sg_eval_tables: bad descriptor of scene %d", b);
        SG_REQUIRE(sov_width == 4 || d.S < 65535, "sg_eval_tables: scene %d has S >= 65535 with 16-bit seg_of_vertex", b);
        d.cnt_off = words;
        words += (long long)nlayers * (128 + 5 * d.max_ins);
        max_V = std::max(max_V, d.V); max_S = std::max(max_S, d.S); max_ins = std::max(max_ins, d.max_ins);
    }
    if (ws_bytes < sg_eval_tables_ws_bytes(B, nlayers, h_desc)) return sg::fail(SG_ENOMEM, "sg_eval_tables: workspace too small");
    EvalScene* d_desc = (EvalScene*)d_ws;
    uint32_t* d_cnt = (uint32_t*)((char*)d_ws + sg::align_up((size_t)B * sizeof(EvalScene)));
    hipStream_t st = sg::as_stream(stream);
    SG_HIP(hipMemcpyAsync(d_desc, desc.data(), (size_t)B * sizeof(EvalScene), hipMemcpyHostToDevice, st));
    const int rc = sov_width == 2 ? launch_eval<2>(B, d_desc, d_tables, d_seg_of_vertex, d_gt, d_cnt, lr, max_V, max_S, max_ins, st)
                                  : launch_eval<4>(B, d_desc, d_tables, d_seg_of_vertex, d_gt, d_cnt, lr, max_V, max_S, max_ins, st);
    if (rc < 0) { (void)hipStreamSynchronize(st); return rc; }
    std::vector<uint32_t> h((size_t)words);
    SG_HIP(hipMemcpyAsync(h.data(), d_cnt, (size_t)words * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    // ratios on the host exactly as sg_evaluate forms them: per (scene, layer) float32 values identical to the per-vector evaluation
    for (int b = 0; b < B; ++b)
        for (int l = 0; l < nlayers; ++l) {
            const size_t o = (size_t)b * nlayers + l;
            sg::eval_finish(h.data() + desc[b].cnt_off + (size_t)l * (128 + 5 * desc[b].max_ins), (int)desc[b].max_ins, h_iou_sem + o * 80,
                            h_iou_ins + o * 80, h_acc + o * 4);
        }
    return SG_OK;
}

}  // extern "C"
