// Label visualisation (reference seggroup/dataset/scannet/util.py:431-527, visualize_labels / visualize_grouping_process): every vertex of
// the scan's mesh takes one of 41 palette colours chosen by its label, and the coloured mesh is the source PLY with three bytes per vertex
// replaced.  A label vector is a look-up vec[t][v] = tables[t][seg_of_vertex[v]] (kernels_sgl.hip), so a colour is a look-up too:
//   sg_colour_tables_unique / _apply   table form: one palette INDEX (0..40, one byte) per (row, table slot); slot S = a vertex without a segment
//   sg_colour_vector_unique / _apply   vector form: one palette index per vertex of an arbitrary label vector
//   sg_ply_vertex_records_device(_batch)   the per-vertex hot path: finished PLY vertex blocks for every requested row in ONE launch
// 'segment' colours are colors[rank % 40 + 1] with rank = position of the label in np.unique of the values that OCCUR among the vertices
// (util.py:457, 467): a radix sort + adjacent-unique of the occurring values (sort_device.h), rank by binary search.  Integer marks only --
// the same bytes on every run.  The *_unique calls return the number of distinct values to the host BEFORE the colours are formed, because
// the reference's shuffle (random.shuffle(labels_dict), util.py:459) is drawn on the host over a sequence of exactly that length.
#include "sg_common.h"
#include "sort_device.h"
#include "palette_device.h"

namespace {

constexpr int kNumColours = SG_NUM_COLOURS;          // 40 class colours + white at index 0
constexpr int kBlock = 256;
constexpr int kRecBlock = 512;
constexpr size_t kLdsBudget = 128 * 1024;            // bytes of LDS a block of the record kernel may take (160 KiB per CU on gfx950)
constexpr int kMaxRows = SG_COLOUR_MAX_ROWS;

using sgpal::kPalette;                               // palette_device.h: ScanNet's class palette, index 0 white

template <int W>
__device__ __forceinline__ int load_sov(const void* __restrict__ sov, long long i) {
    if constexpr (W == 2) {
        const uint16_t u = reinterpret_cast<const uint16_t*>(sov)[i];
        return u == 0xFFFF ? -1 : (int)u;
    } else {
        return reinterpret_cast<const int32_t*>(sov)[i];
    }
}

// sort key of a label: the signed order on unsigned keys
__device__ __forceinline__ uint32_t key_of(int32_t v) { return (uint32_t)v ^ 0x80000000u; }

// position of `key` among the `n` ascending distinct keys (n if it is beyond all of them)
__device__ __forceinline__ int lower_bound(const uint32_t* __restrict__ a, int n, uint32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int pymod40(long long x) { const int r = (int)(x % kNumColours); return r < 0 ? r + kNumColours : r; }

// ---- presence: which table slots occur among the vertices (slot S: a vertex without a segment), the lowest occurring slot -------------------
template <int W>
__global__ __launch_bounds__(kBlock) void k_vis_presence(const void* __restrict__ sov, int V, int S, uint32_t* __restrict__ present,
                                                         int* __restrict__ first_slot) {
    int lo = S + 1;
    for (int v = blockIdx.x * kBlock + threadIdx.x; v < V; v += gridDim.x * kBlock) {
        const int s = load_sov<W>(sov, v);
        const int slot = (s >= 0 && s < S) ? s : S;
        present[slot] = 1u;                                   // every writer stores the same word: no atomic needed
        lo = min(lo, slot);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
    if ((threadIdx.x & 63) == 0 && lo <= S) atomicMin(first_slot, lo);
}

// the sort keys of one 'segment' row: the row's value at every occurring slot; a slot no vertex maps to repeats the value of the lowest
// occurring slot, so it adds no distinct value (util.py:457: unique over the vertices, not over the table)
__global__ __launch_bounds__(kBlock) void k_vis_table_keys(const int32_t* __restrict__ row, int S, const uint32_t* __restrict__ present,
                                                           const int* __restrict__ first_slot, uint32_t* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > S) return;
    const int f = *first_slot;                                // <= S: the caller returns early when no vertex exists
    const int j = present[i] ? i : f;
    keys[i] = key_of(j < S ? row[j] : -1);
}

// semantic rows: an occurring value outside -1..40 has no colour (the reference raises IndexError, util.py:475)
__global__ __launch_bounds__(kBlock) void k_vis_table_check(const int32_t* __restrict__ row, int S, const uint32_t* __restrict__ present,
                                                            int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= S || !present[i]) return;
    const int v = row[i];
    if (v < -1 || v > kNumColours) *bad = 1;
}

struct TableRows {                         // by value: what the colour kernel needs to know about every row
    int type[kMaxRows];                    // SG_COLOUR_*
    int sem_row[kMaxRows];                 // instance rows: the semantic row whose classes 1 and 2 are white, or -1
    int count[kMaxRows];                   // segment rows: distinct occurring values
    int dist_off[kMaxRows];                // ... where they start in `distinct` (elements)
    int perm_off[kMaxRows];                // ... where the row's shuffled positions start in `perm`, or -1
};

// d_cidx[r][i], i in 0..S: the palette index of a vertex whose seg_of_vertex is i (S: no segment).  row = blockIdx.y
__global__ __launch_bounds__(kBlock) void k_vis_table_colours(const int32_t* __restrict__ tables, int S, TableRows tr,
                                                              const uint32_t* __restrict__ distinct, const int32_t* __restrict__ perm,
                                                              uint8_t* __restrict__ cidx) {
    const int i = blockIdx.x * kBlock + threadIdx.x, r = blockIdx.y;
    if (i > S) return;
    const int v = i < S ? tables[(size_t)r * S + i] : -1;
    const int type = tr.type[r];
    int c = 0;
    if (type == SG_COLOUR_SEGMENT) {
        if (v != -1) {
            int rank = lower_bound(distinct + tr.dist_off[r], tr.count[r], key_of(v));
            rank = min(rank, max(tr.count[r] - 1, 0));        // (a slot no vertex maps to may hold a value that does not occur)
            if (tr.perm_off[r] >= 0) rank = perm[tr.perm_off[r] + rank];
            c = pymod40(rank) + 1;
        }
    } else if (v != 0 && v != -1) {
        if (type == SG_COLOUR_SEMANTIC) {
            c = min(max(v, 0), kNumColours);                  // (values outside 1..40 were refused by sg_colour_tables_unique)
        } else {
            const int sem = (tr.sem_row[r] >= 0 && i < S) ? tables[(size_t)tr.sem_row[r] * S + i] : 0;
            c = (sem == 1 || sem == 2) ? 0 : pymod40((long long)v - 1) + 1;
        }
    }
    cidx[(size_t)r * (S + 1) + i] = (uint8_t)c;
}

// ---- vector form ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_vis_vector_keys(const int32_t* __restrict__ labels, int V, uint32_t* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < V) keys[i] = key_of(labels[i]);
}
__global__ __launch_bounds__(kBlock) void k_vis_vector_check(const int32_t* __restrict__ labels, int V, int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < V && (labels[i] < -1 || labels[i] > kNumColours)) *bad = 1;
}
__global__ void k_vis_first_key(const uint32_t* __restrict__ distinct, int* __restrict__ out) { *out = (int)distinct[0]; }

// second: 'instance' -> the semantic labels (may be NULL); 'grouping' -> the segment labels (util.py:489-520)
__global__ __launch_bounds__(kBlock) void k_vis_vector_colours(const int32_t* __restrict__ labels, int V, int type,
                                                               const int32_t* __restrict__ second, const uint32_t* __restrict__ distinct,
                                                               int count, const int32_t* __restrict__ perm, int mult,
                                                               uint8_t* __restrict__ cidx) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    const int v = labels[i];
    int c = 0;
    if (type == SG_COLOUR_SEGMENT) {
        if (v != -1) {
            int rank = min(lower_bound(distinct, count, key_of(v)), max(count - 1, 0));
            if (perm) rank = perm[rank];
            c = pymod40(rank) + 1;
        }
    } else if (type == SG_COLOUR_GROUPING) {
        // ins_labels_dict = np.unique(ins)[1:] (util.py:503): the rank among the distinct values without the lowest one
        if (v != -1) c = pymod40(max(lower_bound(distinct, count, key_of(v)) - 1, 0)) + 1;
        else c = pymod40((long long)second[i] * mult) + 1;
    } else if (v != 0 && v != -1) {
        if (type == SG_COLOUR_SEMANTIC) c = min(max(v, 0), kNumColours);
        else c = (second && (second[i] == 1 || second[i] == 2)) ? 0 : pymod40((long long)v - 1) + 1;
    }
    cidx[i] = (uint8_t)c;
}

// ascending distinct values of keys[0..n) -> distinct, their number -> *d_count.  a = the keys, b = a second buffer of n
int sort_unique_keys(uint32_t* a, uint32_t* b, int n, uint32_t* distinct, int* hist, int* scratch, int* d_count, hipStream_t st) {
    using L32 = sgsort::Lists<unsigned int, int>;
    L32 L = sgsort::one_list<unsigned int, int>(a, b, nullptr, nullptr, hist, n);
    sgsort::radix_sort<unsigned int, int, false>(L, 1, 0, 32, st);
    sgsort::unique_sorted<unsigned int>(L.kin[0], n, distinct, nullptr, d_count, scratch, st);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

// workspace of the table form.  The part behind `distinct` survives from _unique to _apply.
struct TableWs {
    uint32_t *present, *keys_a, *keys_b, *distinct;
    int32_t* perm;
    int *hist, *scratch, *ints;            // ints: [0] first slot, [1] bad flag, [2 + r] counts
    bool ok;
};
TableWs carve_tables(void* d_ws, size_t ws_bytes, int S) {
    const size_t n = (size_t)S + 1;
    sg::Carver cv(d_ws, ws_bytes);
    TableWs w{};
    w.distinct = cv.take<uint32_t>(n * kMaxRows);
    w.perm = cv.take<int32_t>(n * kMaxRows);
    w.ints = cv.take<int>(2 + kMaxRows);
    w.present = cv.take<uint32_t>(n);
    w.keys_a = cv.take<uint32_t>(n);
    w.keys_b = cv.take<uint32_t>(n);
    w.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    w.scratch = cv.take<int>(sgsort::unique_ints((long long)n));
    w.ok = cv.ok;
    return w;
}

struct VectorWs {
    uint32_t *keys_a, *keys_b, *distinct;
    int32_t* perm;
    int *hist, *scratch, *ints;            // ints: [0] count, [1] bad flag, [2] lowest key
    bool ok;
};
VectorWs carve_vector(void* d_ws, size_t ws_bytes, int V) {
    const size_t n = (size_t)std::max(V, 1);
    sg::Carver cv(d_ws, ws_bytes);
    VectorWs w{};
    w.distinct = cv.take<uint32_t>(n);
    w.perm = cv.take<int32_t>(n);
    w.ints = cv.take<int>(4);
    w.keys_a = cv.take<uint32_t>(n);
    w.keys_b = cv.take<uint32_t>(n);
    w.hist = cv.take<int>(sgsort::hist_ints((long long)n));
    w.scratch = cv.take<int>(sgsort::unique_ints((long long)n));
    w.ok = cv.ok;
    return w;
}

// ---- PLY vertex records ----------------------------------------------------------------------------------------------------------------
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
struct RecRows { int n; int row[kMaxRows]; };
struct RecScene { long long src_off, V, sov_off, S, cidx_off, ld, out_off; };     // offsets: bytes / entries / bytes / - / bytes / bytes / bytes

// ScanNet's record (float x, y, z; uchar r, g, b, a -- any order of the four bytes of the last word): one 16-byte load per vertex, one
// 16-byte store per vertex and row.  The rows' palette indices sit in LDS when they fit (table form), otherwise they are read through L2;
// in vector form (sov == NULL) row r's index of vertex v is cidx[r * ld + v], a coalesced byte read.
template <int W>
__device__ __forceinline__ void records16_body(const uint4* __restrict__ src, int V, const void* __restrict__ sov, int S,
                                               const uint8_t* __restrict__ cidx, long long ld, const RecRows& rows, int sh_r, int sh_g, int sh_b,
                                               uint4* __restrict__ out, bool lds_tab, int bid, int nblk) {
    extern __shared__ __align__(16) uint8_t vis_lds[];
    __shared__ uint32_t pal[kNumColours + 1];
    if (threadIdx.x <= kNumColours) pal[threadIdx.x] = kPalette[threadIdx.x];
    const int slots = S + 1;
    if (lds_tab)
        for (int r = 0; r < rows.n; ++r)
            for (int i = threadIdx.x; i < slots; i += blockDim.x) vis_lds[r * slots + i] = cidx[(size_t)rows.row[r] * ld + i];
    __syncthreads();
    const uint32_t keep = ~((0xffu << sh_r) | (0xffu << sh_g) | (0xffu << sh_b));
    for (int v = bid * blockDim.x + threadIdx.x; v < V; v += nblk * blockDim.x) {
        uint4 rec = src[v];
        int slot = 0;
        if (sov) {
            const int s = load_sov<W>(sov, v);
            slot = (s >= 0 && s < S) ? s : S;
        }
        const uint32_t w = rec.w & keep;
#pragma unroll 2
        for (int r = 0; r < rows.n; ++r) {
            int c;
            if (!sov) c = cidx[(size_t)rows.row[r] * ld + v];
            else if (lds_tab) c = vis_lds[r * slots + slot];
            else c = cidx[(size_t)rows.row[r] * ld + slot];
            const uint32_t p = pal[min(c, kNumColours)];
            rec.w = w | ((p & 0xffu) << sh_r) | (((p >> 8) & 0xffu) << sh_g) | (((p >> 16) & 0xffu) << sh_b);
            // written once and never read again by this kernel: non-temporal stores (measured at 8 scenes x 150k vertices x 14 rows: 62 us
            // per launch against 82 us with plain stores, tools/time_visualize.py)
            const u4v o4 = {rec.x, rec.y, rec.z, rec.w};
            __builtin_nontemporal_store(o4, reinterpret_cast<u4v*>(out + (size_t)r * V + v));
        }
    }
}

template <int W>
__global__ __launch_bounds__(kRecBlock) void k_ply_records16(const uint4* __restrict__ src, int V, const void* __restrict__ sov, int S,
                                                             const uint8_t* __restrict__ cidx, long long ld, RecRows rows, int sh_r, int sh_g,
                                                             int sh_b, uint4* __restrict__ out, int lds_tab) {
    records16_body<W>(src, V, sov, S, cidx, ld, rows, sh_r, sh_g, sh_b, out, lds_tab != 0, blockIdx.x, gridDim.x);
}

// scene = blockIdx.y; LDS is sized for the batch's largest table, a scene whose rows fit uses it
template <int W>
__global__ __launch_bounds__(kRecBlock) void k_ply_records16_b(const RecScene* __restrict__ desc, const uint8_t* __restrict__ src,
                                                               const void* __restrict__ sov, const uint8_t* __restrict__ cidx, RecRows rows,
                                                               int sh_r, int sh_g, int sh_b, uint8_t* __restrict__ out, int lds_tab) {
    const RecScene d = desc[blockIdx.y];
    if ((long long)blockIdx.x * blockDim.x >= d.V) return;     // no vertex of this scene for the block (it leaves whole: no barrier skipped)
    const void* sv = !sov ? nullptr
                          : (W == 2) ? (const void*)(reinterpret_cast<const uint16_t*>(sov) + d.sov_off)
                                     : (const void*)(reinterpret_cast<const int32_t*>(sov) + d.sov_off);
    records16_body<W>(reinterpret_cast<const uint4*>(src + d.src_off), (int)d.V, sv, (int)d.S, cidx + d.cidx_off, d.ld, rows, sh_r, sh_g, sh_b,
                      reinterpret_cast<uint4*>(out + d.out_off), lds_tab != 0, blockIdx.x, gridDim.x);
}

// any other fixed-size record: one thread per source byte, every row's copy written from it
template <int W>
__device__ __forceinline__ void records_generic_body(const uint8_t* __restrict__ src, int V, int stride, int off_r, int off_g, int off_b,
                                                     const void* __restrict__ sov, int S, const uint8_t* __restrict__ cidx, long long ld,
                                                     const RecRows& rows, uint8_t* __restrict__ out, int bid, int nblk) {
    const long long total = (long long)V * stride;
    for (long long i = (long long)bid * blockDim.x + threadIdx.x; i < total; i += (long long)nblk * blockDim.x) {
        const int v = (int)(i / stride), o = (int)(i - (long long)v * stride);
        const uint8_t byte = src[i];
        const int ch = o == off_r ? 0 : o == off_g ? 1 : o == off_b ? 2 : -1;
        long long at = v;
        if (ch >= 0 && sov) {
            const int s = load_sov<W>(sov, v);
            at = (s >= 0 && s < S) ? s : S;
        }
        for (int r = 0; r < rows.n; ++r) {
            uint8_t b = byte;
            if (ch >= 0) b = (uint8_t)(kPalette[min((int)cidx[(size_t)rows.row[r] * ld + at], kNumColours)] >> (8 * ch));
            out[(size_t)r * total + i] = b;
        }
    }
}

template <int W>
__global__ __launch_bounds__(kRecBlock) void k_ply_records_generic(const uint8_t* __restrict__ src, int V, int stride, int off_r, int off_g, int off_b,
                                                                   const void* __restrict__ sov, int S, const uint8_t* __restrict__ cidx, long long ld,
                                                                   RecRows rows, uint8_t* __restrict__ out) {
    records_generic_body<W>(src, V, stride, off_r, off_g, off_b, sov, S, cidx, ld, rows, out, blockIdx.x, gridDim.x);
}

template <int W>
__global__ __launch_bounds__(kRecBlock) void k_ply_records_generic_b(const RecScene* __restrict__ desc, const uint8_t* __restrict__ src, int stride,
                                                                     int off_r, int off_g, int off_b, const void* __restrict__ sov,
                                                                     const uint8_t* __restrict__ cidx, RecRows rows, uint8_t* __restrict__ out) {
    const RecScene d = desc[blockIdx.y];
    const void* sv = !sov ? nullptr
                          : (W == 2) ? (const void*)(reinterpret_cast<const uint16_t*>(sov) + d.sov_off)
                                     : (const void*)(reinterpret_cast<const int32_t*>(sov) + d.sov_off);
    records_generic_body<W>(src + d.src_off, (int)d.V, stride, off_r, off_g, off_b, sv, (int)d.S, cidx + d.cidx_off, d.ld, rows, out + d.out_off,
                            blockIdx.x, gridDim.x);
}

// the 16-byte fast path: the three colour bytes in the record's last word
bool fast16(int stride, int off_r, int off_g, int off_b) {
    return stride == 16 && off_r >= 12 && off_g >= 12 && off_b >= 12;
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return SG_OK;
    SG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
    return SG_OK;
}

int check_record_layout(const char* who, int stride, int off_r, int off_g, int off_b, int nrows, const int* h_rows, RecRows* rows) {
    SG_REQUIRE(stride >= 3 && stride <= 65536 && off_r >= 0 && off_g >= 0 && off_b >= 0 && off_r < stride && off_g < stride && off_b < stride &&
               off_r != off_g && off_r != off_b && off_g != off_b, "%s: bad record layout (stride %d, colour bytes at %d %d %d)", who, stride,
               off_r, off_g, off_b);
    SG_REQUIRE(nrows >= 1 && nrows <= kMaxRows && h_rows, "%s: 1..%d rows per launch", who, kMaxRows);
    rows->n = nrows;
    for (int r = 0; r < kMaxRows; ++r) rows->row[r] = r < nrows ? h_rows[r] : 0;
    for (int r = 0; r < nrows; ++r) SG_REQUIRE(h_rows[r] >= 0, "%s: negative row", who);
    return SG_OK;
}

}  // namespace

extern "C" {

size_t sg_colour_tables_ws_bytes(int S) {
    const size_t n = (size_t)std::max(S, 0) + 1;
    return 2 * sg::align_up(n * kMaxRows * 4) + sg::align_up((2 + kMaxRows) * 4) + 3 * sg::align_up(n * 4) +
           sg::align_up(sgsort::hist_ints((long long)n) * 4) + sg::align_up(sgsort::unique_ints((long long)n) * 4) + 512;
}

int sg_colour_tables_unique(const int32_t* d_tables, int nvec, int S, const void* d_seg_of_vertex, int sov_width, int V, const int* h_types,
                            int* h_counts, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_tables && nvec >= 1 && nvec <= kMaxRows && S >= 1 && S <= SG_MAX_POINTS && V >= 0 && V <= SG_MAX_POINTS &&
               (V == 0 || d_seg_of_vertex) && (sov_width == 2 || sov_width == 4) && h_types && h_counts && d_ws,
               "sg_colour_tables_unique: bad arguments");
    SG_REQUIRE(sov_width == 4 || S < 65535, "sg_colour_tables_unique: S >= 65535 with 16-bit seg_of_vertex");
    for (int r = 0; r < nvec; ++r) {
        SG_REQUIRE(h_types[r] == SG_COLOUR_SEMANTIC || h_types[r] == SG_COLOUR_INSTANCE || h_types[r] == SG_COLOUR_SEGMENT,
                   "sg_colour_tables_unique: row %d has type %d", r, h_types[r]);
        h_counts[r] = 0;
    }
    if (V == 0) return SG_OK;
    TableWs w = carve_tables(d_ws, ws_bytes, S);
    if (!w.ok) return sg::fail(SG_ENOMEM, "sg_colour_tables_unique: workspace too small (%zu < %zu)", ws_bytes, sg_colour_tables_ws_bytes(S));
    hipStream_t st = sg::as_stream(stream);
    const int n = S + 1;
    SG_HIP(hipMemsetAsync(w.present, 0, (size_t)n * 4, st));
    SG_HIP(hipMemsetAsync(w.ints, 0, (2 + kMaxRows) * 4, st));
    SG_HIP(hipMemsetAsync(w.ints, 0x7f, 4, st));              // first slot: above every slot
    const int pb = std::max(1, std::min(sg::cdiv(V, kBlock), 1024));
    if (sov_width == 2) k_vis_presence<2><<<pb, kBlock, 0, st>>>(d_seg_of_vertex, V, S, w.present, w.ints);
    else k_vis_presence<4><<<pb, kBlock, 0, st>>>(d_seg_of_vertex, V, S, w.present, w.ints);
    for (int r = 0; r < nvec; ++r) {
        const int32_t* row = d_tables + (size_t)r * S;
        if (h_types[r] == SG_COLOUR_SEMANTIC) {
            k_vis_table_check<<<sg::cdiv(S, kBlock), kBlock, 0, st>>>(row, S, w.present, w.ints + 1);
        } else if (h_types[r] == SG_COLOUR_SEGMENT) {
            k_vis_table_keys<<<sg::cdiv(n, kBlock), kBlock, 0, st>>>(row, S, w.present, w.ints, w.keys_a);
            const int rc = sort_unique_keys(w.keys_a, w.keys_b, n, w.distinct + (size_t)r * n, w.hist, w.scratch, w.ints + 2 + r, st);
            if (rc < 0) return rc;
        }
    }
    SG_LAUNCH_CHECK();
    int h[2 + kMaxRows];
    SG_HIP(hipMemcpyAsync(h, w.ints, sizeof h, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (h[1]) return sg::fail(SG_EINVAL, "sg_colour_tables_unique: a semantic label outside -1..%d has no colour", kNumColours);
    for (int r = 0; r < nvec; ++r) h_counts[r] = h[2 + r];
    return SG_OK;
}

int sg_colour_tables_apply(const int32_t* d_tables, int nvec, int S, const int* h_types, const int* h_sem_rows, const int* h_counts,
                           const int32_t* h_perm, const long long* h_perm_off, uint8_t* d_cidx, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(d_tables && nvec >= 1 && nvec <= kMaxRows && S >= 1 && S <= SG_MAX_POINTS && h_types && h_counts && d_cidx && d_ws,
               "sg_colour_tables_apply: bad arguments");
    TableWs w = carve_tables(d_ws, ws_bytes, S);
    if (!w.ok) return sg::fail(SG_ENOMEM, "sg_colour_tables_apply: workspace too small (%zu < %zu)", ws_bytes, sg_colour_tables_ws_bytes(S));
    hipStream_t st = sg::as_stream(stream);
    const int n = S + 1;
    TableRows tr{};
    for (int r = 0; r < kMaxRows; ++r) { tr.type[r] = SG_COLOUR_SEMANTIC; tr.sem_row[r] = -1; tr.perm_off[r] = -1; }
    for (int r = 0; r < nvec; ++r) {
        tr.type[r] = h_types[r];
        SG_REQUIRE(h_types[r] == SG_COLOUR_SEMANTIC || h_types[r] == SG_COLOUR_INSTANCE || h_types[r] == SG_COLOUR_SEGMENT,
                   "sg_colour_tables_apply: row %d has type %d", r, h_types[r]);
        tr.sem_row[r] = (h_sem_rows && h_types[r] == SG_COLOUR_INSTANCE) ? h_sem_rows[r] : -1;
        SG_REQUIRE(tr.sem_row[r] >= -1 && tr.sem_row[r] < nvec, "sg_colour_tables_apply: row %d names semantic row %d", r, tr.sem_row[r]);
        tr.count[r] = h_counts[r];
        SG_REQUIRE(tr.count[r] >= 0 && tr.count[r] <= n, "sg_colour_tables_apply: row %d has %d distinct values", r, tr.count[r]);
        tr.dist_off[r] = r * n;
        if (h_types[r] == SG_COLOUR_SEGMENT && h_perm && h_perm_off && h_perm_off[r] >= 0 && tr.count[r] > 0) {
            const int32_t* p = h_perm + h_perm_off[r];
            for (int i = 0; i < tr.count[r]; ++i)
                SG_REQUIRE(p[i] >= 0 && p[i] < tr.count[r], "sg_colour_tables_apply: row %d: shuffled position %d outside [0, %d)", r, p[i], tr.count[r]);
            SG_HIP(hipMemcpyAsync(w.perm + (size_t)r * n, p, (size_t)tr.count[r] * 4, hipMemcpyHostToDevice, st));
            tr.perm_off[r] = r * n;
        }
    }
    k_vis_table_colours<<<dim3(sg::cdiv(n, kBlock), nvec), kBlock, 0, st>>>(d_tables, S, tr, w.distinct, w.perm, d_cidx);
    SG_LAUNCH_CHECK();
    SG_HIP(hipStreamSynchronize(st));                          // the host's permutation buffers are free when this returns
    return SG_OK;
}

size_t sg_colour_vector_ws_bytes(int V) {
    const size_t n = (size_t)std::max(V, 1);
    return 4 * sg::align_up(n * 4) + sg::align_up(16) + sg::align_up(sgsort::hist_ints((long long)n) * 4) +
           sg::align_up(sgsort::unique_ints((long long)n) * 4) + 512;
}

int sg_colour_vector_unique(const int32_t* d_labels, int V, int type, int* h_count, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(V >= 0 && V <= SG_MAX_POINTS && (V == 0 || d_labels) && h_count && d_ws && type >= SG_COLOUR_SEMANTIC && type <= SG_COLOUR_GROUPING,
               "sg_colour_vector_unique: bad arguments");
    *h_count = 0;
    if (V == 0 || type == SG_COLOUR_INSTANCE) return SG_OK;
    VectorWs w = carve_vector(d_ws, ws_bytes, V);
    if (!w.ok) return sg::fail(SG_ENOMEM, "sg_colour_vector_unique: workspace too small (%zu < %zu)", ws_bytes, sg_colour_vector_ws_bytes(V));
    hipStream_t st = sg::as_stream(stream);
    SG_HIP(hipMemsetAsync(w.ints, 0, 16, st));
    if (type == SG_COLOUR_SEMANTIC) {
        k_vis_vector_check<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_labels, V, w.ints + 1);
    } else {
        k_vis_vector_keys<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_labels, V, w.keys_a);
        const int rc = sort_unique_keys(w.keys_a, w.keys_b, V, w.distinct, w.hist, w.scratch, w.ints, st);
        if (rc < 0) return rc;
        k_vis_first_key<<<1, 1, 0, st>>>(w.distinct, w.ints + 2);
    }
    SG_LAUNCH_CHECK();
    int h[4];
    SG_HIP(hipMemcpyAsync(h, w.ints, sizeof h, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (h[1]) return sg::fail(SG_EINVAL, "sg_colour_vector_unique: a semantic label outside -1..%d has no colour", kNumColours);
    // grouping: the lowest distinct instance label is dropped from the rank table; a vertex that carries it and is not -1 has no colour
    // (the reference raises IndexError, util.py:511)
    if (type == SG_COLOUR_GROUPING && (uint32_t)h[2] != (0xffffffffu ^ 0x80000000u))
        return sg::fail(SG_EINVAL, "sg_colour_vector_unique: grouping colours need a vertex with instance label -1");
    *h_count = h[0];
    return SG_OK;
}

int sg_colour_vector_apply(const int32_t* d_labels, int V, int type, const int32_t* d_second, int count, const int32_t* h_perm, int mult,
                           uint8_t* d_cidx, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(V >= 0 && V <= SG_MAX_POINTS && (V == 0 || (d_labels && d_cidx)) && d_ws && type >= SG_COLOUR_SEMANTIC && type <= SG_COLOUR_GROUPING &&
               count >= 0 && count <= std::max(V, 1) && (type != SG_COLOUR_GROUPING || V == 0 || d_second),
               "sg_colour_vector_apply: bad arguments");
    if (V == 0) return SG_OK;
    VectorWs w = carve_vector(d_ws, ws_bytes, V);
    if (!w.ok) return sg::fail(SG_ENOMEM, "sg_colour_vector_apply: workspace too small (%zu < %zu)", ws_bytes, sg_colour_vector_ws_bytes(V));
    hipStream_t st = sg::as_stream(stream);
    const int32_t* d_perm = nullptr;
    if (type == SG_COLOUR_SEGMENT && h_perm && count > 0) {
        for (int i = 0; i < count; ++i)
            SG_REQUIRE(h_perm[i] >= 0 && h_perm[i] < count, "sg_colour_vector_apply: shuffled position %d outside [0, %d)", h_perm[i], count);
        SG_HIP(hipMemcpyAsync(w.perm, h_perm, (size_t)count * 4, hipMemcpyHostToDevice, st));
        d_perm = w.perm;
    }
    k_vis_vector_colours<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(d_labels, V, type, d_second, w.distinct, count, d_perm, mult, d_cidx);
    SG_LAUNCH_CHECK();
    SG_HIP(hipStreamSynchronize(st));
    return SG_OK;
}

int sg_ply_vertex_records_device(const void* d_src, int V, int stride, int off_r, int off_g, int off_b, const void* d_seg_of_vertex, int sov_width,
                                 int S, const uint8_t* d_cidx, long long ld, int nrows, const int* h_rows, void* d_out, void* stream) {
    RecRows rows;
    int rc = check_record_layout("sg_ply_vertex_records_device", stride, off_r, off_g, off_b, nrows, h_rows, &rows);
    if (rc < 0) return rc;
    SG_REQUIRE(V >= 0 && V <= SG_MAX_POINTS && (V == 0 || (d_src && d_cidx && d_out)) && (!d_seg_of_vertex || sov_width == 2 || sov_width == 4) &&
               (d_seg_of_vertex ? (S >= 1 && S <= SG_MAX_POINTS && ld >= (long long)S + 1) : ld >= V),
               "sg_ply_vertex_records_device: bad arguments");
    SG_REQUIRE(!d_seg_of_vertex || sov_width == 4 || S < 65535, "sg_ply_vertex_records_device: S >= 65535 with 16-bit seg_of_vertex");
    if (V == 0) return SG_OK;
    hipStream_t st = sg::as_stream(stream);
    const bool w2 = d_seg_of_vertex && sov_width == 2;
    if (fast16(stride, off_r, off_g, off_b) && ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_out)) & 15) == 0) {
        const size_t tab = d_seg_of_vertex ? (size_t)nrows * ((size_t)S + 1) : 0;
        const bool lds = tab > 0 && tab <= kLdsBudget;
        const size_t dyn = lds ? sg::align_up(tab, 16) : 0;
        if (lds) { rc = w2 ? allow_lds(&k_ply_records16<2>, dyn) : allow_lds(&k_ply_records16<4>, dyn); if (rc < 0) return rc; }
        // one vertex per thread and step; every block stages the rows' indices once, so at most two blocks per CU stride over the scene
        const int blocks = std::max(1, std::min(sg::cdiv(V, kRecBlock), 512));
        const int sr = (off_r - 12) * 8, sg_ = (off_g - 12) * 8, sb = (off_b - 12) * 8;
        if (w2) k_ply_records16<2><<<blocks, kRecBlock, dyn, st>>>((const uint4*)d_src, V, d_seg_of_vertex, S, d_cidx, ld, rows, sr, sg_, sb, (uint4*)d_out, lds);
        else k_ply_records16<4><<<blocks, kRecBlock, dyn, st>>>((const uint4*)d_src, V, d_seg_of_vertex, S, d_cidx, ld, rows, sr, sg_, sb, (uint4*)d_out, lds);
    } else {
        const int blocks = std::max(1, std::min(sg::cdiv((long long)V * stride, kRecBlock), 2048));
        if (w2) k_ply_records_generic<2><<<blocks, kRecBlock, 0, st>>>((const uint8_t*)d_src, V, stride, off_r, off_g, off_b, d_seg_of_vertex, S, d_cidx, ld, rows, (uint8_t*)d_out);
        else k_ply_records_generic<4><<<blocks, kRecBlock, 0, st>>>((const uint8_t*)d_src, V, stride, off_r, off_g, off_b, d_seg_of_vertex, S, d_cidx, ld, rows, (uint8_t*)d_out);
    }
    SG_LAUNCH_CHECK();
    return SG_OK;
}

int sg_ply_vertex_records_device_batch(int B, const long long* d_desc, int max_V, int max_S, const void* d_src, int stride, int off_r, int off_g,
                                       int off_b, const void* d_seg_of_vertex, int sov_width, const uint8_t* d_cidx, int nrows, const int* h_rows,
                                       void* d_out, void* stream) {
    RecRows rows;
    int rc = check_record_layout("sg_ply_vertex_records_device_batch", stride, off_r, off_g, off_b, nrows, h_rows, &rows);
    if (rc < 0) return rc;
    SG_REQUIRE(B >= 0 && B <= 65535 && d_desc && max_V >= 0 && max_V <= SG_MAX_POINTS && max_S >= 1 && max_S <= SG_MAX_POINTS &&
               (!d_seg_of_vertex || sov_width == 2 || sov_width == 4), "sg_ply_vertex_records_device_batch: bad arguments");
    SG_REQUIRE(!d_seg_of_vertex || sov_width == 4 || max_S < 65535, "sg_ply_vertex_records_device_batch: S >= 65535 with 16-bit seg_of_vertex");
    if (B == 0 || max_V == 0) return SG_OK;
    SG_REQUIRE(d_src && d_cidx && d_out, "sg_ply_vertex_records_device_batch: null arrays");
    hipStream_t st = sg::as_stream(stream);
    const bool w2 = d_seg_of_vertex && sov_width == 2;
    const RecScene* desc = reinterpret_cast<const RecScene*>(d_desc);
    // (the fast path also needs every scene's source and output offset to be a multiple of 16: the caller's layout, stated in the header)
    if (fast16(stride, off_r, off_g, off_b) && ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_out)) & 15) == 0) {
        const size_t tab = d_seg_of_vertex ? (size_t)nrows * ((size_t)max_S + 1) : 0;
        const bool lds = tab > 0 && tab <= kLdsBudget;
        const size_t dyn = lds ? sg::align_up(tab, 16) : 0;
        if (lds) { rc = w2 ? allow_lds(&k_ply_records16_b<2>, dyn) : allow_lds(&k_ply_records16_b<4>, dyn); if (rc < 0) return rc; }
        // ~1,024 blocks per launch; with the non-temporal stores 256 / 512 / 1,024 / 2,048 measured the same within the run-to-run band
        const int bx = std::max(1, std::min(sg::cdiv(max_V, kRecBlock), std::max(4, 1024 / B)));
        const int sr = (off_r - 12) * 8, sg_ = (off_g - 12) * 8, sb = (off_b - 12) * 8;
        if (w2) k_ply_records16_b<2><<<dim3(bx, B), kRecBlock, dyn, st>>>(desc, (const uint8_t*)d_src, d_seg_of_vertex, d_cidx, rows, sr, sg_, sb, (uint8_t*)d_out, lds);
        else k_ply_records16_b<4><<<dim3(bx, B), kRecBlock, dyn, st>>>(desc, (const uint8_t*)d_src, d_seg_of_vertex, d_cidx, rows, sr, sg_, sb, (uint8_t*)d_out, lds);
    } else {
        const int bx = std::max(1, std::min(sg::cdiv((long long)max_V * stride, kRecBlock), std::max(4, 2048 / B)));
        if (w2) k_ply_records_generic_b<2><<<dim3(bx, B), kRecBlock, 0, st>>>(desc, (const uint8_t*)d_src, stride, off_r, off_g, off_b, d_seg_of_vertex, d_cidx, rows, (uint8_t*)d_out);
        else k_ply_records_generic_b<4><<<dim3(bx, B), kRecBlock, 0, st>>>(desc, (const uint8_t*)d_src, stride, off_r, off_g, off_b, d_seg_of_vertex, d_cidx, rows, (uint8_t*)d_out);
    }
    SG_LAUNCH_CHECK();
    return SG_OK;
}

}  // extern "C"
