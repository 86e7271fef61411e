// Oriented boxes of labelled points, device side: a label index -- a segmented view of a cloud -- and the per-label
// reductions a box needs.  Every result is an exact function of the input: the index is integers, minima and maxima are order-free, and
// the ten sums go on fixed trees.
//
//   k_li_keys          key[i] = label[i], or 2^31 for an ignored point (label < 0), value[i] = i.  sort_device.h's stable radix sort over
//                      32 key bits (three 11-bit passes) leaves the labelled points in front, by label and in ascending index within a
//                      label, and the ignored ones behind them; unique_sorted gives the distinct keys and where each run starts.
//   k_li_finish        one thread: the run of ignored points, if there is one, is taken off the end; start[L] = M.
//   k_lb_counts        per label ceil(count / 1024) chunks, and as many partial rows when that is more than one.  Two scan64_device.h sums
//                      make the chunk table; k_lb_chunk_labels bisects the offsets, one thread a chunk, so that a workgroup finds its
//                      (label, chunk) with one load.
//   k_lb_moments       one workgroup per (label, chunk): count | sum q | sum q q^T with q = p - p_first on the first tree of
//                      moments_device.h (thread t adds entries t, t + 256, .. in order, then sgmom::block_row), the float minima and
//                      maxima beside them.  A label of one chunk is written where it belongs, a longer one leaves a
//                      partial row per chunk and k_lb_moments_fold adds them in ascending order.
//   k_lb_yaw           one workgroup per (label, chunk).  The chunk's x, y go into LDS once, as doubles.  A lane owns an angle: c, s and
//                      four extremes in registers; every lane reads the same LDS address (a broadcast, conflict-free -- 8s.4).  The four
//                      waves split the chunk and their extremes meet through LDS; angles beyond 64 are further turns of the same loop, so
//                      that the best angle of a one-chunk label is found where its extents are.  Longer labels leave [chunk][A][4] and
//                      k_lb_yaw_fold takes the extremes over the chunks -- any order gives the same bits.
//   k_lb_frame         the same walk with the label's own 3 x 3 frame: a thread owns points, six extremes meet through LDS.
// No floating-point atomics.  The only integer atomic is the OR into the flag word.
#include <cmath>

#include "moments_device.h"
#include "overseg_device.h"
#include "scan64_device.h"
#include "sg_common.h"
#include "sort_device.h"
#include "wave_ops.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxPoints = 1 << 24;
constexpr int kMaxAngles = 1024;
constexpr int kMaxAll = 1 << 24;              // L * A of d_all
constexpr int kChunk = sgmom::kItems;         // entries of a label's list per workgroup: the moment kernels' 256 threads x 4
constexpr int kPer = kChunk / kBlock;
static_assert(kBlock == sgmom::kBlock && kPer == sgmom::kPer, "k_lb_moments runs on the launch shape of moments_device.h");
constexpr int kMom = 10;
constexpr unsigned kIgnoredKey = 0x80000000u;
constexpr int kBadPoint = 1, kBadIndex = 2;   // the flag word's bits

struct Landing { int flag, L, ignored, pad; };
struct Chunk { int l, first, rows, chunks, cil; long long prow; };

__global__ __launch_bounds__(kBlock) void k_li_keys(const int32_t* __restrict__ label, int N, unsigned* __restrict__ key, int32_t* __restrict__ val) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int32_t v = label[i];
    key[i] = v < 0 ? kIgnoredKey : (unsigned)v;
    val[i] = i;
}

// unique_sorted left *count runs, their keys in value[] and their first positions in start[]
__global__ void k_li_finish(const unsigned* __restrict__ value, int32_t* __restrict__ start, const int* __restrict__ count, int N,
                            Landing* __restrict__ land) {
    if (blockIdx.x || threadIdx.x) return;
    int L = *count;
    int ignored = 0;
    if (L > 0 && value[L - 1] == kIgnoredKey) {
        --L;
        ignored = N - start[L];                  // start[L] = M already: where the ignored run begins
    } else {
        start[L] = N;
    }
    land->L = L;
    land->ignored = ignored;
}

__device__ __forceinline__ bool label_span(const int32_t* __restrict__ start, int l, int N, int* first, int* count) {
    *first = start[l];
    *count = start[l + 1] - *first;
    return *first >= 0 && *count >= 1 && *count <= N && *first <= N - *count;
}

__global__ __launch_bounds__(kBlock) void k_lb_counts(const int32_t* __restrict__ start, int L, int N, int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ pcnt, int* __restrict__ flag) {
    const int l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= L) return;
    int first, count;
    int c = 0;
    if (label_span(start, l, N, &first, &count)) c = (count + kChunk - 1) / kChunk;
    else atomicOr(flag, kBadIndex);
    cnt[l] = c;
    pcnt[l] = c > 1 ? c : 0;
}

// thread b: the label of chunk b, the first l with coff[l + 1] > b; -1 past the last chunk.  One thread a chunk, so that the bisection's
// dependent loads hide behind one another; a workgroup of the reductions then finds its (label, chunk) with one load.
__global__ __launch_bounds__(kBlock) void k_lb_chunk_labels(const int64_t* __restrict__ coff, int L, int grid, int32_t* __restrict__ lab_of) {
    const long long b = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (b >= (long long)grid) return;
    if (b >= (long long)coff[L]) { lab_of[b] = -1; return; }
    int lo = 0, hi = L - 1;                                           // coff[hi + 1] > b holds
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((long long)coff[mid + 1] > b) hi = mid; else lo = mid + 1;
    }
    lab_of[b] = lo;
}

// the (label, chunk) of this workgroup.  false: past the last chunk, or a label whose span k_lb_counts refused (it has no chunk, so it
// is never found).
__device__ __forceinline__ bool find_chunk(const int32_t* __restrict__ lab_of, const int64_t* __restrict__ coff, const int64_t* __restrict__ poff,
                                           const int32_t* __restrict__ start, int L, int N, Chunk* c) {
    const long long b = blockIdx.x;
    const int lo = lab_of[b];
    if (lo < 0 || lo >= L) return false;
    int first, count;
    if (!label_span(start, lo, N, &first, &count)) return false;
    c->l = lo;
    c->cil = (int)(b - (long long)coff[lo]);
    c->chunks = (count + kChunk - 1) / kChunk;
    if (c->cil < 0 || c->cil >= c->chunks) return false;
    c->first = first + c->cil * kChunk;
    c->rows = min(kChunk, count - c->cil * kChunk);
    c->prow = (long long)poff[lo] + c->cil;
    return true;
}

// entry `pos` of the list -> its point, or NULL with the flag raised: an index outside the cloud, a coordinate that is not finite
__device__ __forceinline__ const float* point_of(const float* __restrict__ xyz, int xs, int N, const int32_t* __restrict__ order, int pos,
                                                 int* __restrict__ flag) {
    const int i = order[pos];
    if (i < 0 || i >= N) { atomicOr(flag, kBadIndex); return nullptr; }
    const float* p = xyz + (size_t)i * xs;
    if (!(sgos::finite_f32(p[0]) && sgos::finite_f32(p[1]) && sgos::finite_f32(p[2]))) { atomicOr(flag, kBadPoint); return nullptr; }
    return p;
}

// every thread of a workgroup that has a chunk reaches block_row and the wave reductions: an entry past the chunk adds 0
__global__ __launch_bounds__(kBlock) void k_lb_moments(const float* __restrict__ xyz, int xs, int N, const int32_t* __restrict__ order,
                                                       const int32_t* __restrict__ start, int L, const int32_t* __restrict__ lab_of, const int64_t* __restrict__ coff,
                                                       const int64_t* __restrict__ poff, double* __restrict__ out_m, float* __restrict__ out_lo,
                                                       float* __restrict__ out_hi, double* __restrict__ part_m, float* __restrict__ part_e,
                                                       int* __restrict__ flag) {
    __shared__ float s_ext[kWaves][6];
    Chunk ck;
    if (!find_chunk(lab_of, coff, poff, start, L, N, &ck)) return;               // uniform over the workgroup
    double o[3] = {0.0, 0.0, 0.0};
    {
        const int i0 = order[start[ck.l]];
        if (i0 >= 0 && i0 < N)
            for (int r = 0; r < 3; ++r) o[r] = (double)xyz[(size_t)i0 * xs + r];
    }
    double acc[kMom];
#pragma unroll
    for (int m = 0; m < kMom; ++m) acc[m] = 0.0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = j * kBlock + (int)threadIdx.x;
        if (e >= ck.rows) continue;
        const float* p = point_of(xyz, xs, N, order, ck.first + e, flag);
        if (!p) continue;
        const double q[3] = {(double)p[0] - o[0], (double)p[1] - o[1], (double)p[2] - o[2]};
        acc[0] += 1.0;
        int k = 4;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            lo[r] = fminf(lo[r], p[r]);
            hi[r] = fmaxf(hi[r], p[r]);
            acc[1 + r] += q[r];
#pragma unroll
            for (int c = r; c < 3; ++c) acc[k++] += q[r] * q[c];
        }
    }
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = sgw::wave_min(lo[r]), b = sgw::wave_max(hi[r]);
        if (lane == 0) { s_ext[wave][r] = a; s_ext[wave][3 + r] = b; }
    }
    const bool whole = ck.chunks == 1;
    sgmom::block_row(acc, whole ? out_m + (size_t)ck.l * kMom : part_m + (size_t)ck.prow * kMom);   // its barrier covers s_ext too
    if (threadIdx.x >= kWave && threadIdx.x < kWave + 6) {
        const int r = threadIdx.x - kWave;
        float v = s_ext[0][r];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v = r < 3 ? fminf(v, s_ext[w][r]) : fmaxf(v, s_ext[w][r]);
        if (!whole) part_e[(size_t)ck.prow * 6 + r] = v;
        else if (r < 3) out_lo[(size_t)ck.l * 3 + r] = v;
        else out_hi[(size_t)ck.l * 3 + r - 3] = v;
    }
}

// thread (l, slot): slots 0..9 add the label's partial rows in ascending chunk order, 10..15 take the extremes
__global__ __launch_bounds__(kBlock) void k_lb_moments_fold(const int32_t* __restrict__ cnt, const int64_t* __restrict__ poff, int L,
                                                            const double* __restrict__ part_m, const float* __restrict__ part_e,
                                                            double* __restrict__ out_m, float* __restrict__ out_lo, float* __restrict__ out_hi) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int l = (int)(t / 16), slot = (int)(t % 16);
    if (l >= L) return;
    const int chunks = cnt[l];
    if (chunks <= 1) return;
    const size_t row = (size_t)poff[l];
    if (slot < kMom) {
        double s = part_m[row * kMom + slot];
        for (int c = 1; c < chunks; ++c) s += part_m[(row + c) * kMom + slot];
        out_m[(size_t)l * kMom + slot] = s;
    } else {
        const int r = slot - kMom;
        float v = part_e[row * 6 + r];
        for (int c = 1; c < chunks; ++c) v = r < 3 ? fminf(v, part_e[(row + c) * 6 + r]) : fmaxf(v, part_e[(row + c) * 6 + r]);
        if (r < 3) out_lo[(size_t)l * 3 + r] = v;
        else out_hi[(size_t)l * 3 + r - 3] = v;
    }
}

// The best angle of one label from what each lane of ONE whole wave holds: lane k offers (area, a, ext) -- the best of the angles it owned,
// the lowest among equals, a < 0 for none -- and a butterfly over the wave leaves every lane with the smallest area and the lowest a
// among equals; the lane that offered it writes.  Areas are not NaN: the coordinates are finite.
struct Offer { double area; int a; double e[4]; };

__device__ __forceinline__ void take_best(const Offer& mine, int l, int32_t* __restrict__ best, double* __restrict__ ext) {
    double area = mine.a < 0 ? INFINITY : mine.area;
    int a = mine.a < 0 ? 0x7fffffff : mine.a;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double other_area = __shfl_xor(area, o);
        const int other_a = __shfl_xor(a, o);
        if (other_area < area || (other_area == area && other_a < a)) { area = other_area; a = other_a; }
    }
    if (mine.a < 0 || mine.a != a) return;                                // A >= 1: lane 0 always offers
    best[l] = a;
    for (int r = 0; r < 4; ++r) ext[(size_t)l * 4 + r] = mine.e[r];
}

__device__ __forceinline__ void offer(Offer& mine, int a, const double* e) {
    const double area = (e[1] - e[0]) * (e[3] - e[2]);
    if (mine.a < 0 || area < mine.area) {
        mine.area = area;
        mine.a = a;
        for (int r = 0; r < 4; ++r) mine.e[r] = e[r];
    }
}

__global__ __launch_bounds__(kBlock) void k_lb_yaw(const float* __restrict__ xyz, int xs, int N, const int32_t* __restrict__ order,
                                                   const int32_t* __restrict__ start, int L, const int32_t* __restrict__ lab_of, const int64_t* __restrict__ coff,
                                                   const int64_t* __restrict__ poff, const double* __restrict__ cs, int A,
                                                   int32_t* __restrict__ best, double* __restrict__ ext, double* __restrict__ all,
                                                   double* __restrict__ part, int* __restrict__ flag) {
    __shared__ double s_x[kChunk], s_y[kChunk];
    __shared__ double s_e[kWaves][kWave][4];
    Chunk ck;
    if (!find_chunk(lab_of, coff, poff, start, L, N, &ck)) return;               // uniform over the workgroup
    for (int e = threadIdx.x; e < ck.rows; e += kBlock) {
        const float* p = point_of(xyz, xs, N, order, ck.first + e, flag);
        // a refused entry is a NaN, which fmin / fmax pass over: it changes no extreme, and the call fails on the flag anyway
        s_x[e] = p ? (double)p[0] : NAN;
        s_y[e] = p ? (double)p[1] : NAN;
    }
    __syncthreads();
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int per = (ck.rows + kWaves - 1) / kWaves;
    const int r0 = min(wave * per, ck.rows), r1 = min(r0 + per, ck.rows);
    Offer mine;
    mine.a = -1;
    mine.area = 0.0;
    for (int r = 0; r < 4; ++r) mine.e[r] = 0.0;
    for (int a0 = 0; a0 < A; a0 += kWave) {
        const int a = a0 + lane;
        const double c = a < A ? cs[2 * a] : 1.0, s = a < A ? cs[2 * a + 1] : 0.0;
        double e[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
        for (int r = r0; r < r1; ++r) {
            const double x = s_x[r], y = s_y[r];
            const double u = c * x + s * y, v = c * y - s * x;
            e[0] = fmin(e[0], u);                                         // fmin / fmax pass over a NaN (a refused entry)
            e[1] = fmax(e[1], u);
            e[2] = fmin(e[2], v);
            e[3] = fmax(e[3], v);
        }
        __syncthreads();                                                  // the previous turn's s_e has been read
        for (int r = 0; r < 4; ++r) s_e[wave][lane][r] = e[r];
        __syncthreads();
        if (wave == 0 && a < A) {
            for (int w = 1; w < kWaves; ++w) {
                e[0] = fmin(e[0], s_e[w][lane][0]);
                e[1] = fmax(e[1], s_e[w][lane][1]);
                e[2] = fmin(e[2], s_e[w][lane][2]);
                e[3] = fmax(e[3], s_e[w][lane][3]);
            }
            if (ck.chunks == 1) {
                offer(mine, a, e);
                if (all)
                    for (int r = 0; r < 4; ++r) all[((size_t)ck.l * A + a) * 4 + r] = e[r];
            } else {
                for (int r = 0; r < 4; ++r) part[((size_t)ck.prow * A + a) * 4 + r] = e[r];
            }
        }
    }
    if (wave == 0 && ck.chunks == 1) take_best(mine, ck.l, best, ext);
}

// one wave per label of more than one chunk
__global__ __launch_bounds__(kWave) void k_lb_yaw_fold(const int32_t* __restrict__ cnt, const int64_t* __restrict__ poff, int L, int A,
                                                       const double* __restrict__ part, int32_t* __restrict__ best, double* __restrict__ ext,
                                                       double* __restrict__ all) {
    const int l = blockIdx.x, lane = threadIdx.x;
    if (l >= L) return;
    const int chunks = cnt[l];
    if (chunks <= 1) return;
    const size_t row = (size_t)poff[l];
    Offer mine;
    mine.a = -1;
    mine.area = 0.0;
    for (int r = 0; r < 4; ++r) mine.e[r] = 0.0;
    for (int a = lane; a < A; a += kWave) {
        double e[4];
        for (int r = 0; r < 4; ++r) e[r] = part[(row * A + a) * 4 + r];
        for (int c = 1; c < chunks; ++c) {
            const double* p = part + ((row + c) * A + a) * 4;
            e[0] = fmin(e[0], p[0]);
            e[1] = fmax(e[1], p[1]);
            e[2] = fmin(e[2], p[2]);
            e[3] = fmax(e[3], p[3]);
        }
        offer(mine, a, e);
        if (all)
            for (int r = 0; r < 4; ++r) all[((size_t)l * A + a) * 4 + r] = e[r];
    }
    take_best(mine, l, best, ext);
}

__global__ __launch_bounds__(kBlock) void k_lb_frame(const float* __restrict__ xyz, int xs, int N, const int32_t* __restrict__ order,
                                                     const int32_t* __restrict__ start, int L, const int32_t* __restrict__ lab_of, const int64_t* __restrict__ coff,
                                                     const int64_t* __restrict__ poff, const double* __restrict__ frame, double* __restrict__ ext,
                                                     double* __restrict__ part, int* __restrict__ flag) {
    __shared__ double s_e[kBlock][6];
    Chunk ck;
    if (!find_chunk(lab_of, coff, poff, start, L, N, &ck)) return;               // uniform over the workgroup
    double f[9];
    for (int r = 0; r < 9; ++r) f[r] = frame[(size_t)ck.l * 9 + r];
    double e[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int en = j * kBlock + (int)threadIdx.x;
        if (en >= ck.rows) continue;
        const float* p = point_of(xyz, xs, N, order, ck.first + en, flag);
        if (!p) continue;
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double d = (f[3 * k] * x + f[3 * k + 1] * y) + f[3 * k + 2] * z;
            e[2 * k] = fmin(e[2 * k], d);
            e[2 * k + 1] = fmax(e[2 * k + 1], d);
        }
    }
    for (int r = 0; r < 6; ++r) s_e[threadIdx.x][r] = e[r];
    __syncthreads();
    for (int half = kBlock / 2; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int r = 0; r < 6; ++r)
                s_e[threadIdx.x][r] = (r & 1) ? fmax(s_e[threadIdx.x][r], s_e[threadIdx.x + half][r]) : fmin(s_e[threadIdx.x][r], s_e[threadIdx.x + half][r]);
        __syncthreads();
    }
    if (threadIdx.x < 6) {
        if (ck.chunks == 1) ext[(size_t)ck.l * 6 + threadIdx.x] = s_e[0][threadIdx.x];
        else part[(size_t)ck.prow * 6 + threadIdx.x] = s_e[0][threadIdx.x];
    }
}

__global__ __launch_bounds__(kBlock) void k_lb_frame_fold(const int32_t* __restrict__ cnt, const int64_t* __restrict__ poff, int L,
                                                          const double* __restrict__ part, double* __restrict__ ext) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int l = (int)(t / 8), r = (int)(t % 8);
    if (l >= L || r >= 6) return;
    const int chunks = cnt[l];
    if (chunks <= 1) return;
    const size_t row = (size_t)poff[l];
    double v = part[row * 6 + r];
    for (int c = 1; c < chunks; ++c) v = (r & 1) ? fmax(v, part[(row + c) * 6 + r]) : fmin(v, part[(row + c) * 6 + r]);
    ext[(size_t)l * 6 + r] = v;
}

constexpr int kStages = 4;
const char* const kStageNames[kStages] = {"index", "moments", "yaw", "frame"};
thread_local sgos::StageTimes<kStages> t_label;

// partial rows at most: a label of more than one chunk has more than 1,024 points, so fewer than 2 count / 1,024 chunks
size_t part_rows(int N) { return 2 * (size_t)sg::cdiv(std::max(N, 1), kChunk) + 2; }

// workgroups of a reduction: at least the chunks there are, sum ceil(c / 1024) <= L + M / 1024
int chunk_grid(int N, int L) { return L + sg::cdiv(N, kChunk); }

// what the three reductions share of the workspace: the flag word and the chunk table
size_t table_bytes(int N, int L) {
    const size_t l = (size_t)std::max(L, 1);
    return sg::align_up(sizeof(Landing)) + 2 * sg::align_up(l * sizeof(int32_t)) + 2 * sg::align_up((l + 1) * sizeof(int64_t)) +
           sg::align_up((size_t)(sgscan::tiles_of(std::max(L, 1)) + 1) * sizeof(long long)) + sg::align_up((size_t)chunk_grid(N, L) * sizeof(int32_t));
}

struct Table {
    Landing* land;
    int32_t *cnt, *pcnt, *lab_of;
    int64_t *coff, *poff;
    int grid;
};

bool sizes_ok(int N, int L) { return N >= 0 && N <= kMaxPoints && L >= 0 && L <= N; }

// carve and launch the chunk table on `st`
int make_table(const char* who, sg::Carver& cv, const int32_t* d_start, int N, int L, hipStream_t st, Table* t) {
    t->land = cv.take<Landing>(1);
    t->cnt = cv.take<int32_t>((size_t)L);
    t->pcnt = cv.take<int32_t>((size_t)L);
    t->coff = cv.take<int64_t>((size_t)L + 1);
    t->poff = cv.take<int64_t>((size_t)L + 1);
    long long* tsum = cv.take<long long>((size_t)sgscan::tiles_of(L) + 1);
    t->grid = chunk_grid(N, L);
    t->lab_of = cv.take<int32_t>((size_t)t->grid);
    SG_REQUIRE(cv.ok, "%s: workspace too small", who);
    SG_HIP(hipMemsetAsync(t->land, 0, sizeof(Landing), st));
    k_lb_counts<<<sg::cdiv(L, kBlock), kBlock, 0, st>>>(d_start, L, N, t->cnt, t->pcnt, &t->land->flag);
    sgscan::exclusive_scan64(t->cnt, L, tsum, t->coff, st);
    sgscan::exclusive_scan64(t->pcnt, L, tsum, t->poff, st);
    k_lb_chunk_labels<<<sg::cdiv(t->grid, kBlock), kBlock, 0, st>>>(t->coff, L, t->grid, t->lab_of);
    return SG_OK;
}

int land_flag(const char* who, const Table& t, hipStream_t st) {
    Landing land{};
    SG_HIP(hipMemcpyAsync(&land, t.land, sizeof(Landing), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land.flag & kBadIndex)
        return sg::fail(SG_EINVAL, "%s: d_start / d_order are not a label index of this cloud (an offset or a point index out of range)", who);
    if (land.flag & kBadPoint) return sg::fail(SG_EINVAL, "%s: a labelled point has a coordinate that is not finite", who);
    return SG_OK;
}

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(label, t_label, kStageNames)

size_t sg_label_index_ws_bytes(int N) {
    if (N < 0 || N > kMaxPoints) return 0;
    const size_t n = (size_t)std::max(N, 1);
    return sg::align_up(sizeof(Landing)) + 2 * sg::align_up(n * sizeof(unsigned)) + sg::align_up(n * sizeof(int32_t)) +
           sg::align_up(sgsort::hist_ints(N) * sizeof(int)) + sg::align_up(sgsort::unique_ints(N) * sizeof(int)) + sg::align_up(sizeof(int));
}

int sg_label_index(const int32_t* d_label, int N, int32_t* d_order, int32_t* d_value, int32_t* d_start, int* h_L, int* h_ignored, void* d_ws,
                   size_t ws_bytes, void* stream) {
    const char* who = "sg_label_index";
    SG_REQUIRE(N >= 0 && h_L && h_ignored && d_start, "%s: bad arguments (%d points)", who, N);
    if (N > kMaxPoints) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, kMaxPoints);
    *h_L = 0;
    *h_ignored = 0;
    hipStream_t st = sg::as_stream(stream);
    if (N == 0) {
        SG_HIP(hipMemsetAsync(d_start, 0, sizeof(int32_t), st));
        SG_HIP(hipStreamSynchronize(st));
        return SG_OK;
    }
    SG_REQUIRE(d_label && d_order && d_value && d_ws, "%s: bad arguments", who);
    const size_t need = sg_label_index_ws_bytes(N);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    Landing* land = cv.take<Landing>(1);
    unsigned* key0 = cv.take<unsigned>((size_t)N);
    unsigned* key1 = cv.take<unsigned>((size_t)N);
    int32_t* val0 = cv.take<int32_t>((size_t)N);
    int* hist = cv.take<int>(sgsort::hist_ints(N));
    int* uniq = cv.take<int>(sgsort::unique_ints(N));
    int* count = cv.take<int>(1);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    Landing h{};
    {
        sgos::StageClock<1> clock(st, t_label.timing, t_label.us);
        SG_HIP(hipMemsetAsync(land, 0, sizeof(Landing), st));
        k_li_keys<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_label, N, key0, val0);
        // three passes: the result lands in what was (kout, vout) = (key1, d_order)
        auto lists = sgsort::one_list<unsigned, int32_t>(key0, key1, val0, d_order, hist, N);
        const int passes = sgsort::radix_sort<unsigned, int32_t, true>(lists, 1, 0, 32, st);
        if (passes != 3 || lists.kin[0] != key1) return sg::fail(SG_EINTERNAL, "%s: %d radix passes", who, passes);
        sgsort::unique_sorted<unsigned>(key1, N, (unsigned*)d_value, d_start, count, uniq, st);
        k_li_finish<<<1, 1, 0, st>>>((const unsigned*)d_value, d_start, count, N, land);
        SG_HIP(hipMemcpyAsync(&h, land, sizeof(Landing), hipMemcpyDeviceToHost, st));
        clock.tick();
        SG_HIP(hipStreamSynchronize(st));
    }
    SG_LAUNCH_CHECK();
    if (h.L < 0 || h.L > N || h.ignored < 0 || h.ignored > N - h.L)
        return sg::fail(SG_EINTERNAL, "%s: %d labels and %d ignored of %d points", who, h.L, h.ignored, N);
    *h_L = h.L;
    *h_ignored = h.ignored;
    return SG_OK;
}

size_t sg_label_moments_ws_bytes(int N, int L) {
    if (!sizes_ok(N, L)) return 0;
    return table_bytes(N, L) + sg::align_up(part_rows(N) * kMom * sizeof(double)) + sg::align_up(part_rows(N) * 6 * sizeof(float));
}

int sg_label_moments(const float* d_xyz, int stride, int N, const int32_t* d_order, const int32_t* d_start, int L, double* d_m, float* d_lo,
                     float* d_hi, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_label_moments";
    SG_REQUIRE(N >= 0 && L >= 0 && stride >= 3, "%s: bad arguments (%d points in rows of %d floats, %d labels)", who, N, stride, L);
    if (N > kMaxPoints) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, kMaxPoints);
    SG_REQUIRE(L <= N, "%s: %d labels of %d points", who, L, N);
    if (L == 0) return SG_OK;
    SG_REQUIRE(d_xyz && d_order && d_start && d_m && d_lo && d_hi && d_ws, "%s: bad arguments", who);
    const size_t need = sg_label_moments_ws_bytes(N, L);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    hipStream_t st = sg::as_stream(stream);
    sg::Carver cv(d_ws, ws_bytes);
    Table t;
    sgos::StageClock<1> clock(st, t_label.timing, t_label.us + 1);
    if (int rc = make_table(who, cv, d_start, N, L, st, &t)) return rc;
    double* part_m = cv.take<double>(part_rows(N) * kMom);
    float* part_e = cv.take<float>(part_rows(N) * 6);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    k_lb_moments<<<t.grid, kBlock, 0, st>>>(d_xyz, stride, N, d_order, d_start, L, t.lab_of, t.coff, t.poff, d_m, d_lo, d_hi, part_m, part_e, &t.land->flag);
    k_lb_moments_fold<<<sg::cdiv((long long)L * 16, kBlock), kBlock, 0, st>>>(t.cnt, t.poff, L, part_m, part_e, d_m, d_lo, d_hi);
    clock.tick();
    return land_flag(who, t, st);
}

size_t sg_label_yaw_boxes_ws_bytes(int N, int L, int A) {
    if (!sizes_ok(N, L) || A < 1 || A > kMaxAngles) return 0;
    return table_bytes(N, L) + sg::align_up((size_t)A * 2 * sizeof(double)) + sg::align_up(part_rows(N) * (size_t)A * 4 * sizeof(double));
}

int sg_label_yaw_boxes(const float* d_xyz, int stride, int N, const int32_t* d_order, const int32_t* d_start, int L, const double* h_cs, int A,
                       int32_t* d_best, double* d_ext, double* d_all, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_label_yaw_boxes";
    SG_REQUIRE(N >= 0 && L >= 0 && stride >= 3, "%s: bad arguments (%d points in rows of %d floats, %d labels)", who, N, stride, L);
    SG_REQUIRE(A >= 1 && A <= kMaxAngles && h_cs, "%s: 1..%d angles are needed (%d)", who, kMaxAngles, A);
    for (int a = 0; a < 2 * A; ++a) SG_REQUIRE(std::isfinite(h_cs[a]), "%s: entry %d of the angle table is not finite", who, a);
    if (N > kMaxPoints) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, kMaxPoints);
    SG_REQUIRE(L <= N, "%s: %d labels of %d points", who, L, N);
    if (d_all && (long long)L * A > (long long)kMaxAll)
        return sg::fail(SG_EUNSUP, "%s: d_all holds at most 2^24 (label, angle) rows (%d x %d)", who, L, A);
    if (L == 0) return SG_OK;
    SG_REQUIRE(d_xyz && d_order && d_start && d_best && d_ext && d_ws, "%s: bad arguments", who);
    const size_t need = sg_label_yaw_boxes_ws_bytes(N, L, A);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    hipStream_t st = sg::as_stream(stream);
    sg::Carver cv(d_ws, ws_bytes);
    Table t;
    sgos::StageClock<1> clock(st, t_label.timing, t_label.us + 2);
    if (int rc = make_table(who, cv, d_start, N, L, st, &t)) return rc;
    double* d_cs = cv.take<double>((size_t)A * 2);
    double* part = cv.take<double>(part_rows(N) * (size_t)A * 4);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    SG_HIP(hipMemcpyAsync(d_cs, h_cs, (size_t)A * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    k_lb_yaw<<<t.grid, kBlock, 0, st>>>(d_xyz, stride, N, d_order, d_start, L, t.lab_of, t.coff, t.poff, d_cs, A, d_best, d_ext, d_all, part, &t.land->flag);
    k_lb_yaw_fold<<<L, kWave, 0, st>>>(t.cnt, t.poff, L, A, part, d_best, d_ext, d_all);
    clock.tick();
    return land_flag(who, t, st);                                         // the synchronisation also ends the copy out of h_cs
}

size_t sg_label_frame_extents_ws_bytes(int N, int L) {
    if (!sizes_ok(N, L)) return 0;
    return table_bytes(N, L) + sg::align_up(part_rows(N) * 6 * sizeof(double));
}

int sg_label_frame_extents(const float* d_xyz, int stride, int N, const int32_t* d_order, const int32_t* d_start, int L, const double* d_frame,
                           double* d_ext, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_label_frame_extents";
    SG_REQUIRE(N >= 0 && L >= 0 && stride >= 3, "%s: bad arguments (%d points in rows of %d floats, %d labels)", who, N, stride, L);
    if (N > kMaxPoints) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, kMaxPoints);
    SG_REQUIRE(L <= N, "%s: %d labels of %d points", who, L, N);
    if (L == 0) return SG_OK;
    SG_REQUIRE(d_xyz && d_order && d_start && d_frame && d_ext && d_ws, "%s: bad arguments", who);
    const size_t need = sg_label_frame_extents_ws_bytes(N, L);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    hipStream_t st = sg::as_stream(stream);
    sg::Carver cv(d_ws, ws_bytes);
    Table t;
    sgos::StageClock<1> clock(st, t_label.timing, t_label.us + 3);
    if (int rc = make_table(who, cv, d_start, N, L, st, &t)) return rc;
    double* part = cv.take<double>(part_rows(N) * 6);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    k_lb_frame<<<t.grid, kBlock, 0, st>>>(d_xyz, stride, N, d_order, d_start, L, t.lab_of, t.coff, t.poff, d_frame, d_ext, part, &t.land->flag);
    k_lb_frame_fold<<<sg::cdiv((long long)L * 8, kBlock), kBlock, 0, st>>>(t.cnt, t.poff, L, part, d_ext);
    clock.tick();
    return land_flag(who, t, st);
}

}  // extern "C"
