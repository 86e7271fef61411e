// Non-maximum suppression of upright boxes, device side: the greedy rule of include/seggroup_hip.h over the one pair
// function of box_iou_device.h, so a suppression bit is the matrix entry of sg_box_iou thresholded.
//
//   k_nm_check         one thread a box: the box tests of k_bi_check and a score that is not finite -> a bit of the flag word
//   k_nm_rank          one workgroup of 256 threads takes up to 256 consecutive boxes of ONE scene (the host's workgroup table says which);
//                      the scene's scores go through LDS in tiles of 256 and are read as a broadcast.  rank_j = #{i : s_i > s_j, or
//                      s_i == s_j and i < j}: a comparison of doubles, so ties and -0.0 are right by construction.  The thread also writes
//                      the inverse (the original index at its rank) and carries its box and class to its rank: what follows reads in
//                      rank order without a gather.
//   k_nm_mask          one workgroup of four waves a 64 x 64 tile of the upper triangle of a scene in RANK order, the diagonal tiles included;
//                      the tile's scene is bisected in the tile offsets and (tile row, tile column) in the triangle's row starts.  A lane is a
//                      COLUMN j and keeps its box in registers; the tile's 64 row boxes and classes sit in LDS and are read as a broadcast; a
//                      wave takes 16 of the rows, one after the other.  Bit (i, j) = j after i, the classes agree, the z intervals overlap
//                      (the header's own two statements: where h is not positive the sequence gives exactly 0) and pair_iou(i, j) > thresh;
//                      a row's 64-bit word is the wave's ballot, and lane q writes the word of the wave's row q.
//   k_nm_scan          one wave a scene.  The scene's `removed` bit set is four words a lane (2^14 boxes = 256 words).  Per block of 64
//                      ranks: lane b holds the DIAGONAL word of row b (asked for a block ahead), the block is resolved in 64 steps that
//                      touch no memory (the word of step b comes from its lane by a read-lane, the running set sits in scalar registers),
//                      then the rows of the block's KEPT ranks are ORed into the rest of `removed`, eight independent loads at a time.
//                      The bits a kept row newly sets (row & ~removed) get that row's RANK as their representative, in LDS (four bytes
//                      a box of the call's longest scene): stores only, nothing waits for them.  keep and rep are written at the end,
//                      through the inverse order, all lanes at once.
// Double arithmetic, nothing contracted (-ffp-contract=off), no floating-point atomics; the only atomic is the integer OR into the flag
// word.  The offsets, the workgroup table and the cleared flag word are ONE upload.
#include <cmath>
#include <vector>

#include "sg_common.h"
#include "box_iou_device.h"

namespace {

using namespace sg_box;

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kMaxScene = 1 << 14;            // boxes of one scene: 256 words a bit row, four a lane of the scan
constexpr long long kMaxWords = 1ll << 24;    // the bit matrix: 128 MB
constexpr int kRemWords = kMaxScene / 64 / kWave;   // words of `removed` a lane holds: 4
constexpr int kMaskRows = kWave / (kBlock / kWave);   // rows of a tile a wave of k_nm_mask takes: 16
constexpr int kAhead = 8;                     // independent row loads in flight in the scan
constexpr int kScore = 8;                     // the flag word: upright_flags' three bits and this one
constexpr int kPad = 64;                      // the sections of the upload start at multiples of 256 bytes

typedef unsigned long long u64;

__global__ __launch_bounds__(kBlock) void k_nm_check(const double* __restrict__ box, const double* __restrict__ score, int K, int* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    int bad = upright_flags(box + (size_t)i * 8);
    if (!finite_f64(score[i])) bad |= kScore;
    if (bad) atomicOr(flag, bad);
}

// A score that is not a number is refused through the flag word; until then it ranks as -inf, so that the predicate stays a total order
// and the ranks of a scene a permutation: what follows reads `order` at every rank.
__device__ __forceinline__ double orderable(double s) { return s != s ? -INFINITY : s; }

__global__ __launch_bounds__(kBlock) void k_nm_rank(const double* __restrict__ box, const double* __restrict__ score, const int32_t* __restrict__ cls,
                                                    const int4* __restrict__ jobs, int32_t* __restrict__ rank, int32_t* __restrict__ order,
                                                    double* __restrict__ sbox, int32_t* __restrict__ scls) {
    __shared__ double tile[kBlock];
    const int4 job = jobs[blockIdx.x];                       // x: first box, y: boxes (1..256), z: the scene's first box, w: its end
    const int t = threadIdx.x;
    const bool live = t < job.y;
    const int i = job.x + t;                                 // < K where live: the host laid the table out from checked offsets
    const int li = i - job.z;
    const double si = live ? orderable(score[i]) : 0.0;
    int before = 0;
    for (int at = job.z; at < job.w; at += kBlock) {         // uniform over the workgroup
        const int nb = min(kBlock, job.w - at);
        if (t < nb) tile[t] = orderable(score[at + t]);
        __syncthreads();
        const int l0 = at - job.z;
#pragma unroll 8                                               // eight LDS reads in flight: a workgroup is alone on its CU for a long scene
        for (int j = 0; j < nb; ++j) {
            const double sj = tile[j];                       // the same address in every lane
            before += (int)(sj > si) | ((int)(sj == si) & (int)(l0 + j < li));      // no branch: three compares and two integer operations
        }
        __syncthreads();
    }
    if (!live) return;
    // before <= n - 1 whatever the scores hold (a box never counts itself), so every write below stays inside the scene
    rank[i] = before;
    const int at = job.z + before;
    order[at] = li;
#pragma unroll
    for (int r = 0; r < 8; ++r) sbox[(size_t)at * 8 + r] = box[(size_t)i * 8 + r];
    if (cls) scls[at] = cls[i];
}

// row ti of the upper triangle of T x T tiles starts at tile ti*T - ti*(ti-1)/2 and has T - ti tiles
__device__ __forceinline__ int row_start(int ti, int T) { return ti * T - ti * (ti - 1) / 2; }

__global__ __launch_bounds__(kBlock) void k_nm_mask(const double* __restrict__ sbox, const int32_t* __restrict__ scls, const int32_t* __restrict__ off,
                                                    const int32_t* __restrict__ woff, const int32_t* __restrict__ toff, int B, double thresh,
                                                    u64* __restrict__ mask) {
    __shared__ double rbox[kWave * 8];
    __shared__ int32_t rcls[kWave];
    const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    const int tile = blockIdx.x;                             // < toff[B]: the grid is the tile count
    const int s = scene_of(toff, B, tile);
    const int first = off[s], n = off[s + 1] - first;
    const int T = (n + kWave - 1) / kWave;
    const int r = tile - toff[s];
    int lo = 0, hi = T - 1;                                   // the last row ti with row_start(ti) <= r
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (row_start(mid, T) <= r) lo = mid; else hi = mid - 1;
    }
    const int ti = lo, tj = ti + (r - row_start(ti, T));      // ti <= tj < T
    if (t < kWave && ti * kWave + t < n) {                    // the tile's rows: the EARLIER boxes, `a` of the pair function
#pragma unroll
        for (int k = 0; k < 8; ++k) rbox[t * 8 + k] = sbox[(size_t)(first + ti * kWave + t) * 8 + k];
        rcls[t] = scls ? scls[first + ti * kWave + t] : 0;
    }
    __syncthreads();
    const int j = tj * kWave + lane;                          // this lane's column: the LATER box, `b`
    const bool live = j < n;
    double b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = live ? sbox[(size_t)(first + j) * 8 + k] : 0.0;
    const int cb = (live && scls) ? scls[first + j] : 0;
    const double hbz = 0.5 * b[5];
    const double btop = b[2] + hbz, bbot = b[2] - hbz;
    const int r0 = wave * kMaskRows;
    const int nr = min(kMaskRows, n - ti * kWave - r0);       // may be <= 0: a wave past the scene's last row has nothing to do
    u64 mine = 0;                                             // lane q keeps the word of the wave's row q
    for (int q = 0; q < nr; ++q) {                            // uniform over the wave
        const double* a = rbox + (r0 + q) * 8;                // the same address in every lane
        const int i = ti * kWave + r0 + q;
        bool cand = live && j > i && rcls[r0 + q] == cb;
        if (cand) {
            const double haz = 0.5 * a[5];
            const double top = fmin(a[2] + haz, btop), bottom = fmax(a[2] - haz, bbot);
            const double h = top - bottom;
            cand = h > 0.0;                                   // else inter = area * 0 and the IoU is exactly 0, or not a number: no bit
        }
        const u64 word = __ballot(cand && pair_iou(a, b) > thresh);
        if (lane == q) mine = word;
    }
    if (lane < nr) mask[(size_t)woff[s] + (size_t)(ti * kWave + r0 + lane) * T + tj] = mine;
}

// the word lane `src` holds, in every lane; `src` is uniform over the wave, so this is two read-lanes into scalar registers
__device__ __forceinline__ u64 lane_word(u64 v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return (u64)hi << 32 | lo;
}

__global__ __launch_bounds__(kWave) void k_nm_scan(const u64* __restrict__ mask, const int32_t* __restrict__ order, const int32_t* __restrict__ off,
                                                   const int32_t* __restrict__ woff, int32_t* __restrict__ keep, int32_t* __restrict__ rep) {
    extern __shared__ int32_t by_rank[];                      // per rank of the scene the RANK of its representative: the call's longest scene
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    const int first = off[s], n = off[s + 1] - first;
    if (n == 0) return;
    const int T = (n + kWave - 1) / kWave;                    // <= 256
    const u64* rows = mask + woff[s];
    u64 rem[kRemWords];                                       // word w of `removed` is rem[w / 64] of lane w % 64
#pragma unroll
    for (int q = 0; q < kRemWords; ++q) rem[q] = 0;
    u64 diag = lane < n ? rows[(size_t)lane * T] : 0;         // block 0's diagonal words
    for (int blk = 0; blk < T; ++blk) {
        const int base = blk * kWave;
        const int nb = min(kWave, n - base);
        const int row = base + lane;
        // the next block's diagonal words do not depend on this block: asked for now, used in the next turn
        const u64 next = row + kWave < n ? rows[(size_t)(row + kWave) * T + blk + 1] : 0;
        u64 mine = 0;
#pragma unroll
        for (int q = 0; q < kRemWords; ++q)
            if (q == blk / kWave) mine = rem[q];
        const u64 before = lane_word(mine, blk % kWave);      // this block's bits that earlier blocks set; uniform
        u64 gone = before, kept = 0;
        int by = lane;                                        // the rank within the block that suppressed this lane's box
#pragma unroll
        for (int b = 0; b < kWave; ++b) {
            const u64 d = lane_word(diag, b);                 // uniform: 0 for b >= nb
            if (b < nb && !(gone >> b & 1)) {
                kept |= 1ull << b;
                if ((d & ~gone) >> lane & 1) by = b;
                gone |= d;
            }
        }
        if (lane < nb && !(before >> lane & 1)) by_rank[row] = base + by;    // a box an earlier block suppressed has its entry already
        // the rows of the kept ranks into the words after this block's, in rank order, kAhead loads at a time
#pragma unroll
        for (int q = 0; q < kRemWords; ++q) {
            const int w = q * kWave + lane;
            if (q * kWave + kWave - 1 <= blk || q * kWave >= T) continue;     // uniform
            const bool mineq = w > blk && w < T;
            u64 left = kept;
            while (left) {                                    // uniform
                int rr[kAhead];
                u64 got[kAhead];
#pragma unroll
                for (int k = 0; k < kAhead; ++k) {
                    rr[k] = left ? __ffsll((long long)left) - 1 : -1;
                    if (left) left &= left - 1;
                }
#pragma unroll
                for (int k = 0; k < kAhead; ++k) got[k] = (mineq && rr[k] >= 0) ? rows[(size_t)(base + rr[k]) * T + w] : 0;
#pragma unroll
                for (int k = 0; k < kAhead; ++k) {
                    u64 fresh = got[k] & ~rem[q];
                    rem[q] |= got[k];
                    while (fresh) {
                        by_rank[w * kWave + __ffsll((long long)fresh) - 1] = base + rr[k];      // < n: the mask sets no bit past the scene
                        fresh &= fresh - 1;
                    }
                }
            }
        }
        diag = next;
    }
    __syncthreads();                                          // one wave: every entry of by_rank is written before it is read
    const int32_t* ord = order + first;
    for (int j = lane; j < n; j += kWave) {                   // through the inverse order; the turns do not depend on one another
        const int me = ord[j], r = by_rank[j];
        keep[first + me] = r == j ? 1 : 0;
        rep[first + me] = ord[r];
    }
}

bool sizes_ok(int K, int B, long long words) { return K >= 0 && K <= sg::kMaxBoxes && B >= 0 && B <= sg::kMaxScenes && words >= 0 && words <= kMaxWords; }

size_t pad(size_t ints) { return (ints + kPad - 1) / kPad * kPad; }
size_t job_entries(int K, int B) { return (size_t)sg::cdiv(K, kBlock) + (size_t)B; }
// flag word | off | woff | toff | the workgroup table of k_nm_rank: one upload
size_t table_ints(int K, int B) { return kPad + 3 * pad((size_t)B + 1) + pad(4 * job_entries(K, B)); }
size_t need_bytes(int K, int B, long long words) {
    const size_t k = (size_t)std::max(K, 1);
    return sg::align_up(table_ints(K, B) * sizeof(int32_t)) + 2 * sg::align_up(k * sizeof(int32_t)) + sg::align_up(k * 8 * sizeof(double)) +
           sg::align_up((size_t)std::max(words, 1ll) * sizeof(u64));
}

}  // namespace

extern "C" {

size_t sg_box_nms_ws_bytes(int K, int B, long long words) { return sizes_ok(K, B, words) ? need_bytes(K, B, words) : 0; }

int sg_box_nms(const double* d_box, const double* d_score, const int32_t* d_cls, int K, const int32_t* h_off, int B, double thresh,
               int32_t* d_rank, int32_t* d_keep, int32_t* d_rep, long long words, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_box_nms";
    SG_REQUIRE(K >= 0 && B >= 0 && h_off, "%s: bad arguments (%d boxes, %d scenes, a null pointer for the offsets)", who, K, B);
    if (K > sg::kMaxBoxes || B > sg::kMaxScenes)
        return sg::fail(SG_EUNSUP, "%s: %d boxes in %d scenes; a call takes at most 2^20 boxes and 2^16 scenes", who, K, B);
    if (int rc = sg::check_offsets(who, "the boxes", h_off, B, K)) return rc;
    SG_REQUIRE(std::isfinite(thresh) && thresh >= 0.0 && thresh < 1.0, "%s: the threshold is not finite or outside [0, 1) (%g)", who, thresh);
    long long sum = 0, tiles = 0, longest = 0;
    for (int s = 0; s < B; ++s) {
        const long long n = h_off[s + 1] - h_off[s], T = (n + kWave - 1) / kWave;
        if (n > kMaxScene) return sg::fail(SG_EUNSUP, "%s: scene %d has %lld boxes; a scene takes at most 2^14", who, s, n);
        sum += n * T;
        tiles += T * (T + 1) / 2;
        longest = std::max(longest, n);
    }
    if (sum > kMaxWords)
        return sg::fail(SG_EUNSUP, "%s: the bit matrix has %lld words; a call takes at most 2^24 (the sum over scenes of n * ceil(n / 64))", who, sum);
    SG_REQUIRE(words == sum, "%s: `words` is %lld and the scenes' sum of n * ceil(n / 64) is %lld", who, words, sum);
    if (K == 0) return SG_OK;
    SG_REQUIRE(d_box && d_score && d_rank && d_keep && d_rep && d_ws, "%s: bad arguments (a null pointer)", who);
    const size_t need = need_bytes(K, B, words);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    int32_t* table = cv.take<int32_t>(table_ints(K, B));
    int32_t* order = cv.take<int32_t>((size_t)K);
    int32_t* scls = cv.take<int32_t>((size_t)K);
    double* sbox = cv.take<double>((size_t)K * 8);
    u64* mask = cv.take<u64>((size_t)words);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const size_t nB = pad((size_t)B + 1);
    std::vector<int32_t> host(table_ints(K, B), 0);          // alive until the call has synchronised; entry 0 is the cleared flag word
    int32_t *h_o = host.data() + kPad, *h_w = h_o + nB, *h_t = h_w + nB, *h_j = h_t + nB;
    int jobs = 0;
    long long wat = 0, tat = 0;
    for (int s = 0; s <= B; ++s) {
        h_o[s] = h_off[s];
        h_w[s] = (int32_t)wat;
        h_t[s] = (int32_t)tat;
        if (s == B) break;
        const long long n = h_off[s + 1] - h_off[s], T = (n + kWave - 1) / kWave;
        wat += n * T;
        tat += T * (T + 1) / 2;
        for (int at = h_off[s]; at < h_off[s + 1]; at += kBlock, ++jobs) {
            h_j[4 * jobs] = at;
            h_j[4 * jobs + 1] = std::min(kBlock, h_off[s + 1] - at);
            h_j[4 * jobs + 2] = h_off[s];
            h_j[4 * jobs + 3] = h_off[s + 1];
        }
    }
    hipStream_t st = sg::as_stream(stream);
    const size_t used = (size_t)(h_j - host.data()) + 4 * (size_t)jobs;
    SG_HIP(hipMemcpyAsync(table, host.data(), used * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int* flag = table;
    const int32_t *d_off = table + kPad, *d_woff = d_off + nB, *d_toff = d_woff + nB;
    const int4* d_jobs = reinterpret_cast<const int4*>(d_toff + nB);
    k_nm_check<<<sg::cdiv(K, kBlock), kBlock, 0, st>>>(d_box, d_score, K, flag);
    k_nm_rank<<<jobs, kBlock, 0, st>>>(d_box, d_score, d_cls, d_jobs, d_rank, order, sbox, d_cls ? scls : nullptr);
    k_nm_mask<<<(int)tiles, kBlock, 0, st>>>(sbox, d_cls ? scls : nullptr, d_off, d_woff, d_toff, B, thresh, mask);
    k_nm_scan<<<B, kWave, (size_t)longest * sizeof(int32_t), st>>>(mask, order, d_off, d_woff, d_keep, d_rep);
    int land[4] = {0, 0, 0, 0};
    const hipError_t copied = hipMemcpyAsync(land, table, sizeof(land), hipMemcpyDeviceToHost, st);
    SG_HIP(hipStreamSynchronize(st));                         // whatever the copy said: the upload out of `host` ends here
    SG_HIP(copied);
    SG_LAUNCH_CHECK();
    // a value that is not finite comes first, then the score, then what upright_refusal lists after it
    if (!(land[0] & kNotFinite) && (land[0] & kScore)) return sg::fail(SG_EINVAL, "%s: a score is not finite", who);
    return upright_refusal(who, nullptr, land[0]);
}

}  // extern "C"
