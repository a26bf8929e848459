// pileup.hip -- `gffx coverage --mean-depth`: the bases that the source rows lay on feature segments.
//      bases(a, b) = sum over the rows [s, e) of the segment's seqid of max(0, min(e, b) - max(s, a))
// The quantity is a sum over rows, so the rows may arrive in any grouping: every fold of at most kPileupFold rows adds its
// own share to the segments' totals, nothing is folded between batches, and the totals of several devices are added as
// integers.  One fold, on the pileup's own stream (pileup_core.hpp has the rule and why it needs no array over the bases):
//   k_pileup_keys       rows {seqid, s, e} -> two W = 2 record arrays {seqid, s} and {seqid, e}; a row with s >= e or
//                       seqid >= n_seq sets the error word (the union builder's bits: coverage.hip)
//   DeviceSort x 2      each array by (seqid, coordinate), on its own (radix_sort.hpp)
//   k_pileup_tile_sums  per tile of kPileupScanTile records the sum of the coordinates (both arrays: blockIdx.y)
//   k_pileup_carry      one block per array: exclusive sum over the tiles (reduce-then-scan: nothing spins anywhere)
//   k_pileup_apply      the coordinates as a plain u32 array and their n + 1 exclusive u64 prefix sums
//   k_pileup_offsets    off[c] = the records with seqid < c, c = 0 .. n_seq: one search per seqid
//   k_pileup_segments   one thread per segment (resident since _create, in the order given: neighbours search neighbouring
//                       keys): four lower bounds inside [off[c], off[c + 1]), acc[i] += B(b) - B(a) as a plain 64-bit store.
//                       The thread owns its segment and folds are serialised on the stream: no atomics.
//   k_pileup_meta       (only after _meta_set: `gffx meta`) one wave per feature, kMetaTile features per block: the
//                       B + 1 column boundaries of meta_core.hpp, 64 at a time, one per lane; B(x) once per boundary, a column
//                       as the difference of two neighbouring lanes.  The feature's searches are confined first: four searches
//                       by the whole wave (64 probes a step) find where the window's two ends fall among the starts and the
//                       ends, and a lane's own two searches run inside that.  Column sums: LDS, then one 64-bit atomic add per
//                       column and block (integers: any order gives the same bits); the matrix, if kept: plain stores, the
//                       wave owns its feature's row.
// Roofline bound: the sorts HBM (8 W bytes per record and pass), the segment kernel latency (dependent gathers, like Join A).
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "gffx_device.hpp"
#include "handle_status.hpp"
#include "meta_core.hpp"
#include "pileup_core.hpp"
#include "radix_sort.hpp"
#include "regions_store.hpp"

namespace gffx {

constexpr int kPileupThreads = 256;
constexpr uint32_t kPileupScanTile = 4 * kPileupThreads;  // 4 consecutive records per thread: two 16-byte loads
constexpr uint64_t kPileupFold = 4ull << 20;              // rows per fold (the default batch of `gffx coverage`)
constexpr uint32_t kPileupErrRange = 2u;                  // err word: a row with seqid >= n_seq (the sort's own bit for it)
constexpr uint32_t kPileupErrInverted = 8u;               // ... with start >= end (4 is the sort's time-out)
constexpr uint32_t kMetaMaxColumns = 4096;                // k_pileup_meta's column sums in LDS: 32 KB of u64
constexpr uint32_t kMetaTile = 64;                        // features per block of k_pileup_meta: 16 per wave
constexpr uint32_t kMetaGeometrySlice = 1024;             // features per block of k_pileup_meta_geometry

// rows [i0, i0 + 4) -> their key records.  wide: `rows` is 16-byte aligned (a region-store slot that starts at a row that is
// no multiple of four is not)
__global__ __launch_bounds__(kPileupThreads) void k_pileup_keys(const uint32_t *rows, u64 n, uint32_t n_seq, int wide, uint32_t *ks, uint32_t *ke,
                                                                uint32_t *err) {
    const u64 i0 = 4ull * ((u64)blockIdx.x * kPileupThreads + threadIdx.x);
    if (i0 >= n) return;
    const bool full = i0 + 4 <= n;
    uint32_t w[12];
    if (full && wide) {
        const uint4 *p = reinterpret_cast<const uint4 *>(rows + 3 * i0);
        const uint4 a = p[0], b = p[1], c = p[2];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w, w[8] = c.x, w[9] = c.y,
        w[10] = c.z, w[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = (i0 + k / 3 < n) ? rows[3 * i0 + k] : 0u;
    }
    bool inverted = false, range = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) {
            inverted |= w[3 * j + 1] >= w[3 * j + 2];
            range |= w[3 * j] >= n_seq;
        }
    if (full) {  // (32 i0 bytes into a hipMalloc'd buffer: 16-byte aligned)
        uint4 *ps = reinterpret_cast<uint4 *>(ks + 2 * i0), *pe = reinterpret_cast<uint4 *>(ke + 2 * i0);
        ps[0] = make_uint4(w[0], w[1], w[3], w[4]);
        ps[1] = make_uint4(w[6], w[7], w[9], w[10]);
        pe[0] = make_uint4(w[0], w[2], w[3], w[5]);
        pe[1] = make_uint4(w[6], w[8], w[9], w[11]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) {
                ks[2 * (i0 + j)] = w[3 * j], ks[2 * (i0 + j) + 1] = w[3 * j + 1];
                ke[2 * (i0 + j)] = w[3 * j], ke[2 * (i0 + j) + 1] = w[3 * j + 2];
            }
    }
    if (range) atomicOr(err, kPileupErrRange);
    if (inverted) atomicOr(err, kPileupErrInverted);
}

// the coordinate words of records [i0, i0 + 4) of a sorted {seqid, coordinate} array (0 beyond n)
__device__ __forceinline__ void pileup_load(const uint32_t *rec, u64 n, u64 i0, uint32_t (&c)[4]) {
    if (i0 + 4 <= n) {
        const uint4 *p = reinterpret_cast<const uint4 *>(rec + 2 * i0);
        const uint4 a = p[0], b = p[1];
        c[0] = a.y, c[1] = a.w, c[2] = b.y, c[3] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = i0 + j < n ? rec[2 * (i0 + j) + 1] : 0u;
    }
}

// exclusive sum of v over the block's 256 threads; *total = the block's whole.  s_w: 4 words
__device__ __forceinline__ u64 pileup_block_scan(u64 v, u64 *s_w, u64 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 base = 0, all = 0;
#pragma unroll
    for (int x = 0; x < kPileupThreads / 64; ++x) {
        if (x < wave) base += s_w[x];
        all += s_w[x];
    }
    *total = all;
    return base + inc - v;
}

// blockIdx.y = 0: the starts, 1: the ends.  tile_sum[y * tiles + tile]
__global__ __launch_bounds__(kPileupThreads) void k_pileup_tile_sums(const uint32_t *rec_s, const uint32_t *rec_e, u64 n, u64 *tile_sum) {
    __shared__ u64 s_w[kPileupThreads / 64];
    const uint32_t *rec = blockIdx.y ? rec_e : rec_s;
    uint32_t c[4];
    pileup_load(rec, n, (u64)blockIdx.x * kPileupScanTile + 4ull * threadIdx.x, c);
    u64 total;
    (void)pileup_block_scan((u64)c[0] + c[1] + c[2] + c[3], s_w, &total);
    if (threadIdx.x == 0) tile_sum[(u64)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one block per array: its tile sums <- their exclusive sum, in place
__global__ __launch_bounds__(kPileupThreads) void k_pileup_carry(u64 *tile_sum, uint32_t tiles) {
    __shared__ u64 s_w[kPileupThreads / 64];
    u64 *v = tile_sum + (u64)blockIdx.x * tiles;
    u64 run = 0;
    for (uint32_t base = 0; base < tiles; base += kPileupThreads) {
        const uint32_t i = base + threadIdx.x;
        u64 all;
        const u64 ex = pileup_block_scan(i < tiles ? v[i] : 0ull, s_w, &all);
        if (i < tiles) v[i] = run + ex;
        run += all;
        __syncthreads();  // (s_w is rewritten by the next step)
    }
}

// co[i] = coordinate of sorted record i; pre[i] = sum of the coordinates of records [0, i), i = 0 .. n
__global__ __launch_bounds__(kPileupThreads) void k_pileup_apply(const uint32_t *rec_s, const uint32_t *rec_e, u64 n, const u64 *carry, uint32_t *co_s,
                                                                 uint32_t *co_e, u64 *pre_s, u64 *pre_e) {
    __shared__ u64 s_w[kPileupThreads / 64];
    const uint32_t *rec = blockIdx.y ? rec_e : rec_s;
    uint32_t *co = blockIdx.y ? co_e : co_s;
    u64 *pre = blockIdx.y ? pre_e : pre_s;
    const u64 i0 = (u64)blockIdx.x * kPileupScanTile + 4ull * threadIdx.x;
    uint32_t c[4];
    pileup_load(rec, n, i0, c);
    u64 total;
    u64 run = carry[(u64)blockIdx.y * gridDim.x + blockIdx.x] + pileup_block_scan((u64)c[0] + c[1] + c[2] + c[3], s_w, &total);
    if (i0 + 4 <= n) {  // (16 i0 and 32 i0 bytes into hipMalloc'd buffers)
        *reinterpret_cast<uint4 *>(co + i0) = make_uint4(c[0], c[1], c[2], c[3]);
        const u64 p1 = run + c[0], p2 = p1 + c[1], p3 = p2 + c[2];
        ulonglong2 *pp = reinterpret_cast<ulonglong2 *>(pre + i0);
        pp[0] = make_ulonglong2(run, p1);
        pp[1] = make_ulonglong2(p2, p3);
        if (i0 + 4 == n) pre[n] = p3 + c[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) {
                co[i0 + j] = c[j], pre[i0 + j] = run;
                run += c[j];
                if (i0 + j + 1 == n) pre[n] = run;
            }
    }
}

// off[c] = the records with seqid < c (the same for both arrays: they hold the same seqids)
__global__ __launch_bounds__(kPileupThreads) void k_pileup_offsets(const uint32_t *rec, u64 n, uint32_t n_seq, u64 *off) {
    const u64 c = (u64)blockIdx.x * kPileupThreads + threadIdx.x;
    if (c > n_seq) return;
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (rec[2 * mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    off[c] = lo;
}

__global__ __launch_bounds__(kPileupThreads) void k_pileup_segments(pileup::Keys K, const u64 *off, uint32_t n_seq, u64 n_seg, const uint32_t *seg_seq,
                                                                    const uint32_t *seg_start, const uint32_t *seg_end, u64 *acc) {
    const u64 i = (u64)blockIdx.x * kPileupThreads + threadIdx.x;
    if (i >= n_seg) return;
    const uint32_t c = seg_seq[i];
    if (c >= n_seq) return;  // (refused at _create)
    const u64 add = pileup::segment_bases(K, off[c], off[c + 1], seg_start[i], seg_end[i]);
    if (add) acc[i] += add;
}

// the features of `gffx meta`, resident since _meta_set, in the order given
struct MetaFeatures {
    const uint32_t *seq, *start, *end;
    const uint8_t *minus;
    const uint32_t *seq_len;  // n_seq lengths, or NULL: every seqid is 2^32 - 1 long
    u64 n;
};

// The first position p of [lo, hi) with keys[p] >= x (hi if none), found by the whole wave: 64 probes a step cut the range to a
// 65th, the last step looks at up to 64 neighbours.  lo, hi and x are the same in every lane and all 64 lanes are here.  Every
// probe lies inside [lo, hi).
__device__ __forceinline__ u64 meta_wave_lower_bound(const uint32_t *keys, u64 lo, u64 hi, uint32_t x, int lane) {
    while (hi - lo > 64) {
        const u64 n = hi - lo;  // (below 2^28: 65 n fits)
        const u64 below = __ballot(keys[lo + ((u64)(lane + 1) * n) / 65] < x);  // probes ascend with the lane: a prefix of the lanes
        const int c = __popcll(below);
        const u64 new_lo = c ? lo + ((u64)c * n) / 65 + 1 : lo;
        const u64 new_hi = c < 64 ? lo + ((u64)(c + 1) * n) / 65 : hi;
        lo = new_lo, hi = new_hi;  // (at most n / 65 + 1 wide: the loop ends)
    }
    const u64 p = lo + (u64)lane;
    return lo + (u64)__popcll(__ballot(p < hi && keys[p] < x));
}

// col_bases[j] += the bases this fold's rows lay on column j of every feature; matrix (or NULL): n x B, the same per feature.
// B <= kMetaMaxColumns words of dynamic LDS.
__global__ __launch_bounds__(kPileupThreads) void k_pileup_meta(pileup::Keys K, const u64 *off, uint32_t n_seq, MetaFeatures F, meta::Layout lay, uint32_t B,
                                                                u64 *col_bases, u64 *matrix) {
    extern __shared__ u64 s_col[];
    for (uint32_t j = threadIdx.x; j < B; j += kPileupThreads) s_col[j] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = wave; t < kMetaTile; t += kPileupThreads / 64) {  // (everything up to the column loop is the same in all lanes)
        const u64 i = (u64)blockIdx.x * kMetaTile + t;
        if (i >= F.n) break;
        const uint32_t c = F.seq[i];
        if (c >= n_seq) continue;  // (refused at _meta_set)
        const u64 lo = off[c], hi = off[c + 1];
        if (lo >= hi) continue;  // no row on the seqid in this fold
        const uint32_t s = F.start[i], e = F.end[i], len = F.seq_len ? F.seq_len[c] : 0xFFFFFFFFu;
        const bool minus = F.minus[i] != 0;
        const uint32_t x_first = meta::boundary(lay, s, e, minus, len, 0), x_last = meta::boundary(lay, s, e, minus, len, B);
        const uint32_t x_min = minus ? x_last : x_first, x_max = minus ? x_first : x_last;
        // every boundary x has x_min <= x <= x_max: its searches end inside [s_lo, s_hi] and [e_lo, e_hi]
        const u64 s_lo = meta_wave_lower_bound(K.starts, lo, hi, x_min, lane);
        const u64 s_hi = meta_wave_lower_bound(K.starts, s_lo, hi, x_max, lane);
        if (s_hi == lo) continue;  // no row starts below the window's end: B(x) = 0 all over it
        const u64 e_lo = meta_wave_lower_bound(K.ends, lo, hi, x_min, lane);
        if (e_lo == hi) continue;  // every row ends below the window: B(x) is the same all over it
        const u64 e_hi = meta_wave_lower_bound(K.ends, e_lo, hi, x_max, lane);
        const u64 base_s = K.pre_s[lo], base_e = K.pre_e[lo];
        for (uint32_t k0 = 0; k0 < B; k0 += 63) {  // boundaries k0 .. k0 + 63, columns k0 .. k0 + 62
            const uint32_t k = min(k0 + (uint32_t)lane, B);
            const uint32_t x = meta::boundary(lay, s, e, minus, len, k);
            const u64 ps = pileup::lower_bound(K.starts, s_lo, s_hi, x), pe = pileup::lower_bound(K.ends, e_lo, e_hi, x);
            const u64 below = pileup::bases_below(x, ps - lo, K.pre_s[ps] - base_s, pe - lo, K.pre_e[pe] - base_e);
            const u64 next = __shfl_down(below, 1, 64);
            if (lane < 63 && k0 + (uint32_t)lane < B) {
                const u64 add = minus ? below - next : next - below;
                if (add) {
                    atomicAdd(&s_col[k], add);
                    if (matrix) matrix[i * B + k] += add;
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < B; j += kPileupThreads)
        if (s_col[j]) atomicAdd(&col_bases[j], s_col[j]);
}

// what does not depend on the rows, once at _meta_set: col_len[j] = the clamped lengths of column j over the features,
// col_features[j] = the features whose column j is not empty.  blockIdx.x: a slice of kMetaGeometrySlice features, blockIdx.y: 256 columns
__global__ __launch_bounds__(kPileupThreads) void k_pileup_meta_geometry(uint32_t n_seq, MetaFeatures F, meta::Layout lay, uint32_t B, u64 *col_len,
                                                                         u64 *col_features) {
    const uint32_t j = blockIdx.y * kPileupThreads + threadIdx.x;
    if (j >= B) return;
    const u64 i0 = (u64)blockIdx.x * kMetaGeometrySlice, i1 = i0 + kMetaGeometrySlice < F.n ? i0 + kMetaGeometrySlice : F.n;
    u64 total = 0, features = 0;
    for (u64 i = i0; i < i1; ++i) {
        const uint32_t c = F.seq[i];
        if (c >= n_seq) continue;
        uint32_t a, b;
        meta::column(lay, F.start[i], F.end[i], F.minus[i] != 0, F.seq_len ? F.seq_len[c] : 0xFFFFFFFFu, j, &a, &b);
        total += b - a, features += b > a;
    }
    if (total) atomicAdd(&col_len[j], total), atomicAdd(&col_features[j], features);
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_pileup : gffx::HandleStatus {
    static constexpr const char *kName = "pileup", *kNoun = "pileup";
    uint32_t n_seq = 0;
    uint64_t n_seg = 0;
    hipStream_t stream = nullptr;
    // two folds in flight, each: 0 start, 1 keys done, 2 sorts start (the host looked at the error word in between), 3 sorts done,
    // 4 scan done, 5 segments done, 6 the error word is on the host, 7 the meta kernel done (recorded between 5 and 6)
    hipEvent_t ev[2][8] = {};
    hipEvent_t read = nullptr;  // the fold's rows have been read
    bool pending[2] = {false, false};  // ev[j] and h_ctl[j] wait to be looked at
    int next_set = 0;
    uint32_t *d_seg[3] = {nullptr, nullptr, nullptr};
    u64 *d_acc = nullptr;
    uint32_t *d_rows = nullptr;  // _add_host: the fold's rows
    uint64_t cap_rows = 0;
    uint32_t *ks[2] = {nullptr, nullptr}, *ke[2] = {nullptr, nullptr};  // the key records and the sort's second buffer
    uint32_t *co[2] = {nullptr, nullptr};                               // sorted coordinates: starts, ends
    u64 *pre[2] = {nullptr, nullptr};                                   // ... their n + 1 prefix sums
    u64 *tile_sum = nullptr, *off = nullptr;
    uint32_t *work = nullptr;
    uint64_t cap = 0, cap_work = 0, cap_tiles = 0;
    uint32_t *ctl = nullptr;    // device words {err, 7 x pad}
    uint32_t *h_ctl = nullptr;  // pinned, 3 x 8 words: the two folds in flight, the check after k_pileup_keys
    uint32_t *h_stage = nullptr;  // pinned
    uint64_t cap_stage = 0;
    SortPlan plan{};
    double stage_ms[4] = {0, 0, 0, 0};  // keys, the two sorts, scan (+ offsets), segments
    uint64_t rows_added = 0, folds = 0;
    // the second consumer (`gffx meta`): nothing of it exists before _meta_set
    bool meta = false, meta_matrix = false;
    uint64_t n_feat = 0;
    uint32_t meta_cols = 0;
    meta::Layout meta_layout{};
    uint32_t *d_feat[3] = {nullptr, nullptr, nullptr}, *d_seq_len = nullptr;
    uint8_t *d_feat_minus = nullptr;
    u64 *d_col = nullptr;  // 3 x meta_cols: bases, length, features
    u64 *d_matrix = nullptr;
    double meta_ms = 0;
};

namespace {

// the fold behind event set j is through: its stage times, and what the sort said
int pileup_collect(gffx_hip_pileup *P, int j) {
    if (!P->pending[j]) return GFFX_OK;
    P->pending[j] = false;
    GFFX_HIP_TRY(hipEventSynchronize(P->ev[j][6]));
    const int from[4] = {0, 2, 3, 4};
    for (int s = 0; s < 4; ++s) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, P->ev[j][from[s]], P->ev[j][s == 0 ? 1 : from[s] + 1]) == hipSuccess) P->stage_ms[s] += ms;
    }
    if (P->meta) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, P->ev[j][5], P->ev[j][7]) == hipSuccess) P->meta_ms += ms;
    }
    if (P->h_ctl[8 * j] & 4u) return fail(GFFX_E_HIP, "gffx_hip_pileup: the device sort timed out waiting for an earlier tile");
    return GFFX_OK;
}

// room for a fold of m rows
int pileup_reserve(gffx_hip_pileup *P, uint64_t m) {
    int rc;
    if (m > P->cap) {
        GFFX_HIP_TRY(hipStreamSynchronize(P->stream));  // (an earlier fold may still read what is freed here)
        const uint64_t cap = std::min<uint64_t>(kPileupFold, m + m / 4 + 1024);
        for (void *p : {(void *)P->ks[0], (void *)P->ks[1], (void *)P->ke[0], (void *)P->ke[1], (void *)P->co[0], (void *)P->co[1], (void *)P->pre[0],
                        (void *)P->pre[1], (void *)P->tile_sum, (void *)P->work})
            if (p) GFFX_HIP_TRY(hipFree(p));
        P->ks[0] = P->ks[1] = P->ke[0] = P->ke[1] = P->co[0] = P->co[1] = P->work = nullptr;
        P->pre[0] = P->pre[1] = P->tile_sum = nullptr;
        P->cap = P->cap_work = P->cap_tiles = 0;
        const uint64_t tiles = (cap + kPileupScanTile - 1) / kPileupScanTile;
        const uint64_t work = DeviceSort::work_words(cap, P->plan.n_passes);
        for (int k = 0; k < 2; ++k)
            if ((rc = dev_alloc_padded(&P->ks[k], 2 * cap)) || (rc = dev_alloc_padded(&P->ke[k], 2 * cap)) || (rc = dev_alloc_padded(&P->co[k], cap)) ||
                (rc = dev_alloc_padded(&P->pre[k], cap + 1)))
                return rc;
        if ((rc = dev_alloc_padded(&P->tile_sum, 2 * tiles)) || (rc = dev_alloc_padded(&P->work, work))) return rc;
        P->cap = cap, P->cap_work = work, P->cap_tiles = tiles;
    }
    return GFFX_OK;
}

// one fold: the m <= kPileupFold rows at `rows` (device memory; their copy, if any, is enqueued on the stream).  Returns when
// the rows have been read and found well-formed; the sorts, the scan and the segment kernel go on behind.  A refused row
// keeps ITS fold out of the totals; the folds of the same _add before it (an _add of more than kPileupFold rows) are in.
int pileup_fold(gffx_hip_pileup *P, const uint32_t *rows, uint64_t m) {
    if (!m) return GFFX_OK;
    const int j = P->next_set;
    int rc = pileup_collect(P, j);
    if (rc) return rc;
    const unsigned long long n = m;
    GFFX_HIP_TRY(hipMemsetAsync(P->ctl, 0, 32, P->stream));
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][0], P->stream));
    const int wide = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0;
    hipLaunchKernelGGL(k_pileup_keys, dim3((uint32_t)((n + 4 * kPileupThreads - 1) / (4 * kPileupThreads))), dim3(kPileupThreads), 0, P->stream, rows, n,
                       P->n_seq, wide, P->ks[0], P->ke[0], P->ctl);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][1], P->stream));
    uint32_t *h_now = P->h_ctl + 16;
    GFFX_HIP_TRY(hipMemcpyAsync(h_now, P->ctl, 32, hipMemcpyDeviceToHost, P->stream));
    GFFX_HIP_TRY(hipEventRecord(P->read, P->stream));
    GFFX_HIP_TRY(hipEventSynchronize(P->read));
    if (h_now[0] & kPileupErrRange) return fail(GFFX_E_CHR_RANGE, "gffx_hip_pileup: a row has chr >= %u", P->n_seq);
    if (h_now[0] & kPileupErrInverted) return fail(GFFX_E_INVALID, "gffx_hip_pileup: a row has start >= end");
    uint32_t *sorted_s = nullptr, *sorted_e = nullptr;
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][2], P->stream));
    if ((rc = DeviceSort::run<2>(P->stream, P->ks[0], P->ks[1], n, P->plan, P->n_seq, P->work, P->ctl, &sorted_s))) return rc;
    if ((rc = DeviceSort::run<2>(P->stream, P->ke[0], P->ke[1], n, P->plan, P->n_seq, P->work, P->ctl, &sorted_e))) return rc;
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][3], P->stream));
    const uint32_t tiles = (uint32_t)((n + kPileupScanTile - 1) / kPileupScanTile);
    hipLaunchKernelGGL(k_pileup_tile_sums, dim3(tiles, 2), dim3(kPileupThreads), 0, P->stream, sorted_s, sorted_e, n, P->tile_sum);
    hipLaunchKernelGGL(k_pileup_carry, dim3(2), dim3(kPileupThreads), 0, P->stream, P->tile_sum, tiles);
    hipLaunchKernelGGL(k_pileup_apply, dim3(tiles, 2), dim3(kPileupThreads), 0, P->stream, sorted_s, sorted_e, n, P->tile_sum, P->co[0], P->co[1], P->pre[0],
                       P->pre[1]);
    hipLaunchKernelGGL(k_pileup_offsets, dim3(P->n_seq / kPileupThreads + 1), dim3(kPileupThreads), 0, P->stream, sorted_s, n, P->n_seq, P->off);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][4], P->stream));
    if (P->n_seg) {
        const pileup::Keys K{P->co[0], P->co[1], P->pre[0], P->pre[1]};
        hipLaunchKernelGGL(k_pileup_segments, dim3((uint32_t)((P->n_seg + kPileupThreads - 1) / kPileupThreads)), dim3(kPileupThreads), 0, P->stream, K, P->off,
                           P->n_seq, (u64)P->n_seg, P->d_seg[0], P->d_seg[1], P->d_seg[2], P->d_acc);
        GFFX_HIP_TRY(hipGetLastError());
    }
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][5], P->stream));
    if (P->meta) {
        if (P->n_feat) {
            const pileup::Keys K{P->co[0], P->co[1], P->pre[0], P->pre[1]};
            const MetaFeatures F{P->d_feat[0], P->d_feat[1], P->d_feat[2], P->d_feat_minus, P->d_seq_len, (u64)P->n_feat};
            hipLaunchKernelGGL(k_pileup_meta, dim3((uint32_t)((P->n_feat + kMetaTile - 1) / kMetaTile)), dim3(kPileupThreads), P->meta_cols * sizeof(u64),
                               P->stream, K, P->off, P->n_seq, F, P->meta_layout, P->meta_cols, P->d_col, P->meta_matrix ? P->d_matrix : nullptr);
            GFFX_HIP_TRY(hipGetLastError());
        }
        GFFX_HIP_TRY(hipEventRecord(P->ev[j][7], P->stream));
    }
    GFFX_HIP_TRY(hipMemcpyAsync(P->h_ctl + 8 * j, P->ctl, 32, hipMemcpyDeviceToHost, P->stream));
    GFFX_HIP_TRY(hipEventRecord(P->ev[j][6], P->stream));
    P->pending[j] = true;
    P->next_set = j ^ 1;
    P->rows_added += m;
    P->folds++;
    return GFFX_OK;
}

// the meta consumer's device memory (the stream is idle)
void pileup_meta_free(gffx_hip_pileup *P) {
    for (void *p : {(void *)P->d_feat[0], (void *)P->d_feat[1], (void *)P->d_feat[2], (void *)P->d_seq_len, (void *)P->d_feat_minus, (void *)P->d_col,
                    (void *)P->d_matrix})
        if (p) (void)hipFree(p);
    P->d_feat[0] = P->d_feat[1] = P->d_feat[2] = P->d_seq_len = nullptr;
    P->d_feat_minus = nullptr;
    P->d_col = P->d_matrix = nullptr;
    P->meta = P->meta_matrix = false;
    P->n_feat = 0, P->meta_cols = 0;
}

// every fold enqueued so far is through and looked at
int pileup_drain(gffx_hip_pileup *P) {
    GFFX_HIP_TRY(hipStreamSynchronize(P->stream));
    for (int j = 0; j < 2; ++j) {
        const int rc = pileup_collect(P, j);
        if (rc) return rc;
    }
    return GFFX_OK;
}

}  // namespace

extern "C" uint64_t gffx_hip_pileup_fold_rows(void) { return kPileupFold; }
extern "C" uint32_t gffx_hip_pileup_scan_tile(void) { return kPileupScanTile; }
extern "C" uint32_t gffx_hip_pileup_meta_max_columns(void) { return kMetaMaxColumns; }
extern "C" uint32_t gffx_hip_pileup_meta_tile(void) { return kMetaTile; }

extern "C" uint64_t gffx_hip_pileup_meta_columns(const gffx_hip_meta_layout *layout) {
    if (!layout) return 0;
    return meta::columns(meta::Layout{layout->mode, layout->anchor, layout->up, layout->down, layout->bin, layout->body_bins});
}

extern "C" void gffx_hip_pileup_destroy(gffx_hip_pileup *P) {
    if (!P) return;
    (void)hipSetDevice(P->device);
    if (P->stream) (void)hipStreamSynchronize(P->stream);
    for (void *p : {(void *)P->d_seg[0], (void *)P->d_seg[1], (void *)P->d_seg[2], (void *)P->d_acc, (void *)P->d_rows, (void *)P->ks[0], (void *)P->ks[1],
                    (void *)P->ke[0], (void *)P->ke[1], (void *)P->co[0], (void *)P->co[1], (void *)P->pre[0], (void *)P->pre[1], (void *)P->tile_sum,
                    (void *)P->off, (void *)P->work, (void *)P->ctl})
        if (p) (void)hipFree(p);
    pileup_meta_free(P);
    if (P->h_stage) (void)hipHostFree(P->h_stage);
    if (P->h_ctl) (void)hipHostFree(P->h_ctl);
    for (auto &set : P->ev)
        for (hipEvent_t e : set)
            if (e) (void)hipEventDestroy(e);
    if (P->read) (void)hipEventDestroy(P->read);
    if (P->stream) (void)hipStreamDestroy(P->stream);
    delete P;
}

extern "C" int gffx_hip_pileup_create(int device, uint32_t n_seq, uint64_t n_seg, const uint32_t *seg_seq, const uint32_t *seg_start,
                                      const uint32_t *seg_end, gffx_hip_pileup **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_pileup_create: out is NULL");
    *out = nullptr;
    if (n_seg && (!seg_seq || !seg_start || !seg_end)) return fail(GFFX_E_INVALID, "gffx_hip_pileup_create: NULL segment array");
    if (n_seg >= (1ull << 32)) return fail(GFFX_E_INVALID, "gffx_hip_pileup_create: %llu segments exceed the limit of 2^32 - 1", (unsigned long long)n_seg);
    for (uint64_t i = 0; i < n_seg; i++)
        if (seg_seq[i] >= n_seq)
            return fail(GFFX_E_INVALID, "gffx_hip_pileup_create: segment %llu has chr %u >= %u", (unsigned long long)i, seg_seq[i], n_seq);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    if (ndev <= 0) return fail(GFFX_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFFX_E_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_pileup, void (*)(gffx_hip_pileup *)> P(new gffx_hip_pileup, gffx_hip_pileup_destroy);
    P->device = device;
    P->n_seq = n_seq;
    P->n_seg = n_seg;
    // by (seqid, coordinate): the four bytes of the coordinate, then as many bytes of the seqid as n_seq needs (the union's rule)
    int seq_bytes = 1;
    while (seq_bytes < 4 && (n_seq > (1u << (8 * seq_bytes)))) seq_bytes++;
    for (int b = 0; b < 4; ++b) P->plan.word[P->plan.n_passes] = 1, P->plan.shift[P->plan.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < seq_bytes; ++b) P->plan.word[P->plan.n_passes] = 0, P->plan.shift[P->plan.n_passes++] = (uint8_t)(8 * b);
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
    for (auto &set : P->ev)
        for (hipEvent_t &e : set) GFFX_HIP_TRY(hipEventCreate(&e));
    GFFX_HIP_TRY(hipEventCreateWithFlags(&P->read, hipEventDisableTiming));
    GFFX_HIP_TRY(hipHostMalloc((void **)&P->h_ctl, 3 * 32, hipHostMallocDefault));
    std::memset(P->h_ctl, 0, 3 * 32);
    int rc;
    if ((rc = dev_alloc_padded(&P->ctl, 8)) || (rc = dev_alloc_padded(&P->off, (uint64_t)n_seq + 1)) || (rc = dev_alloc_padded(&P->d_acc, n_seg))) return rc;
    for (uint32_t *&p : P->d_seg)
        if ((rc = dev_alloc_padded(&p, n_seg))) return rc;
    GFFX_HIP_TRY(hipMemsetAsync(P->d_acc, 0, std::max<uint64_t>(n_seg, 4) * 8, P->stream));
    if (n_seg) {
        GFFX_HIP_TRY(hipMemcpyAsync(P->d_seg[0], seg_seq, n_seg * 4, hipMemcpyHostToDevice, P->stream));
        GFFX_HIP_TRY(hipMemcpyAsync(P->d_seg[1], seg_start, n_seg * 4, hipMemcpyHostToDevice, P->stream));
        GFFX_HIP_TRY(hipMemcpyAsync(P->d_seg[2], seg_end, n_seg * 4, hipMemcpyHostToDevice, P->stream));
    }
    GFFX_HIP_TRY(hipStreamSynchronize(P->stream));  // (the caller's arrays are free again)
    *out = P.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_add_host(gffx_hip_pileup *P, const uint32_t *rows, uint64_t n_rows) {
    int rc = enter_handle(P, "gffx_hip_pileup_add_host");
    if (rc) return rc;
    if (n_rows && !rows) return fail(GFFX_E_INVALID, "gffx_hip_pileup_add_host: rows is NULL");
    const uint64_t want = std::min<uint64_t>(n_rows, kPileupFold);
    if (want > P->cap_stage) {
        if (P->h_stage) (void)hipHostFree(P->h_stage);
        P->h_stage = nullptr, P->cap_stage = 0;
        hipError_t e = hipHostMalloc((void **)&P->h_stage, want * 12, hipHostMallocDefault);
        if (e != hipSuccess)
            return keep_failure(P, fail(GFFX_E_OOM, "hipHostMalloc of a %llu-row staging buffer failed: %s", (unsigned long long)want, hipGetErrorString(e)));
        P->cap_stage = want;
    }
    if (want > P->cap_rows) {
        GFFX_KEEP_HIP(P, hipStreamSynchronize(P->stream));
        if (P->d_rows) GFFX_KEEP_HIP(P, hipFree(P->d_rows));
        P->d_rows = nullptr, P->cap_rows = 0;
        GFFX_KEEP_TRY(P, dev_alloc_padded(&P->d_rows, 3 * want));
        P->cap_rows = want;
    }
    for (uint64_t at = 0; at < n_rows; at += kPileupFold) {
        const uint64_t m = std::min<uint64_t>(kPileupFold, n_rows - at);
        GFFX_KEEP_TRY(P, pileup_reserve(P, m));
        std::memcpy(P->h_stage, rows + 3 * at, m * 12);  // (a fold returns after its rows were read: the buffer is free again)
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_rows, P->h_stage, m * 12, hipMemcpyHostToDevice, P->stream));
        GFFX_KEEP_TRY(P, pileup_fold(P, P->d_rows, m));
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_add_store(gffx_hip_pileup *P, const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows) {
    int rc = enter_handle(P, "gffx_hip_pileup_add_store");
    if (rc) return rc;
    const uint32_t *src = nullptr;
    if ((rc = store_slot_rows(R, k, first, n_rows, P->device, "gffx_hip_pileup_add_store", "pileup", &src))) return rc;
    if (R->pending[k]) GFFX_KEEP_HIP(P, hipStreamWaitEvent(P->stream, R->copied[k], 0));
    for (uint64_t at = 0; at < n_rows; at += kPileupFold) {
        const uint64_t m = std::min<uint64_t>(kPileupFold, n_rows - at);
        GFFX_KEEP_TRY(P, pileup_reserve(P, m));
        GFFX_KEEP_TRY(P, pileup_fold(P, src + 3 * at, m));  // (the slot is read in place: no copy)
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_copy(gffx_hip_pileup *P, uint64_t *bases) {
    int rc = enter_handle(P, "gffx_hip_pileup_copy");
    if (rc) return rc;
    if (P->n_seg && !bases) return fail(GFFX_E_INVALID, "gffx_hip_pileup_copy: bases is NULL");
    GFFX_KEEP_TRY(P, pileup_drain(P));
    if (P->n_seg) GFFX_KEEP_HIP(P, hipMemcpy(bases, P->d_acc, P->n_seg * 8, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_reset(gffx_hip_pileup *P) {
    int rc = enter_handle(P, "gffx_hip_pileup_reset");
    if (rc) return rc;
    GFFX_KEEP_HIP(P, hipMemsetAsync(P->d_acc, 0, std::max<uint64_t>(P->n_seg, 4) * 8, P->stream));  // (behind the folds enqueued so far)
    if (P->meta) {  // the column totals and the matrix; length and features are the features' own and stay
        GFFX_KEEP_HIP(P, hipMemsetAsync(P->d_col, 0, (size_t)P->meta_cols * 8, P->stream));
        if (P->meta_matrix) GFFX_KEEP_HIP(P, hipMemsetAsync(P->d_matrix, 0, std::max<uint64_t>(P->n_feat * P->meta_cols, 4) * 8, P->stream));
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_meta_set(gffx_hip_pileup *P, uint64_t n_feat, const uint32_t *feat_seq, const uint32_t *feat_start, const uint32_t *feat_end,
                                        const uint8_t *feat_minus, const uint32_t *seq_len, const gffx_hip_meta_layout *layout, int keep_matrix) {
    int rc = enter_handle(P, "gffx_hip_pileup_meta_set");
    if (rc) return rc;
    if (!layout) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: layout is NULL");
    if (n_feat && (!feat_seq || !feat_start || !feat_end || !feat_minus)) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: NULL feature array");
    if (n_feat >= (1ull << 32)) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: %llu features exceed the limit of 2^32 - 1", (unsigned long long)n_feat);
    const meta::Layout lay{layout->mode, layout->anchor, layout->up, layout->down, layout->bin, layout->body_bins};
    const uint64_t B = meta::columns(lay);
    if (!B)
        return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: no such layout (mode %u, anchor %u, up %u, down %u, bin %u, body bins %u)", lay.mode, lay.anchor, lay.up,
                    lay.down, lay.bin, lay.body_bins);
    if (B > kMetaMaxColumns) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: %llu columns exceed the limit of %u", (unsigned long long)B, kMetaMaxColumns);
    for (uint64_t i = 0; i < n_feat; i++) {
        if (feat_seq[i] >= P->n_seq)
            return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: feature %llu has chr %u >= %u", (unsigned long long)i, feat_seq[i], P->n_seq);
        if (feat_start[i] >= feat_end[i]) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_set: feature %llu has start >= end", (unsigned long long)i);
    }
    GFFX_KEEP_TRY(P, pileup_drain(P));  // (folds in flight read the features that are replaced here)
    pileup_meta_free(P);
    for (uint32_t *&p : P->d_feat) GFFX_KEEP_TRY(P, dev_alloc_padded(&p, n_feat));
    GFFX_KEEP_TRY(P, dev_alloc_padded(&P->d_feat_minus, n_feat));
    GFFX_KEEP_TRY(P, dev_alloc_padded(&P->d_col, 3 * B));
    if (seq_len) GFFX_KEEP_TRY(P, dev_alloc_padded(&P->d_seq_len, (uint64_t)P->n_seq));
    if (keep_matrix) GFFX_KEEP_TRY(P, dev_alloc_padded(&P->d_matrix, n_feat * B));
    if (n_feat) {
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_feat[0], feat_seq, n_feat * 4, hipMemcpyHostToDevice, P->stream));
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_feat[1], feat_start, n_feat * 4, hipMemcpyHostToDevice, P->stream));
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_feat[2], feat_end, n_feat * 4, hipMemcpyHostToDevice, P->stream));
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_feat_minus, feat_minus, n_feat, hipMemcpyHostToDevice, P->stream));
    }
    if (seq_len && P->n_seq) GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_seq_len, seq_len, (size_t)P->n_seq * 4, hipMemcpyHostToDevice, P->stream));
    GFFX_KEEP_HIP(P, hipMemsetAsync(P->d_col, 0, std::max<uint64_t>(3 * B, 4) * 8, P->stream));
    if (keep_matrix) GFFX_KEEP_HIP(P, hipMemsetAsync(P->d_matrix, 0, std::max<uint64_t>(n_feat * B, 4) * 8, P->stream));
    if (n_feat) {
        const MetaFeatures F{P->d_feat[0], P->d_feat[1], P->d_feat[2], P->d_feat_minus, P->d_seq_len, (u64)n_feat};
        hipLaunchKernelGGL(k_pileup_meta_geometry, dim3((uint32_t)((n_feat + kMetaGeometrySlice - 1) / kMetaGeometrySlice), (uint32_t)((B + kPileupThreads - 1) / kPileupThreads)),
                           dim3(kPileupThreads), 0, P->stream, P->n_seq, F, lay, (uint32_t)B, P->d_col + B, P->d_col + 2 * B);
        GFFX_KEEP_HIP(P, hipGetLastError());
    }
    GFFX_KEEP_HIP(P, hipStreamSynchronize(P->stream));  // (the caller's arrays are free again)
    P->meta = true, P->meta_matrix = keep_matrix != 0;
    P->n_feat = n_feat, P->meta_cols = (uint32_t)B, P->meta_layout = lay;
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_meta_copy(gffx_hip_pileup *P, uint64_t *col_bases, uint64_t *col_len, uint64_t *col_features, uint64_t *matrix) {
    int rc = enter_handle(P, "gffx_hip_pileup_meta_copy");
    if (rc) return rc;
    if (!P->meta) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_copy: the pileup has no features (gffx_hip_pileup_meta_set)");
    if (matrix && !P->meta_matrix) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_copy: the matrix was not kept");
    GFFX_KEEP_TRY(P, pileup_drain(P));
    const size_t B = P->meta_cols;
    if (col_bases) GFFX_KEEP_HIP(P, hipMemcpy(col_bases, P->d_col, B * 8, hipMemcpyDeviceToHost));
    if (col_len) GFFX_KEEP_HIP(P, hipMemcpy(col_len, P->d_col + B, B * 8, hipMemcpyDeviceToHost));
    if (col_features) GFFX_KEEP_HIP(P, hipMemcpy(col_features, P->d_col + 2 * B, B * 8, hipMemcpyDeviceToHost));
    if (matrix && P->n_feat) GFFX_KEEP_HIP(P, hipMemcpy(matrix, P->d_matrix, P->n_feat * B * 8, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

// (const in the interface: like _stage_ms it waits for the folds in flight)
extern "C" int gffx_hip_pileup_meta_ms(const gffx_hip_pileup *Pc, double *ms) {
    if (!Pc) return fail(GFFX_E_INVALID, "gffx_hip_pileup_meta_ms: pileup is NULL");
    const int rc = gffx_hip_pileup_stage_ms(Pc, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (ms) *ms = Pc->meta_ms;
    return GFFX_OK;
}

// (const in the interface; the times of folds that are still in flight are fetched here, which waits for them)
extern "C" int gffx_hip_pileup_stage_ms(const gffx_hip_pileup *Pc, double *keys, double *sorts, double *scan, double *segments) {
    if (!Pc) return fail(GFFX_E_INVALID, "gffx_hip_pileup_stage_ms: pileup is NULL");
    gffx_hip_pileup *P = const_cast<gffx_hip_pileup *>(Pc);
    if (P->status == GFFX_OK && (P->pending[0] || P->pending[1])) {
        GFFX_KEEP_HIP(P, hipSetDevice(P->device));
        GFFX_KEEP_TRY(P, pileup_drain(P));
    }
    if (keys) *keys = P->stage_ms[0];
    if (sorts) *sorts = P->stage_ms[1];
    if (scan) *scan = P->stage_ms[2];
    if (segments) *segments = P->stage_ms[3];
    return GFFX_OK;
}

extern "C" int gffx_hip_pileup_stats(const gffx_hip_pileup *P, double *kernel_ms, uint64_t *rows, uint64_t *folds) {
    if (!P) return fail(GFFX_E_INVALID, "gffx_hip_pileup_stats: pileup is NULL");
    double s[4] = {0, 0, 0, 0};
    const int rc = gffx_hip_pileup_stage_ms(P, &s[0], &s[1], &s[2], &s[3]);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = s[0] + s[1] + s[2] + s[3];
    if (rows) *rows = P->rows_added;
    if (folds) *folds = P->folds;
    return GFFX_OK;
}
