// profile.hip -- `gffx coverage --thresholds / --bedgraph`: the per-base depth of the source rows as a canonical list of
// points per seqid (profile_core.hpp has the quantity, the point rule and the threshold rule).
// The profile is a function of the MULTISET of rows: depth(x) counts rows, and the canonical points are a normal form of the
// function depth().  So any grouping of the rows into folds, any order, and profiles merged with one another give the same
// points bit for bit.  One fold of at most kProfileFold new rows, on the profile's own stream:
//   k_profile_events     rows {seqid, s, e} -> two W = 3 records {seqid, s, +1}, {seqid, e, -1}; a row with seqid >= n_seq or
//                        s >= e sets the error word (the union builder's bits and precedence: coverage.hip)
//   k_profile_deltas     the points carried so far (and the points of _add_points, which it also checks for canonical form):
//                        {seqid, pos_i, d_i} -> {seqid, pos_i, d_i - d_{i-1}}.  The host reads the error word right here.
//   DeviceSort<3>        all records by (seqid, position) (radix_sort.hpp); the order among equal keys is free: deltas are summed
//   k_profile_tile_sums  per tile of kProfileScanTile records: the sum of the deltas, and the sum up to the tile's last TAIL (the
//                        last record of a run of equal keys), if it has one
//   k_profile_carry      one block: exclusive sum over the tiles, and per tile the depth behind the last tail before it
//                        (reduce-then-scan: nothing spins anywhere).  ONE SCAN OVER ALL RECORDS NEEDS NO SEGMENTATION: a seqid's
//                        deltas add up to zero (every row adds +1 and -1, every carried seqid ends at depth 0), so the running sum
//                        is 0 at every seqid border by itself.  tools/profile_check.cpp asserts that invariant.
//                        32-BIT SUMS ARE EXACT: deltas are two's complement words, a true depth lies in 0 .. 2^32 - 1 (at most
//                        2^32 - 1 rows per profile), and the sum at a tail equals the true depth modulo 2^32, hence the depth.
//                        Sums inside a run of equal keys may wrap; they are never looked at.
//   k_profile_count      per tile the tails whose depth differs from the depth behind the previous tail: the points
//   k_profile_carry_count  exclusive sum of the counts, and their total
//   k_profile_emit       point k = {seqid, position, depth} of the k-th such tail, in the sorted order: the new carried points
// _finish adds p_off (k_profile_offsets: one search per seqid).  gffx_hip_profile_union_at_least(T): k_profile_span_count /
// k_profile_carry_count / k_profile_spans apply the threshold rule to every point and write the spans "depth >= T" as
// {seqid, start, end} records into a fresh union object's rec_a (union_private.hpp) -- they never leave HBM --, and
// gffx_hip_union_finish, k_segments_covered, _copy_spans and _destroy serve that object like any other union.
// Roofline bound: the sort HBM (24 bytes per record and pass), the three passes over the sorted records HBM (12 bytes each).
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "gffx_device.hpp"
#include "profile_core.hpp"
#include "radix_sort.hpp"
#include "regions_store.hpp"
#include "union_private.hpp"

namespace gffx {

constexpr int kProfileThreads = 256;
constexpr uint32_t kProfileScanTile = 4 * kProfileThreads;  // 4 consecutive records per thread: three 16-byte loads
constexpr uint64_t kProfileFold = 4ull << 20;               // new rows per fold (the default batch of `gffx coverage`)
constexpr uint32_t kProfileErrRange = 2u;                   // err word: a row with seqid >= n_seq (the sort's own bit for it)
constexpr uint32_t kProfileErrInverted = 8u;                // ... with start >= end (4 is the sort's time-out)
constexpr uint32_t kProfileErrCanon = 16u;                  // ... points handed to _add_points that are not canonical

// records [i0, i0 + 4) of a three-word array (0 beyond n).  wide: `rec` is 16-byte aligned
__device__ __forceinline__ void profile_load(const uint32_t *rec, u64 n, u64 i0, int wide, uint32_t (&w)[12]) {
    if (i0 + 4 <= n && wide) {
        const uint4 *p = reinterpret_cast<const uint4 *>(rec + 3 * i0);  // (48 i0 bytes behind an aligned base)
        const uint4 a = p[0], b = p[1], c = p[2];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w, w[8] = c.x, w[9] = c.y,
        w[10] = c.z, w[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = (i0 + k / 3 < n) ? rec[3 * i0 + k] : 0u;
    }
}

// rows [i0, i0 + 4) -> their 8 event records at ev[2 i0 ..).  wide: `rows` is 16-byte aligned (a region-store slot that starts
// at a row that is no multiple of four is not); ev is a hipMalloc'd buffer
__global__ __launch_bounds__(kProfileThreads) void k_profile_events(const uint32_t *rows, u64 n, uint32_t n_seq, int wide, uint32_t *ev, uint32_t *err) {
    const u64 i0 = 4ull * ((u64)blockIdx.x * kProfileThreads + threadIdx.x);
    if (i0 >= n) return;
    uint32_t w[12];
    profile_load(rows, n, i0, wide, w);
    bool inverted = false, range = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) {
            inverted |= w[3 * j + 1] >= w[3 * j + 2];
            range |= w[3 * j] >= n_seq;
        }
    const uint32_t up = 1u, down = 0xFFFFFFFFu;  // +1 and -1
    if (i0 + 4 <= n) {  // (96 i0 bytes into a hipMalloc'd buffer: 16-byte aligned)
        uint4 *p = reinterpret_cast<uint4 *>(ev + 6 * i0);
        p[0] = make_uint4(w[0], w[1], up, w[0]);
        p[1] = make_uint4(w[2], down, w[3], w[4]);
        p[2] = make_uint4(up, w[3], w[5], down);
        p[3] = make_uint4(w[6], w[7], up, w[6]);
        p[4] = make_uint4(w[8], down, w[9], w[10]);
        p[5] = make_uint4(up, w[9], w[11], down);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) {
                uint32_t *o = ev + 6 * (i0 + j);
                o[0] = w[3 * j], o[1] = w[3 * j + 1], o[2] = up;
                o[3] = w[3 * j], o[4] = w[3 * j + 2], o[5] = down;
            }
    }
    if (range) atomicOr(err, kProfileErrRange);
    if (inverted) atomicOr(err, kProfileErrInverted);
}

// points [i0, i0 + 4) {seqid, pos, d} -> events {seqid, pos, d - d of the point before in the seqid (0 at its first)}.
// check: the points are a caller's (_add_points): anything not canonical sets the error word.  pts is a hipMalloc'd buffer;
// out_wide: `ev` is 16-byte aligned
__global__ __launch_bounds__(kProfileThreads) void k_profile_deltas(const uint32_t *pts, u64 n, uint32_t n_seq, int check, int out_wide, uint32_t *ev,
                                                                    uint32_t *err) {
    const u64 i0 = 4ull * ((u64)blockIdx.x * kProfileThreads + threadIdx.x);
    if (i0 >= n) return;
    uint32_t w[12], o[12];
    profile_load(pts, n, i0, 1, w);
    bool have_prev = i0 > 0, have_next = i0 + 4 < n;
    uint32_t seq_prev = 0, pos_prev = 0, d_prev = 0, seq_next = 0;
    if (have_prev) seq_prev = pts[3 * (i0 - 1)], pos_prev = pts[3 * (i0 - 1) + 1], d_prev = pts[3 * (i0 - 1) + 2];
    if (have_next) seq_next = pts[3 * (i0 + 4)];
    bool bad = false, range = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t seq = w[3 * j], pos = w[3 * j + 1], d = w[3 * j + 2];
        const bool valid = i0 + j < n;
        const bool first = !have_prev || seq_prev != seq;
        if (valid && check) {
            const bool more = j < 3 ? i0 + j + 1 < n : have_next;
            const uint32_t sn = j < 3 ? w[3 * (j < 3 ? j + 1 : 0)] : seq_next;  // (the inner test keeps the unrolled j == 3 inside w)
            bad |= !profile::canonical_step(first, pos_prev, d_prev, pos, d, !more || sn != seq);
            range |= seq >= n_seq;
        }
        o[3 * j] = seq, o[3 * j + 1] = pos, o[3 * j + 2] = d - (first ? 0u : d_prev);
        have_prev = true, seq_prev = seq, pos_prev = pos, d_prev = d;
    }
    if (i0 + 4 <= n && out_wide) {
        uint4 *p = reinterpret_cast<uint4 *>(ev + 3 * i0);
        p[0] = make_uint4(o[0], o[1], o[2], o[3]);
        p[1] = make_uint4(o[4], o[5], o[6], o[7]);
        p[2] = make_uint4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (i0 + k / 3 < n) ev[3 * i0 + k] = o[k];
    }
    if (range) atomicOr(err, kProfileErrRange);
    if (bad) atomicOr(err, kProfileErrCanon);
}

template <bool SUM>
__device__ __forceinline__ u64 profile_op(u64 a, u64 b) {
    return SUM ? a + b : (a > b ? a : b);
}

// exclusive scan of v over the block's 256 threads (0 is the identity of both operations); *total = the block's whole.  s_w: 4 words
template <bool SUM>
__device__ __forceinline__ u64 profile_block_scan(u64 v, u64 *s_w, u64 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc = profile_op<SUM>(inc, t);
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 base = 0, all = 0;
#pragma unroll
    for (int x = 0; x < kProfileThreads / 64; ++x) {
        if (x < wave) base = profile_op<SUM>(base, s_w[x]);
        all = profile_op<SUM>(all, s_w[x]);
    }
    const u64 prev = __shfl_up(inc, 1, 64);
    *total = all;
    return lane ? profile_op<SUM>(base, prev) : base;
}

struct ProfileTile {
    uint32_t seq[4], pos[4], depth[4];
    bool point[4];
};

// The tile's four records of this thread under the point rule.  base: the sum of the deltas before the tile; prev: the depth
// behind the last tail before the tile.  *tile_sum: the tile's deltas; *tile_tail: 0 if the tile has no tail, else
// (1 + its last tail's place in the tile) << 32 | the sum up to that tail (from `base` on).  s_sum, s_max: 4 words each
__device__ __forceinline__ void profile_tile(const uint32_t *rec, u64 n, uint32_t base, uint32_t prev, u64 *s_sum, u64 *s_max, ProfileTile &t,
                                             u64 *tile_sum, u64 *tile_tail) {
    const u64 i0 = (u64)blockIdx.x * kProfileScanTile + 4ull * threadIdx.x;
    uint32_t w[12];
    profile_load(rec, n, i0, 1, w);
    u64 key[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) t.seq[j] = w[3 * j], t.pos[j] = w[3 * j + 1], key[j] = profile::event_key(w[3 * j], w[3 * j + 1]);
    if (i0 + 4 < n) key[4] = profile::event_key(rec[3 * (i0 + 4)], rec[3 * (i0 + 4) + 1]);  // the record behind my fourth
    const uint32_t mine = w[2] + w[5] + w[8] + w[11];  // (0 beyond n)
    u64 total;
    uint32_t run = base + (uint32_t)profile_block_scan<true>(mine, s_sum, &total);
    uint32_t incl[4];
    bool tail[4];
    u64 last = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        run += w[3 * j + 2];
        incl[j] = run;
        tail[j] = i0 + j < n && profile::is_tail(key[j], i0 + j + 1 < n, key[j + 1]);
        if (tail[j]) last = ((u64)(4 * threadIdx.x + j + 1) << 32) | incl[j];
    }
    u64 all;
    const u64 before_me = profile_block_scan<false>(last, s_max, &all);
    uint32_t before = before_me ? (uint32_t)before_me : prev;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t.point[j] = i0 + j < n && profile::point_here(key[j], i0 + j + 1 < n, key[j + 1], before, incl[j], &t.depth[j]);
        if (tail[j]) before = incl[j];
    }
    *tile_sum = (uint32_t)total;
    *tile_tail = all;
}

__global__ __launch_bounds__(kProfileThreads) void k_profile_tile_sums(const uint32_t *rec, u64 n, u64 *tile_sum, u64 *tile_tail) {
    __shared__ u64 s_sum[kProfileThreads / 64], s_max[kProfileThreads / 64];
    ProfileTile t;
    u64 sum, tail;
    profile_tile(rec, n, 0u, 0u, s_sum, s_max, t, &sum, &tail);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum, tile_tail[blockIdx.x] = tail;
}

// one block: tile_sum[i] <- the sum of the deltas before tile i; tile_tail[i] <- the depth behind the last tail before tile i
__global__ __launch_bounds__(kProfileThreads) void k_profile_carry(u64 *tile_sum, u64 *tile_tail, uint32_t tiles) {
    __shared__ u64 s_sum[kProfileThreads / 64], s_max[kProfileThreads / 64];
    u64 run = 0, run_tail = 0;  // run_tail: (1 + tile) << 32 | depth behind the last tail so far
    for (uint32_t base = 0; base < tiles; base += kProfileThreads) {
        const uint32_t i = base + threadIdx.x;
        u64 all, all_tail;
        const u64 before = run + profile_block_scan<true>(i < tiles ? tile_sum[i] : 0ull, s_sum, &all);
        const u64 tl = i < tiles ? tile_tail[i] : 0ull;
        const u64 mine = tl ? ((u64)(i + 1) << 32) | (uint32_t)((uint32_t)before + (uint32_t)tl) : 0ull;
        const u64 ex = profile_block_scan<false>(mine, s_max, &all_tail);
        if (i < tiles) {
            tile_sum[i] = (uint32_t)before;
            tile_tail[i] = (uint32_t)(ex > run_tail ? ex : run_tail);
        }
        run += all;
        run_tail = all_tail > run_tail ? all_tail : run_tail;
        __syncthreads();  // (s_sum and s_max are rewritten by the next step)
    }
}

// one block: v[i] <- the exclusive sum of v (in place), *total <- the whole
__global__ __launch_bounds__(kProfileThreads) void k_profile_carry_count(u64 *v, uint32_t n, u64 *total) {
    __shared__ u64 s_w[kProfileThreads / 64];
    u64 run = 0;
    for (uint32_t base = 0; base < n; base += kProfileThreads) {
        const uint32_t i = base + threadIdx.x;
        u64 all;
        const u64 ex = profile_block_scan<true>(i < n ? v[i] : 0ull, s_w, &all);
        if (i < n) v[i] = run + ex;
        run += all;
        __syncthreads();  // (s_w is rewritten by the next step)
    }
    if (threadIdx.x == 0) *total = run;
}

__global__ __launch_bounds__(kProfileThreads) void k_profile_count(const uint32_t *rec, u64 n, const u64 *tile_sum, const u64 *tile_tail, u64 *tile_points) {
    __shared__ u64 s_sum[kProfileThreads / 64], s_max[kProfileThreads / 64], s_cnt[kProfileThreads / 64];
    ProfileTile t;
    u64 sum, tail;
    profile_tile(rec, n, (uint32_t)tile_sum[blockIdx.x], (uint32_t)tile_tail[blockIdx.x], s_sum, s_max, t, &sum, &tail);
    u64 total;
    (void)profile_block_scan<true>((u64)t.point[0] + t.point[1] + t.point[2] + t.point[3], s_cnt, &total);
    if (threadIdx.x == 0) tile_points[blockIdx.x] = total;
}

// out: point k = {seqid, position, depth} of the k-th point in the sorted order.  tile_base: the points before the tile; the
// host sized `out` for n records and there are at most n points
__global__ __launch_bounds__(kProfileThreads) void k_profile_emit(const uint32_t *rec, u64 n, const u64 *tile_sum, const u64 *tile_tail, const u64 *tile_base,
                                                                  uint32_t *out) {
    __shared__ u64 s_sum[kProfileThreads / 64], s_max[kProfileThreads / 64], s_cnt[kProfileThreads / 64];
    ProfileTile t;
    u64 sum, tail;
    profile_tile(rec, n, (uint32_t)tile_sum[blockIdx.x], (uint32_t)tile_tail[blockIdx.x], s_sum, s_max, t, &sum, &tail);
    u64 total;
    u64 k = tile_base[blockIdx.x] + profile_block_scan<true>((u64)t.point[0] + t.point[1] + t.point[2] + t.point[3], s_cnt, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (t.point[j] && k < n) {
            out[3 * k] = t.seq[j], out[3 * k + 1] = t.pos[j], out[3 * k + 2] = t.depth[j];
            ++k;
        }
}

// p_off[c] = the points with seqid < c, c = 0 .. n_seq: one search per seqid
__global__ __launch_bounds__(kProfileThreads) void k_profile_offsets(const uint32_t *pts, u64 n, uint32_t n_seq, u64 *p_off) {
    const u64 c = (u64)blockIdx.x * kProfileThreads + threadIdx.x;
    if (c > n_seq) return;
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (pts[3 * mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    p_off[c] = lo;
}

// the threshold rule at points [i0, i0 + 4): where a span "depth >= T" opens and where one closes
__device__ __forceinline__ void profile_span_flags(const uint32_t *pts, u64 n, uint32_t T, u64 i0, uint32_t (&w)[12], bool (&opens)[4], bool (&closes)[4]) {
    profile_load(pts, n, i0, 1, w);
    bool have_prev = i0 > 0 && i0 < n;
    uint32_t seq_prev = 0, d_prev = 0;
    if (have_prev) seq_prev = pts[3 * (i0 - 1)], d_prev = pts[3 * (i0 - 1) + 2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool valid = i0 + j < n, first = !have_prev || seq_prev != w[3 * j];
        opens[j] = valid && profile::span_opens(T, first, d_prev, w[3 * j + 2]);
        closes[j] = valid && profile::span_closes(T, first, d_prev, w[3 * j + 2]);
        have_prev = true, seq_prev = w[3 * j], d_prev = w[3 * j + 2];
    }
}

__global__ __launch_bounds__(kProfileThreads) void k_profile_span_count(const uint32_t *pts, u64 n, uint32_t T, u64 *tile_spans) {
    __shared__ u64 s_w[kProfileThreads / 64];
    uint32_t w[12];
    bool opens[4], closes[4];
    profile_span_flags(pts, n, T, (u64)blockIdx.x * kProfileScanTile + 4ull * threadIdx.x, w, opens, closes);
    u64 total;
    (void)profile_block_scan<true>((u64)opens[0] + opens[1] + opens[2] + opens[3], s_w, &total);
    if (threadIdx.x == 0) tile_spans[blockIdx.x] = total;
}

// span k = {seqid, the k-th opening point's position, the position of the close behind it}.  A canonical seqid ends at depth
// 0 < T, so every open has its close in the same seqid and a close has an open before it.  n_spans: the room in `out`
__global__ __launch_bounds__(kProfileThreads) void k_profile_spans(const uint32_t *pts, u64 n, uint32_t T, const u64 *tile_base, u64 n_spans, uint32_t *out) {
    __shared__ u64 s_w[kProfileThreads / 64];
    uint32_t w[12];
    bool opens[4], closes[4];
    profile_span_flags(pts, n, T, (u64)blockIdx.x * kProfileScanTile + 4ull * threadIdx.x, w, opens, closes);
    u64 total;
    u64 k = tile_base[blockIdx.x] + profile_block_scan<true>((u64)opens[0] + opens[1] + opens[2] + opens[3], s_w, &total);  // opens before mine
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (opens[j] && k < n_spans) out[3 * k] = w[3 * j], out[3 * k + 1] = w[3 * j + 1];
        if (opens[j]) ++k;
        if (closes[j] && k > 0 && k <= n_spans) out[3 * (k - 1) + 2] = w[3 * j + 1];
    }
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_profile : gffx::HandleStatus {
    static constexpr const char *kName = "profile", *kNoun = "profile";
    uint32_t n_seq = 0;
    hipStream_t stream = nullptr;
    // the fold in flight: 0 start, 1 events done, 2 sort starts (the host looked at the error word in between), 3 sort done,
    // 4 running depth done, 5 points done, 6 the error word and the point count are on the host
    hipEvent_t ev[7] = {};
    hipEvent_t read = nullptr;  // the fold's rows have been read
    bool pending = false;       // ev and h_ctl[8 ..] wait to be looked at
    uint32_t *buf[2] = {nullptr, nullptr};  // buf[cur][0 .. n_points) = the points so far as {seqid, pos, depth} records
    int cur = 0;
    uint64_t cap = 0, n_points = 0;
    uint32_t *work = nullptr;
    uint64_t cap_work = 0;
    u64 *tile[3] = {nullptr, nullptr, nullptr};  // per tile: delta sums, tails, point counts
    uint64_t cap_tiles = 0;
    uint32_t *d_rows = nullptr;  // _add_host: the fold's rows; _add_points: the points
    uint64_t cap_rows = 0;
    uint32_t *ctl = nullptr;    // device words {err, 3 x pad, count (64 bits), 2 x pad}
    uint32_t *h_ctl = nullptr;  // pinned, 2 x 8 words: the check behind the event kernels, the fold's end
    uint32_t *h_stage = nullptr;  // pinned
    uint64_t cap_stage = 0;
    u64 *d_poff = nullptr;  // n_seq + 1, after _finish
    bool finished = false;
    SortPlan plan{};
    double stage_ms[4] = {0, 0, 0, 0};  // events, sort, running depth, points
    uint64_t rows_added = 0, folds = 0;
    uint64_t budget = 0;  // rows in the profile (for merged points: their largest depth, which no more rows than that can reach)
};

namespace {

// the fold in flight is through: its stage times, what the sort said, and how many points there are now
int profile_collect(gffx_hip_profile *P) {
    if (!P->pending) return GFFX_OK;
    P->pending = false;
    GFFX_HIP_TRY(hipEventSynchronize(P->ev[6]));
    const int from[4] = {0, 2, 3, 4};
    for (int s = 0; s < 4; ++s) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, P->ev[from[s]], P->ev[from[s] + 1]) == hipSuccess) P->stage_ms[s] += ms;
    }
    const uint32_t *h = P->h_ctl + 8;
    if (h[0] & 4u) return fail(GFFX_E_HIP, "gffx_hip_profile: the device sort timed out waiting for an earlier tile");
    P->n_points = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
    return GFFX_OK;
}

// room for a fold of `need` records = the points so far + two per new row + the points added (the points stay in buf[cur])
int profile_reserve(gffx_hip_profile *P, uint64_t need) {
    if (need >= (1ull << 30))
        return fail(GFFX_E_INVALID, "gffx_hip_profile: %llu records (points so far + two per row of a fold + points added) exceed the device sort's limit of 2^30 - 1",
                    (unsigned long long)need);
    int rc;
    if (need > P->cap) {
        const uint64_t cap = std::min<uint64_t>(need + need / 4 + 1024, 1ull << 30);
        uint32_t *a = nullptr, *b = nullptr;
        if ((rc = dev_alloc_padded(&a, 3 * cap))) return rc;
        if ((rc = dev_alloc_padded(&b, 3 * cap))) {
            (void)hipFree(a);
            return rc;
        }
        hipError_t e = hipSuccess;
        if (P->n_points) e = hipMemcpyAsync(a, P->buf[P->cur], P->n_points * 12, hipMemcpyDeviceToDevice, P->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(P->stream);
        if (e != hipSuccess) {
            (void)hipFree(a);
            (void)hipFree(b);
            return fail(GFFX_E_HIP, "gffx_hip_profile: moving the points failed: %s", hipGetErrorString(e));
        }
        (void)hipFree(P->buf[0]);
        (void)hipFree(P->buf[1]);
        P->buf[0] = a, P->buf[1] = b, P->cur = 0, P->cap = cap;
    }
    const uint64_t want_work = DeviceSort::work_words(P->cap, P->plan.n_passes), want_tiles = (P->cap + kProfileScanTile - 1) / kProfileScanTile + 1;
    if (want_work > P->cap_work) {
        GFFX_HIP_TRY(hipStreamSynchronize(P->stream));
        if (P->work) GFFX_HIP_TRY(hipFree(P->work));
        P->work = nullptr, P->cap_work = 0;
        if ((rc = dev_alloc_padded(&P->work, want_work))) return rc;
        P->cap_work = want_work;
    }
    if (want_tiles > P->cap_tiles) {
        GFFX_HIP_TRY(hipStreamSynchronize(P->stream));
        for (u64 *&p : P->tile) {
            if (p) GFFX_HIP_TRY(hipFree(p));
            p = nullptr;
        }
        P->cap_tiles = 0;
        for (u64 *&p : P->tile)
            if ((rc = dev_alloc_padded(&p, want_tiles))) return rc;
        P->cap_tiles = want_tiles;
    }
    return GFFX_OK;
}

int profile_rows_room(gffx_hip_profile *P, uint64_t want) {  // d_rows for `want` three-word records
    if (want <= P->cap_rows) return GFFX_OK;
    GFFX_HIP_TRY(hipStreamSynchronize(P->stream));
    if (P->d_rows) GFFX_HIP_TRY(hipFree(P->d_rows));
    P->d_rows = nullptr, P->cap_rows = 0;
    const int rc = dev_alloc_padded(&P->d_rows, 3 * want);
    if (rc) return rc;
    P->cap_rows = want;
    return GFFX_OK;
}

uint32_t profile_grid(uint64_t n) { return (uint32_t)((n + kProfileScanTile - 1) / kProfileScanTile); }

// One fold: the m <= kProfileFold rows at `rows` and the q points at `extra` (device memory; their copy, if any, is enqueued
// on the stream or done) are merged with the points so far.  The earlier fold is collected and the room reserved by the
// caller.  Returns when the rows have been read and found well-formed; the sort, the scan and the compaction go on behind.
// Nothing of a refused fold enters the profile: the points so far are only read before the error word is looked at.
int profile_fold(gffx_hip_profile *P, const uint32_t *rows, uint64_t m, const uint32_t *extra, uint64_t q) {
    const u64 np = P->n_points, n = 2 * m + np + q;
    if (!m && !q) return GFFX_OK;
    uint32_t *X = P->buf[P->cur], *Y = P->buf[P->cur ^ 1];
    GFFX_HIP_TRY(hipMemsetAsync(P->ctl, 0, 32, P->stream));
    GFFX_HIP_TRY(hipEventRecord(P->ev[0], P->stream));
    if (m) {
        const int wide = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0;
        hipLaunchKernelGGL(k_profile_events, dim3(profile_grid(m)), dim3(kProfileThreads), 0, P->stream, rows, (u64)m, P->n_seq, wide, Y, P->ctl);
    }
    if (np) {
        uint32_t *to = Y + 6 * m;
        hipLaunchKernelGGL(k_profile_deltas, dim3(profile_grid(np)), dim3(kProfileThreads), 0, P->stream, (const uint32_t *)X, np, P->n_seq, 0,
                           (int)((reinterpret_cast<uintptr_t>(to) & 15u) == 0), to, P->ctl);
    }
    if (q) {
        uint32_t *to = Y + 6 * m + 3 * np;
        hipLaunchKernelGGL(k_profile_deltas, dim3(profile_grid(q)), dim3(kProfileThreads), 0, P->stream, extra, (u64)q, P->n_seq, 1,
                           (int)((reinterpret_cast<uintptr_t>(to) & 15u) == 0), to, P->ctl);
    }
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(P->ev[1], P->stream));
    uint32_t *h_now = P->h_ctl;
    GFFX_HIP_TRY(hipMemcpyAsync(h_now, P->ctl, 32, hipMemcpyDeviceToHost, P->stream));
    GFFX_HIP_TRY(hipEventRecord(P->read, P->stream));
    GFFX_HIP_TRY(hipEventSynchronize(P->read));
    if (h_now[0] & kProfileErrRange) return fail(GFFX_E_CHR_RANGE, "gffx_hip_profile: a row has chr >= %u", P->n_seq);
    if (h_now[0] & kProfileErrInverted) return fail(GFFX_E_INVALID, "gffx_hip_profile: a row has start >= end");
    if (h_now[0] & kProfileErrCanon)
        return fail(GFFX_E_INVALID, "gffx_hip_profile_add_points: the points are not canonical (positions ascending, depths changing, a first depth > 0, a last depth of 0)");
    uint32_t *sorted = nullptr;
    GFFX_HIP_TRY(hipEventRecord(P->ev[2], P->stream));
    const int rc = DeviceSort::run<3>(P->stream, Y, X, n, P->plan, P->n_seq, P->work, P->ctl, &sorted);
    if (rc) return rc;
    uint32_t *out = sorted == Y ? X : Y;
    GFFX_HIP_TRY(hipEventRecord(P->ev[3], P->stream));
    const uint32_t tiles = profile_grid(n);
    hipLaunchKernelGGL(k_profile_tile_sums, dim3(tiles), dim3(kProfileThreads), 0, P->stream, (const uint32_t *)sorted, n, P->tile[0], P->tile[1]);
    hipLaunchKernelGGL(k_profile_carry, dim3(1), dim3(kProfileThreads), 0, P->stream, P->tile[0], P->tile[1], tiles);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(P->ev[4], P->stream));
    hipLaunchKernelGGL(k_profile_count, dim3(tiles), dim3(kProfileThreads), 0, P->stream, (const uint32_t *)sorted, n, (const u64 *)P->tile[0],
                       (const u64 *)P->tile[1], P->tile[2]);
    hipLaunchKernelGGL(k_profile_carry_count, dim3(1), dim3(kProfileThreads), 0, P->stream, P->tile[2], tiles, reinterpret_cast<u64 *>(P->ctl + 4));
    hipLaunchKernelGGL(k_profile_emit, dim3(tiles), dim3(kProfileThreads), 0, P->stream, (const uint32_t *)sorted, n, (const u64 *)P->tile[0],
                       (const u64 *)P->tile[1], (const u64 *)P->tile[2], out);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(P->ev[5], P->stream));
    GFFX_HIP_TRY(hipMemcpyAsync(P->h_ctl + 8, P->ctl, 32, hipMemcpyDeviceToHost, P->stream));
    GFFX_HIP_TRY(hipEventRecord(P->ev[6], P->stream));
    P->pending = true;
    P->cur = out == P->buf[0] ? 0 : 1;
    P->finished = false;
    P->rows_added += m;
    P->folds++;
    return GFFX_OK;
}

int profile_budget(gffx_hip_profile *P, uint64_t more, const char *who) {
    if (P->budget + more > 0xFFFFFFFFull) return fail(GFFX_E_INVALID, "%s: a profile holds at most 2^32 - 1 rows (depths are 32 bits)", who);
    return GFFX_OK;
}

}  // namespace

extern "C" uint64_t gffx_hip_profile_fold_rows(void) { return kProfileFold; }
extern "C" uint32_t gffx_hip_profile_scan_tile(void) { return kProfileScanTile; }

extern "C" void gffx_hip_profile_destroy(gffx_hip_profile *P) {
    if (!P) return;
    (void)hipSetDevice(P->device);
    if (P->stream) (void)hipStreamSynchronize(P->stream);
    for (void *p : {(void *)P->buf[0], (void *)P->buf[1], (void *)P->work, (void *)P->tile[0], (void *)P->tile[1], (void *)P->tile[2], (void *)P->d_rows,
                    (void *)P->ctl, (void *)P->d_poff})
        if (p) (void)hipFree(p);
    if (P->h_stage) (void)hipHostFree(P->h_stage);
    if (P->h_ctl) (void)hipHostFree(P->h_ctl);
    for (hipEvent_t e : P->ev)
        if (e) (void)hipEventDestroy(e);
    if (P->read) (void)hipEventDestroy(P->read);
    if (P->stream) (void)hipStreamDestroy(P->stream);
    delete P;
}

extern "C" int gffx_hip_profile_create(int device, uint32_t n_seq, gffx_hip_profile **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_profile_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    if (ndev <= 0) return fail(GFFX_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFFX_E_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_profile, void (*)(gffx_hip_profile *)> P(new gffx_hip_profile, gffx_hip_profile_destroy);
    P->device = device;
    P->n_seq = n_seq;
    // by (seqid, position): the four bytes of the position, then as many bytes of the seqid as n_seq needs (the union's rule)
    int seq_bytes = 1;
    while (seq_bytes < 4 && (n_seq > (1u << (8 * seq_bytes)))) seq_bytes++;
    for (int b = 0; b < 4; ++b) P->plan.word[P->plan.n_passes] = 1, P->plan.shift[P->plan.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < seq_bytes; ++b) P->plan.word[P->plan.n_passes] = 0, P->plan.shift[P->plan.n_passes++] = (uint8_t)(8 * b);
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : P->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    GFFX_HIP_TRY(hipEventCreateWithFlags(&P->read, hipEventDisableTiming));
    GFFX_HIP_TRY(hipHostMalloc((void **)&P->h_ctl, 2 * 32, hipHostMallocDefault));
    std::memset(P->h_ctl, 0, 2 * 32);
    int rc;
    if ((rc = dev_alloc_padded(&P->ctl, 8)) || (rc = dev_alloc_padded(&P->d_poff, (uint64_t)n_seq + 1))) return rc;
    *out = P.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_add_host(gffx_hip_profile *P, const uint32_t *rows, uint64_t n_rows) {
    int rc = enter_handle(P, "gffx_hip_profile_add_host");
    if (rc) return rc;
    if (n_rows && !rows) return fail(GFFX_E_INVALID, "gffx_hip_profile_add_host: rows is NULL");
    if ((rc = profile_budget(P, n_rows, "gffx_hip_profile_add_host"))) return rc;
    const uint64_t want = std::min<uint64_t>(n_rows, kProfileFold);
    if (want > P->cap_stage) {
        if (P->h_stage) (void)hipHostFree(P->h_stage);
        P->h_stage = nullptr, P->cap_stage = 0;
        hipError_t e = hipHostMalloc((void **)&P->h_stage, want * 12, hipHostMallocDefault);
        if (e != hipSuccess)
            return keep_failure(P, fail(GFFX_E_OOM, "hipHostMalloc of a %llu-row staging buffer failed: %s", (unsigned long long)want, hipGetErrorString(e)));
        P->cap_stage = want;
    }
    GFFX_KEEP_TRY(P, profile_rows_room(P, want));
    for (uint64_t at = 0; at < n_rows; at += kProfileFold) {
        const uint64_t m = std::min<uint64_t>(kProfileFold, n_rows - at);
        GFFX_KEEP_TRY(P, profile_collect(P));
        GFFX_KEEP_TRY(P, profile_reserve(P, P->n_points + 2 * m));
        std::memcpy(P->h_stage, rows + 3 * at, m * 12);  // (a fold returns after its rows were read: the buffer is free again)
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->d_rows, P->h_stage, m * 12, hipMemcpyHostToDevice, P->stream));
        GFFX_KEEP_TRY(P, profile_fold(P, P->d_rows, m, nullptr, 0));
        P->budget += m;
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_add_store(gffx_hip_profile *P, const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows) {
    int rc = enter_handle(P, "gffx_hip_profile_add_store");
    if (rc) return rc;
    const uint32_t *src = nullptr;
    if ((rc = store_slot_rows(R, k, first, n_rows, P->device, "gffx_hip_profile_add_store", "profile", &src))) return rc;
    if ((rc = profile_budget(P, n_rows, "gffx_hip_profile_add_store"))) return rc;
    if (R->pending[k]) GFFX_KEEP_HIP(P, hipStreamWaitEvent(P->stream, R->copied[k], 0));
    for (uint64_t at = 0; at < n_rows; at += kProfileFold) {
        const uint64_t m = std::min<uint64_t>(kProfileFold, n_rows - at);
        GFFX_KEEP_TRY(P, profile_collect(P));
        GFFX_KEEP_TRY(P, profile_reserve(P, P->n_points + 2 * m));
        GFFX_KEEP_TRY(P, profile_fold(P, src + 3 * at, m, nullptr, 0));  // (the slot is read in place: no copy)
        P->budget += m;
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_add_points(gffx_hip_profile *P, const uint64_t *p_off, const uint32_t *pos, const uint32_t *depth) {
    int rc = enter_handle(P, "gffx_hip_profile_add_points");
    if (rc) return rc;
    if (!p_off) return fail(GFFX_E_INVALID, "gffx_hip_profile_add_points: p_off is NULL");
    const uint64_t n = p_off[P->n_seq];
    if (n && (!pos || !depth)) return fail(GFFX_E_INVALID, "gffx_hip_profile_add_points: NULL point array");
    // (p_off is looked at here: the arrays cannot be read without it; everything else is checked on the device)
    if (p_off[0] != 0) return keep_failure(P, fail(GFFX_E_INVALID, "gffx_hip_profile_add_points: p_off does not start at 0"));
    for (uint32_t c = 0; c < P->n_seq; ++c)
        if (p_off[c + 1] < p_off[c] || p_off[c + 1] > n) return keep_failure(P, fail(GFFX_E_INVALID, "gffx_hip_profile_add_points: p_off is not ascending"));
    if (!n) return GFFX_OK;
    std::vector<uint32_t> rec(3 * n);
    uint32_t deepest = 0;
    for (uint32_t c = 0; c < P->n_seq; ++c)
        for (uint64_t i = p_off[c]; i < p_off[c + 1]; ++i) {
            rec[3 * i] = c, rec[3 * i + 1] = pos[i], rec[3 * i + 2] = depth[i];
            deepest = std::max(deepest, depth[i]);
        }
    if ((rc = profile_budget(P, deepest, "gffx_hip_profile_add_points"))) return rc;
    GFFX_KEEP_TRY(P, profile_collect(P));
    GFFX_KEEP_TRY(P, profile_reserve(P, P->n_points + n));
    GFFX_KEEP_TRY(P, profile_rows_room(P, n));
    GFFX_KEEP_HIP(P, hipMemcpy(P->d_rows, rec.data(), n * 12, hipMemcpyHostToDevice));  // (no fold reads d_rows any more: each returned behind its `read`)
    GFFX_KEEP_TRY(P, profile_fold(P, nullptr, 0, P->d_rows, n));
    P->budget += deepest;
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_finish(gffx_hip_profile *P) {
    int rc = enter_handle(P, "gffx_hip_profile_finish");
    if (rc) return rc;
    GFFX_KEEP_TRY(P, profile_collect(P));
    if (P->finished) return GFFX_OK;
    hipLaunchKernelGGL(k_profile_offsets, dim3(P->n_seq / kProfileThreads + 1), dim3(kProfileThreads), 0, P->stream, (const uint32_t *)P->buf[P->cur],
                       (u64)P->n_points, P->n_seq, P->d_poff);
    GFFX_KEEP_HIP(P, hipGetLastError());
    GFFX_KEEP_HIP(P, hipStreamSynchronize(P->stream));
    P->finished = true;
    return GFFX_OK;
}

// (const in the interface; a fold that is still in flight is waited for here)
extern "C" uint64_t gffx_hip_profile_n_points(const gffx_hip_profile *Pc) {
    if (!Pc) return 0;
    gffx_hip_profile *P = const_cast<gffx_hip_profile *>(Pc);
    if (P->status == GFFX_OK && P->pending) {
        if (hipSetDevice(P->device) != hipSuccess) return 0;
        const int rc = profile_collect(P);
        if (rc) return (void)keep_failure(P, rc), 0;
    }
    return P->n_points;
}

extern "C" int gffx_hip_profile_copy_points(gffx_hip_profile *P, uint64_t *p_off, uint32_t *pos, uint32_t *depth) {
    int rc = enter_handle(P, "gffx_hip_profile_copy_points");
    if (rc) return rc;
    if (!P->finished || P->pending) return fail(GFFX_E_STATE, "gffx_hip_profile_copy_points: call gffx_hip_profile_finish first");
    if (p_off) GFFX_KEEP_HIP(P, hipMemcpy(p_off, P->d_poff, ((uint64_t)P->n_seq + 1) * 8, hipMemcpyDeviceToHost));
    if ((pos || depth) && P->n_points) {
        std::vector<uint32_t> rec(3 * P->n_points);
        GFFX_KEEP_HIP(P, hipMemcpy(rec.data(), P->buf[P->cur], P->n_points * 12, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < P->n_points; ++i) {
            if (pos) pos[i] = rec[3 * i + 1];
            if (depth) depth[i] = rec[3 * i + 2];
        }
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_union_at_least(gffx_hip_profile *P, uint32_t T, gffx_hip_union **out) {
    int rc = enter_handle(P, "gffx_hip_profile_union_at_least");
    if (rc) return rc;
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_profile_union_at_least: out is NULL");
    *out = nullptr;
    if (T == 0) return fail(GFFX_E_INVALID, "gffx_hip_profile_union_at_least: T is 0 (every base has depth >= 0)");
    if (!P->finished || P->pending) return fail(GFFX_E_STATE, "gffx_hip_profile_union_at_least: call gffx_hip_profile_finish first");
    gffx_hip_union *raw = nullptr;
    GFFX_KEEP_TRY(P, gffx_hip_union_create(P->device, P->n_seq, &raw));
    std::unique_ptr<gffx_hip_union, void (*)(gffx_hip_union *)> U(raw, gffx_hip_union_destroy);
    const u64 np = P->n_points;
    if (np) {
        const uint32_t tiles = profile_grid(np);  // (<= cap_tiles: the points came out of a fold of at least np records)
        const uint32_t *pts = P->buf[P->cur];
        hipLaunchKernelGGL(k_profile_span_count, dim3(tiles), dim3(kProfileThreads), 0, P->stream, pts, np, T, P->tile[2]);
        hipLaunchKernelGGL(k_profile_carry_count, dim3(1), dim3(kProfileThreads), 0, P->stream, P->tile[2], tiles, reinterpret_cast<u64 *>(P->ctl + 4));
        GFFX_KEEP_HIP(P, hipGetLastError());
        GFFX_KEEP_HIP(P, hipMemcpyAsync(P->h_ctl, P->ctl, 32, hipMemcpyDeviceToHost, P->stream));
        GFFX_KEEP_HIP(P, hipStreamSynchronize(P->stream));
        const uint64_t spans = (uint64_t)P->h_ctl[4] | ((uint64_t)P->h_ctl[5] << 32);
        if (spans) {
            GFFX_KEEP_TRY(P, dev_alloc_padded(&U->rec_a, 3 * spans));
            GFFX_KEEP_TRY(P, dev_alloc_padded(&U->rec_b, 3 * spans));
            U->cap = std::max<uint64_t>(spans, 1);
            hipLaunchKernelGGL(k_profile_spans, dim3(tiles), dim3(kProfileThreads), 0, P->stream, pts, np, T, (const u64 *)P->tile[2], (u64)spans, U->rec_a);
            GFFX_KEEP_HIP(P, hipGetLastError());
            GFFX_KEEP_HIP(P, hipStreamSynchronize(P->stream));  // (the union reads rec_a on its own stream)
            U->n_spans = spans;
        }
    }
    U->rows_added = P->rows_added;
    GFFX_KEEP_TRY(P, gffx_hip_union_finish(U.get()));
    *out = U.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_reset(gffx_hip_profile *P) {
    int rc = enter_handle(P, "gffx_hip_profile_reset");
    if (rc) return rc;
    GFFX_KEEP_TRY(P, profile_collect(P));
    P->n_points = 0, P->budget = 0, P->finished = false;
    return GFFX_OK;
}

// (const in the interface; the times of a fold that is still in flight are fetched here, which waits for it)
extern "C" int gffx_hip_profile_stage_ms(const gffx_hip_profile *Pc, double *events, double *sort, double *scan, double *points) {
    if (!Pc) return fail(GFFX_E_INVALID, "gffx_hip_profile_stage_ms: profile is NULL");
    gffx_hip_profile *P = const_cast<gffx_hip_profile *>(Pc);
    if (P->status == GFFX_OK && P->pending) {
        GFFX_KEEP_HIP(P, hipSetDevice(P->device));
        GFFX_KEEP_TRY(P, profile_collect(P));
    }
    if (events) *events = P->stage_ms[0];
    if (sort) *sort = P->stage_ms[1];
    if (scan) *scan = P->stage_ms[2];
    if (points) *points = P->stage_ms[3];
    return GFFX_OK;
}

extern "C" int gffx_hip_profile_stats(const gffx_hip_profile *P, double *kernel_ms, uint64_t *rows, uint64_t *folds) {
    if (!P) return fail(GFFX_E_INVALID, "gffx_hip_profile_stats: profile is NULL");
    double s[4] = {0, 0, 0, 0};
    const int rc = gffx_hip_profile_stage_ms(P, &s[0], &s[1], &s[2], &s[3]);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = s[0] + s[1] + s[2] + s[3];
    if (rows) *rows = P->rows_added;
    if (folds) *folds = P->folds;
    return GFFX_OK;
}
