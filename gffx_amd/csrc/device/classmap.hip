// classmap.hip -- `gffx annotate`: per region the bases of every feature class (classmap_core.hpp has the
// definition, the point rule and the region rule).  The class map is a function of the MULTISET of (layer, seqid, start, end)
// rows: the per-layer unions are a normal form of the layers and the canonical points a normal form of class(), so any
// grouping of the rows into calls, any order and duplicates give the same points bit for bit.
//   union builder          one union per (layer, seqid): rows go in under the pseudo-seqid seqid * T + layer (coverage.hip)
// _finish, on the object's own stream:
//   k_classmap_toggles     the union's span records {pseudo, s, e}, read where they lie -> two W = 3 records {seqid, s, 1 << k},
//                          {seqid, e, 1 << k}
//   DeviceSort<3>          by (seqid, position) (radix_sort.hpp); the order among equal keys is free: toggles are XORed
//   k_classmap_tile_xor    per tile of kClassScanTile records: the XOR of the tile, and the XOR up to the tile's last TAIL
//   k_classmap_carry       one block: exclusive XOR over the tiles, and per tile the mask behind the last tail before it.  No
//                          segmentation: a seqid's toggles XOR to zero
//   k_classmap_count       per tile the tails whose class differs from the class behind the previous tail: the points
//   k_classmap_carry_sum   exclusive sum of the counts, and their total (the host sizes the point arrays by it)
//   k_classmap_emit        point i = (seqid, position, class) of the i-th such tail, in the sorted order, no atomics
//   k_classmap_offsets     p_off[c] = the points with seqid < c: one search per seqid
//   k_classmap_tile_bases / _carry_bases / k_classmap_bases   cb[i * T + k]: per class a tile scan of 64-bit lengths
// a run:
//   k_classmap_regions     one thread per region: two searches bounded by [p_off[c], p_off[c + 1]), 2 T reads of cb, T + 1
//                          counts and a class byte.  The region's numbers are only compared, never used as an index.
// Roofline bound: the build is the sort's HBM traffic; the regions kernel is latency: ~2 log2(points per seqid) dependent loads.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "classmap_core.hpp"
#include "classmap_private.hpp"
#include "gffx_device.hpp"
#include "radix_sort.hpp"
#include "regions_store.hpp"
#include "union_private.hpp"

namespace gffx {

constexpr uint32_t kClassScanTile = 4 * kClassThreads;  // 4 consecutive records per thread

enum { kOpSum = 0, kOpMax = 1, kOpXor = 2 };
template <int OP>
__device__ __forceinline__ u64 class_op(u64 a, u64 b) {
    return OP == kOpSum ? a + b : OP == kOpXor ? (a ^ b) : (a > b ? a : b);
}

// exclusive scan of v over the block's 256 threads (0 is the identity of the three operations); *total = the block's whole.
// s_w: 4 words, free again behind the caller's next barrier
template <int OP>
__device__ __forceinline__ u64 class_block_scan(u64 v, u64 *s_w, u64 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc = class_op<OP>(inc, t);
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 base = 0, all = 0;
#pragma unroll
    for (int x = 0; x < kClassThreads / 64; ++x) {
        if (x < wave) base = class_op<OP>(base, s_w[x]);
        all = class_op<OP>(all, s_w[x]);
    }
    const u64 prev = __shfl_up(inc, 1, 64);
    *total = all;
    return lane ? class_op<OP>(base, prev) : base;
}

// span i {pseudo, s, e} -> events 2 i and 2 i + 1.  pseudo = seqid * T + layer (the union's rows were checked: pseudo < n_seq * T)
__global__ __launch_bounds__(kClassThreads) void k_classmap_toggles(const uint32_t *spans, u64 n, uint32_t T, uint32_t *ev) {
    const u64 i = (u64)blockIdx.x * kClassThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t pseudo = spans[3 * i], s = spans[3 * i + 1], e = spans[3 * i + 2];
    const uint32_t seq = pseudo / T, bit = 1u << (pseudo % T);
    uint32_t *o = ev + 6 * i;
    o[0] = seq, o[1] = s, o[2] = bit;
    o[3] = seq, o[4] = e, o[5] = bit;
}

struct ClassTile {
    uint32_t seq[4], pos[4], cls[4];
    bool point[4];
};

// The tile's four records of this thread under the point rule.  base: the XOR of the toggles before the tile; prev: the mask
// behind the last tail before the tile.  *tile_xor: the tile's toggles; *tile_tail: 0 if the tile has no tail, else
// (1 + its last tail's place in the tile) << 32 | the XOR up to that tail (from `base` on).  s_a, s_b: 4 words each
__device__ __forceinline__ void class_tile(const uint32_t *rec, u64 n, uint32_t T, uint32_t base, uint32_t prev, u64 *s_a, u64 *s_b, ClassTile &t, u64 *tile_xor,
                                           u64 *tile_tail) {
    const u64 i0 = (u64)blockIdx.x * kClassScanTile + 4ull * threadIdx.x;
    uint32_t w[4];
    u64 key[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < n;
        t.seq[j] = in ? rec[3 * (i0 + j)] : 0u, t.pos[j] = in ? rec[3 * (i0 + j) + 1] : 0u, w[j] = in ? rec[3 * (i0 + j) + 2] : 0u;
        key[j] = classmap::event_key(t.seq[j], t.pos[j]);
    }
    if (i0 + 4 < n) key[4] = classmap::event_key(rec[3 * (i0 + 4)], rec[3 * (i0 + 4) + 1]);  // the record behind my fourth
    u64 total;
    uint32_t run = base ^ (uint32_t)class_block_scan<kOpXor>(w[0] ^ w[1] ^ w[2] ^ w[3], s_a, &total);
    uint32_t incl[4];
    bool tail[4];
    u64 last = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        run ^= w[j];
        incl[j] = run;
        tail[j] = i0 + j < n && classmap::is_tail(key[j], i0 + j + 1 < n, key[j + 1]);
        if (tail[j]) last = ((u64)(4 * threadIdx.x + j + 1) << 32) | incl[j];
    }
    u64 all;
    const u64 before_me = class_block_scan<kOpMax>(last, s_b, &all);
    uint32_t before = before_me ? (uint32_t)before_me : prev;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t.point[j] = i0 + j < n && classmap::point_here(key[j], i0 + j + 1 < n, key[j + 1], before, incl[j], T, &t.cls[j]);
        if (tail[j]) before = incl[j];
    }
    *tile_xor = (uint32_t)total;
    *tile_tail = all;
}

__global__ __launch_bounds__(kClassThreads) void k_classmap_tile_xor(const uint32_t *rec, u64 n, uint32_t T, u64 *tile_xor, u64 *tile_tail) {
    __shared__ u64 s_a[kClassThreads / 64], s_b[kClassThreads / 64];
    ClassTile t;
    u64 x, tail;
    class_tile(rec, n, T, 0u, 0u, s_a, s_b, t, &x, &tail);
    if (threadIdx.x == 0) tile_xor[blockIdx.x] = x, tile_tail[blockIdx.x] = tail;
}

// one block: tile_xor[i] <- the XOR of the toggles before tile i; tile_tail[i] <- the mask behind the last tail before tile i
__global__ __launch_bounds__(kClassThreads) void k_classmap_carry(u64 *tile_xor, u64 *tile_tail, uint32_t tiles) {
    __shared__ u64 s_a[kClassThreads / 64], s_b[kClassThreads / 64];
    u64 run = 0, run_tail = 0;  // run_tail: (1 + tile) << 32 | mask behind the last tail so far
    for (uint32_t base = 0; base < tiles; base += kClassThreads) {
        const uint32_t i = base + threadIdx.x;
        u64 all, all_tail;
        const u64 before = run ^ class_block_scan<kOpXor>(i < tiles ? tile_xor[i] : 0ull, s_a, &all);
        const u64 tl = i < tiles ? tile_tail[i] : 0ull;
        const u64 mine = tl ? ((u64)(i + 1) << 32) | (uint32_t)((uint32_t)before ^ (uint32_t)tl) : 0ull;
        const u64 ex = class_block_scan<kOpMax>(mine, s_b, &all_tail);
        if (i < tiles) {
            tile_xor[i] = (uint32_t)before;
            tile_tail[i] = (uint32_t)(ex > run_tail ? ex : run_tail);
        }
        run ^= all;
        run_tail = all_tail > run_tail ? all_tail : run_tail;
        __syncthreads();  // (s_a and s_b are rewritten by the next step)
    }
}

// one block: v[i] <- the exclusive sum of v (in place), *total <- the whole
__global__ __launch_bounds__(kClassThreads) void k_classmap_carry_sum(u64 *v, uint32_t n, u64 *total) {
    __shared__ u64 s_w[kClassThreads / 64];
    u64 run = 0;
    for (uint32_t base = 0; base < n; base += kClassThreads) {
        const uint32_t i = base + threadIdx.x;
        u64 all;
        const u64 ex = class_block_scan<kOpSum>(i < n ? v[i] : 0ull, s_w, &all);
        if (i < n) v[i] = run + ex;
        run += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = run;
}

__global__ __launch_bounds__(kClassThreads) void k_classmap_count(const uint32_t *rec, u64 n, uint32_t T, const u64 *tile_xor, const u64 *tile_tail,
                                                                  u64 *tile_points) {
    __shared__ u64 s_a[kClassThreads / 64], s_b[kClassThreads / 64], s_c[kClassThreads / 64];
    ClassTile t;
    u64 x, tail;
    class_tile(rec, n, T, (uint32_t)tile_xor[blockIdx.x], (uint32_t)tile_tail[blockIdx.x], s_a, s_b, t, &x, &tail);
    u64 total;
    (void)class_block_scan<kOpSum>((u64)t.point[0] + t.point[1] + t.point[2] + t.point[3], s_c, &total);
    if (threadIdx.x == 0) tile_points[blockIdx.x] = total;
}

// point i of the sorted order -> p_seq[i], p_pos[i], p_cls[i].  tile_base: the points before the tile; n_points: the arrays' room
__global__ __launch_bounds__(kClassThreads) void k_classmap_emit(const uint32_t *rec, u64 n, uint32_t T, const u64 *tile_xor, const u64 *tile_tail,
                                                                 const u64 *tile_base, u64 n_points, uint32_t *p_seq, uint32_t *p_pos, uint8_t *p_cls) {
    __shared__ u64 s_a[kClassThreads / 64], s_b[kClassThreads / 64], s_c[kClassThreads / 64];
    ClassTile t;
    u64 x, tail;
    class_tile(rec, n, T, (uint32_t)tile_xor[blockIdx.x], (uint32_t)tile_tail[blockIdx.x], s_a, s_b, t, &x, &tail);
    u64 total;
    u64 i = tile_base[blockIdx.x] + class_block_scan<kOpSum>((u64)t.point[0] + t.point[1] + t.point[2] + t.point[3], s_c, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (t.point[j] && i < n_points) {
            p_seq[i] = t.seq[j], p_pos[i] = t.pos[j], p_cls[i] = (uint8_t)t.cls[j];
            ++i;
        }
}

// p_off[c] = the points with seqid < c, c = 0 .. n_seq: one search per seqid
__global__ __launch_bounds__(kClassThreads) void k_classmap_offsets(const uint32_t *p_seq, u64 n, uint32_t n_seq, u64 *p_off) {
    const u64 c = (u64)blockIdx.x * kClassThreads + threadIdx.x;
    if (c > n_seq) return;
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (p_seq[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    p_off[c] = lo;
}

// this thread's four points of the tile: class and length (class T and 0 beyond n)
__device__ __forceinline__ void class_lens(const uint32_t *p_seq, const uint32_t *p_pos, const uint8_t *p_cls, u64 n, uint32_t T, uint32_t (&cls)[4],
                                           uint32_t (&len)[4]) {
    const u64 i0 = (u64)blockIdx.x * kClassScanTile + 4ull * threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 i = i0 + j;
        cls[j] = T, len[j] = 0u;
        if (i < n) {
            const bool next = i + 1 < n && p_seq[i + 1] == p_seq[i];
            cls[j] = p_cls[i];
            len[j] = classmap::point_len(p_pos[i], next, next ? p_pos[i + 1] : 0u);
        }
    }
}

// tile_tot[tile * T + k] = the bases of class k on the tile's points
__global__ __launch_bounds__(kClassThreads) void k_classmap_tile_bases(const uint32_t *p_seq, const uint32_t *p_pos, const uint8_t *p_cls, u64 n, uint32_t T,
                                                                       u64 *tile_tot) {
    __shared__ u64 s_w[kClassThreads / 64];
    uint32_t cls[4], len[4];
    class_lens(p_seq, p_pos, p_cls, n, T, cls, len);
    for (uint32_t k = 0; k < T; ++k) {
        u64 v = 0, total;
#pragma unroll
        for (int j = 0; j < 4; ++j) v += cls[j] == k ? len[j] : 0u;
        (void)class_block_scan<kOpSum>(v, s_w, &total);
        if (threadIdx.x == 0) tile_tot[(u64)blockIdx.x * T + k] = total;
        __syncthreads();  // (s_w is rewritten by the next class)
    }
}

// one block: per class k, tile_tot[tile * T + k] <- the exclusive sum over the tiles (in place)
__global__ __launch_bounds__(kClassThreads) void k_classmap_carry_bases(u64 *tile_tot, uint32_t tiles, uint32_t T) {
    __shared__ u64 s_w[kClassThreads / 64];
    for (uint32_t k = 0; k < T; ++k) {
        u64 run = 0;
        for (uint32_t base = 0; base < tiles; base += kClassThreads) {
            const uint32_t i = base + threadIdx.x;
            u64 all;
            const u64 ex = class_block_scan<kOpSum>(i < tiles ? tile_tot[(u64)i * T + k] : 0ull, s_w, &all);
            if (i < tiles) tile_tot[(u64)i * T + k] = run + ex;
            run += all;
            __syncthreads();
        }
    }
}

// cb[i * T + k] = the bases of class k on the points before point i
__global__ __launch_bounds__(kClassThreads) void k_classmap_bases(const uint32_t *p_seq, const uint32_t *p_pos, const uint8_t *p_cls, u64 n, uint32_t T,
                                                                  const u64 *tile_base, u64 *cb) {
    __shared__ u64 s_w[kClassThreads / 64];
    const u64 i0 = (u64)blockIdx.x * kClassScanTile + 4ull * threadIdx.x;
    uint32_t cls[4], len[4];
    class_lens(p_seq, p_pos, p_cls, n, T, cls, len);
    for (uint32_t k = 0; k < T; ++k) {
        u64 v = 0, total;
#pragma unroll
        for (int j = 0; j < 4; ++j) v += cls[j] == k ? len[j] : 0u;
        u64 run = tile_base[(u64)blockIdx.x * T + k] + class_block_scan<kOpSum>(v, s_w, &total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < n) cb[(i0 + j) * T + k] = run;
            run += cls[j] == k ? len[j] : 0u;
        }
        __syncthreads();
    }
}

// region i = rows[3 i ..] -> counts[i * (T + 1) ..], cls[i].  A region with chr >= n_seq sets the error word and writes nothing
__global__ __launch_bounds__(kClassThreads) void k_classmap_regions(ClassMapView M, const uint32_t *rows, u64 nq, uint32_t *counts, uint8_t *cls, uint32_t *err) {
    const u64 i = (u64)blockIdx.x * kClassThreads + threadIdx.x;
    if (i >= nq) return;
    const uint32_t c = rows[3 * i], qs = rows[3 * i + 1], qe = rows[3 * i + 2];
    if (c >= M.n_seq) {
        atomicOr(err, kClassErrRange);
        return;
    }
    // (the rule writes the T + 1 counts where they belong: no per-thread array)
    cls[i] = (uint8_t)classmap::region_bases(M.p_pos, M.p_cls, M.cb, M.T, M.p_off[c], M.p_off[c + 1], qs, qe, counts + i * (M.T + 1));
}

}  // namespace gffx

using namespace gffx;

namespace {

void classmap_drop_points(gffx_hip_classmap *H) {
    for (void *p : {(void *)H->p_seq, (void *)H->p_pos, (void *)H->p_cls, (void *)H->cb})
        if (p) (void)hipFree(p);
    H->p_seq = H->p_pos = nullptr, H->p_cls = nullptr, H->cb = nullptr;
    H->n_points = 0;
    H->finished = false;
    classmap_perm_drop(H);  // (permutation totals are totals over this map)
}

// the spans of the union -> points, p_off and cb.  The work buffers live for this call only
int classmap_build(gffx_hip_classmap *H) {
    const gffx_hip_union *U = H->U;
    const u64 ns = U->n_spans, n = 2 * ns;
    const uint32_t T = H->T;
    H->stage_ms[0] = U->kernel_ms;
    if (n >= (1ull << 30)) return fail(GFFX_E_INVALID, "gffx_hip_classmap_finish: %llu events exceed the device sort's limit of 2^30 - 1", n);
    if (!ns) {
        GFFX_HIP_TRY(hipMemsetAsync(H->p_off, 0, ((size_t)H->n_seq + 1) * 8, H->stream));
        GFFX_HIP_TRY(hipStreamSynchronize(H->stream));
        return GFFX_OK;
    }
    SortPlan plan{};
    // by (seqid, position): the four bytes of the position, then as many bytes of the seqid as n_seq needs
    int seq_bytes = 1;
    while (seq_bytes < 4 && (H->n_seq > (1u << (8 * seq_bytes)))) seq_bytes++;
    for (int b = 0; b < 4; ++b) plan.word[plan.n_passes] = 1, plan.shift[plan.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < seq_bytes; ++b) plan.word[plan.n_passes] = 0, plan.shift[plan.n_passes++] = (uint8_t)(8 * b);
    const uint32_t tiles = classmap_grid(n, kClassScanTile);
    uint32_t *buf[2] = {nullptr, nullptr}, *work = nullptr, *sorted = nullptr;
    u64 *tile[3] = {nullptr, nullptr, nullptr}, *tile_tot = nullptr;
    auto release = [&]() {
        for (void *p : {(void *)buf[0], (void *)buf[1], (void *)work, (void *)tile[0], (void *)tile[1], (void *)tile[2], (void *)tile_tot})
            if (p) (void)hipFree(p);
    };
    int rc = [&]() -> int {
        int r;
        if ((r = dev_alloc_padded(&buf[0], 3 * n)) || (r = dev_alloc_padded(&buf[1], 3 * n)) || (r = dev_alloc_padded(&work, DeviceSort::work_words(n, plan.n_passes))) ||
            (r = dev_alloc_padded(&tile[0], tiles)) || (r = dev_alloc_padded(&tile[1], tiles)) || (r = dev_alloc_padded(&tile[2], tiles)))
            return r;
        GFFX_HIP_TRY(hipMemsetAsync(H->ctl, 0, 32, H->stream));
        GFFX_HIP_TRY(hipEventRecord(H->ev[0], H->stream));
        // (the union's folds ended with a synchronisation of its stream: rec_a is at rest)
        hipLaunchKernelGGL(k_classmap_toggles, dim3(classmap_grid(ns, kClassThreads)), dim3(kClassThreads), 0, H->stream, (const uint32_t *)U->rec_a, ns, T, buf[0]);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(H->ev[1], H->stream));
        if ((r = DeviceSort::run<3>(H->stream, buf[0], buf[1], n, plan, H->n_seq, work, H->ctl, &sorted))) return r;
        GFFX_HIP_TRY(hipEventRecord(H->ev[2], H->stream));
        hipLaunchKernelGGL(k_classmap_tile_xor, dim3(tiles), dim3(kClassThreads), 0, H->stream, (const uint32_t *)sorted, n, T, tile[0], tile[1]);
        hipLaunchKernelGGL(k_classmap_carry, dim3(1), dim3(kClassThreads), 0, H->stream, tile[0], tile[1], tiles);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(H->ev[3], H->stream));
        hipLaunchKernelGGL(k_classmap_count, dim3(tiles), dim3(kClassThreads), 0, H->stream, (const uint32_t *)sorted, n, T, (const u64 *)tile[0], (const u64 *)tile[1],
                           tile[2]);
        hipLaunchKernelGGL(k_classmap_carry_sum, dim3(1), dim3(kClassThreads), 0, H->stream, tile[2], tiles, reinterpret_cast<u64 *>(H->ctl + 4));
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(H->ev[4], H->stream));
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        GFFX_HIP_TRY(hipMemcpyAsync(h, H->ctl, 32, hipMemcpyDeviceToHost, H->stream));
        GFFX_HIP_TRY(hipStreamSynchronize(H->stream));
        if (h[0] & 4u) return fail(GFFX_E_HIP, "gffx_hip_classmap_finish: the device sort timed out waiting for an earlier tile");
        if (h[0] & 2u) return fail(GFFX_E_HIP, "gffx_hip_classmap_finish: an event has seqid >= %u", H->n_seq);
        const u64 np = (u64)h[4] | ((u64)h[5] << 32);
        if (np > n) return fail(GFFX_E_HIP, "gffx_hip_classmap_finish: more points than events");
        const uint32_t ptiles = classmap_grid(np, kClassScanTile);
        if ((r = dev_alloc_padded(&H->p_seq, np)) || (r = dev_alloc_padded(&H->p_pos, np)) || (r = dev_alloc_padded(&H->p_cls, np)) ||
            (r = dev_alloc_padded(&H->cb, np * T)) || (r = dev_alloc_padded(&tile_tot, (u64)ptiles * T)))
            return r;
        GFFX_HIP_TRY(hipEventRecord(H->ev[5], H->stream));
        hipLaunchKernelGGL(k_classmap_emit, dim3(tiles), dim3(kClassThreads), 0, H->stream, (const uint32_t *)sorted, n, T, (const u64 *)tile[0], (const u64 *)tile[1],
                           (const u64 *)tile[2], np, H->p_seq, H->p_pos, H->p_cls);
        hipLaunchKernelGGL(k_classmap_offsets, dim3(H->n_seq / kClassThreads + 1), dim3(kClassThreads), 0, H->stream, (const uint32_t *)H->p_seq, np, H->n_seq,
                           H->p_off);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(H->ev[6], H->stream));
        if (np) {
            hipLaunchKernelGGL(k_classmap_tile_bases, dim3(ptiles), dim3(kClassThreads), 0, H->stream, (const uint32_t *)H->p_seq, (const uint32_t *)H->p_pos,
                               (const uint8_t *)H->p_cls, np, T, tile_tot);
            hipLaunchKernelGGL(k_classmap_carry_bases, dim3(1), dim3(kClassThreads), 0, H->stream, tile_tot, ptiles, T);
            hipLaunchKernelGGL(k_classmap_bases, dim3(ptiles), dim3(kClassThreads), 0, H->stream, (const uint32_t *)H->p_seq, (const uint32_t *)H->p_pos,
                               (const uint8_t *)H->p_cls, np, T, (const u64 *)tile_tot, H->cb);
            GFFX_HIP_TRY(hipGetLastError());
        }
        GFFX_HIP_TRY(hipEventRecord(H->ev[7], H->stream));
        GFFX_HIP_TRY(hipStreamSynchronize(H->stream));
        H->n_points = np;
        const int pairs[5][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {6, 7}};
        for (int s = 0; s < 5; ++s) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, H->ev[pairs[s][0]], H->ev[pairs[s][1]]) == hipSuccess) H->stage_ms[1 + s] = ms;
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, H->ev[5], H->ev[6]) == hipSuccess) H->stage_ms[4] += ms;
        return GFFX_OK;
    }();
    if (rc) (void)hipStreamSynchronize(H->stream);  // (nothing may still read what is freed next)
    release();
    return rc;
}

int classmap_run(gffx_hip_classmap *H, const uint32_t *rows, uint64_t nq, const char *who) {
    H->ran = H->waited = false;
    H->nq = nq;
    H->kernel_ms = 0;
    if (!nq) {
        H->ran = true;
        return GFFX_OK;
    }
    GFFX_KEEP_TRY(H, classmap_ensure(H->d_counts, nq * (H->T + 1), "the counts"));
    GFFX_KEEP_TRY(H, classmap_ensure(H->d_class, nq, "the class bytes"));
    const ClassMapView M{H->p_off, H->p_pos, H->p_cls, H->cb, H->n_seq, H->T};
    GFFX_KEEP_HIP(H, hipMemsetAsync(H->ctl, 0, 4, H->stream));
    GFFX_KEEP_HIP(H, hipEventRecord(H->ev[8], H->stream));
    hipLaunchKernelGGL(k_classmap_regions, dim3(classmap_grid(nq, kClassThreads)), dim3(kClassThreads), 0, H->stream, M, rows, (u64)nq, H->d_counts.p, H->d_class.p,
                       H->ctl);
    GFFX_KEEP_HIP(H, hipGetLastError());
    GFFX_KEEP_HIP(H, hipEventRecord(H->ev[9], H->stream));
    uint32_t err = 0;
    GFFX_KEEP_HIP(H, hipMemcpyAsync(&err, H->ctl, 4, hipMemcpyDeviceToHost, H->stream));
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));
    if (err & kClassErrRange) return fail(GFFX_E_CHR_RANGE, "%s: a region has chr >= %u", who, H->n_seq);  // (the run is void, the object stays usable)
    H->ran = true;
    return GFFX_OK;
}

int classmap_results(gffx_hip_classmap *H, const char *who) {
    const int rc = enter_handle(H, who);
    if (rc) return rc;
    if (!H->ran || !H->waited) return fail(GFFX_E_STATE, "%s: no run has been waited for", who);
    return GFFX_OK;
}

}  // namespace

extern "C" uint32_t gffx_hip_classmap_scan_tile(void) { return kClassScanTile; }
extern "C" uint32_t gffx_hip_classmap_block_size(void) { return kClassThreads; }
// tiles per step of k_classmap_carry, _carry_sum and _carry_bases (a block-wide step: one tile per thread)
extern "C" uint32_t gffx_hip_classmap_carry_tiles(void) { return kClassThreads; }

extern "C" void gffx_hip_classmap_destroy(gffx_hip_classmap *H) {
    if (!H) return;
    (void)hipSetDevice(H->device);
    if (H->stream) (void)hipStreamSynchronize(H->stream);
    classmap_drop_points(H);
    for (void *p : {(void *)H->p_off, (void *)H->ctl})
        if (p) (void)hipFree(p);
    if (H->U) gffx_hip_union_destroy(H->U);
    for (hipEvent_t e : H->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : H->perm_ev_free) (void)hipEventDestroy(e);  // (classmap_perm_drop has put them all here)
    if (H->stream) (void)hipStreamDestroy(H->stream);
    delete H;
}

extern "C" int gffx_hip_classmap_create(int device, uint32_t n_seq, uint32_t n_layers, gffx_hip_classmap **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_classmap_create: out is NULL");
    *out = nullptr;
    if (n_layers < 1 || n_layers > classmap::kMaxLayers) return fail(GFFX_E_INVALID, "gffx_hip_classmap_create: %u layers (1 .. 32 are possible)", n_layers);
    if ((uint64_t)n_seq * n_layers > 0xFFFFFFFFull)
        return fail(GFFX_E_INVALID, "gffx_hip_classmap_create: %u seqids x %u layers do not fit 32 bits", n_seq, n_layers);
    gffx_hip_union *U = nullptr;
    int rc = gffx_hip_union_create(device, n_seq * n_layers, &U);  // (looks at the device, too)
    if (rc) return rc;
    std::unique_ptr<gffx_hip_classmap, void (*)(gffx_hip_classmap *)> H(new gffx_hip_classmap, gffx_hip_classmap_destroy);
    H->U = U;
    H->device = device;
    H->n_seq = n_seq, H->T = n_layers;
    GFFX_HIP_TRY(hipSetDevice(device));
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : H->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    if ((rc = dev_alloc_padded(&H->ctl, 8)) || (rc = dev_alloc_padded(&H->p_off, (uint64_t)n_seq + 1))) return rc;
    *out = H.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_add_rows_host(gffx_hip_classmap *H, const uint32_t *rows, uint64_t n_rows) {
    int rc = enter_handle(H, "gffx_hip_classmap_add_rows_host");
    if (rc) return rc;
    if (n_rows && !rows) return fail(GFFX_E_INVALID, "gffx_hip_classmap_add_rows_host: rows is NULL");
    if (!n_rows) return GFFX_OK;
    // (the union's own checks would name pseudo-seqids: the same codes, in the union's order of precedence, with the row's words)
    bool range = false, inverted = false;
    H->pseudo.resize(3 * n_rows);
    for (uint64_t i = 0; i < n_rows; ++i) {
        const uint32_t k = rows[4 * i], c = rows[4 * i + 1], s = rows[4 * i + 2], e = rows[4 * i + 3];
        range |= k >= H->T || c >= H->n_seq;
        inverted |= s >= e;
        H->pseudo[3 * i] = c * H->T + k, H->pseudo[3 * i + 1] = s, H->pseudo[3 * i + 2] = e;  // (wraps only in a refused call)
    }
    if (range) return keep_failure(H, fail(GFFX_E_CHR_RANGE, "gffx_hip_classmap_add_rows_host: a row has layer >= %u or chr >= %u", H->T, H->n_seq));
    if (inverted) return keep_failure(H, fail(GFFX_E_INVALID, "gffx_hip_classmap_add_rows_host: a row has start >= end"));
    H->finished = false;
    GFFX_KEEP_TRY(H, gffx_hip_union_add_host(H->U, H->pseudo.data(), n_rows));
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_finish(gffx_hip_classmap *H) {
    int rc = enter_handle(H, "gffx_hip_classmap_finish");
    if (rc) return rc;
    if (H->finished) return GFFX_OK;
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));  // (no run reads the points that go away next)
    classmap_drop_points(H);
    H->ran = H->waited = false;
    GFFX_KEEP_TRY(H, classmap_build(H));
    H->finished = true;
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_classmap_n_points(const gffx_hip_classmap *H) { return H && H->finished ? H->n_points : 0; }

extern "C" int gffx_hip_classmap_copy_points(gffx_hip_classmap *H, uint64_t *p_off, uint32_t *pos, uint8_t *cls) {
    const int rc = classmap_ready(H, "gffx_hip_classmap_copy_points");
    if (rc) return rc;
    if (p_off) GFFX_KEEP_HIP(H, hipMemcpy(p_off, H->p_off, ((size_t)H->n_seq + 1) * 8, hipMemcpyDeviceToHost));
    if (pos && H->n_points) GFFX_KEEP_HIP(H, hipMemcpy(pos, H->p_pos, H->n_points * 4, hipMemcpyDeviceToHost));
    if (cls && H->n_points) GFFX_KEEP_HIP(H, hipMemcpy(cls, H->p_cls, H->n_points, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_copy_bases(gffx_hip_classmap *H, uint64_t *cb) {
    const int rc = classmap_ready(H, "gffx_hip_classmap_copy_bases");
    if (rc) return rc;
    if (H->n_points && !cb) return fail(GFFX_E_INVALID, "gffx_hip_classmap_copy_bases: cb is NULL");
    if (!H->n_points) return GFFX_OK;
    std::vector<u64> v(H->n_points * H->T);
    GFFX_KEEP_HIP(H, hipMemcpy(v.data(), H->cb, v.size() * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < H->n_points; ++i)  // (the device keeps a point's T sums side by side; the caller gets cb[k][i])
        for (uint32_t k = 0; k < H->T; ++k) cb[k * H->n_points + i] = v[i * H->T + k];
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_run_host(gffx_hip_classmap *H, const uint32_t *regions, uint64_t nq) {
    const int rc = classmap_ready(H, "gffx_hip_classmap_run_host");
    if (rc) return rc;
    if (nq && !regions) return fail(GFFX_E_INVALID, "gffx_hip_classmap_run_host: regions is NULL");
    if (nq) {
        GFFX_KEEP_TRY(H, classmap_ensure(H->d_regions, 3 * nq, "the regions"));
        GFFX_KEEP_HIP(H, hipMemcpyAsync(H->d_regions.p, regions, nq * 12, hipMemcpyHostToDevice, H->stream));
    }
    return classmap_run(H, H->d_regions.p, nq, "gffx_hip_classmap_run_host");  // (it waits for the kernel: the caller's array is free)
}

extern "C" int gffx_hip_classmap_run_store(gffx_hip_classmap *H, const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows) {
    const int rc = classmap_ready(H, "gffx_hip_classmap_run_store");
    if (rc) return rc;
    const uint32_t *rows = nullptr;
    if (const int bad = store_slot_rows(R, k, first, n_rows, H->device, "gffx_hip_classmap_run_store", "class map", &rows)) return bad;
    if (R->pending[k]) GFFX_KEEP_HIP(H, hipStreamWaitEvent(H->stream, R->copied[k], 0));
    return classmap_run(H, rows, n_rows, "gffx_hip_classmap_run_store");  // (the slot is read in place)
}

extern "C" int gffx_hip_classmap_wait(gffx_hip_classmap *H) {
    const int rc = enter_handle(H, "gffx_hip_classmap_wait");
    if (rc) return rc;
    if (!H->ran) return fail(GFFX_E_STATE, "gffx_hip_classmap_wait: nothing has been run");
    if (H->waited) return GFFX_OK;
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));
    float ms = 0.f;
    if (H->nq && hipEventElapsedTime(&ms, H->ev[8], H->ev[9]) == hipSuccess) H->kernel_ms = ms;
    H->waited = true;
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_copy_counts(gffx_hip_classmap *H, uint32_t *counts) {
    const int rc = classmap_results(H, "gffx_hip_classmap_copy_counts");
    if (rc) return rc;
    if (H->nq && !counts) return fail(GFFX_E_INVALID, "gffx_hip_classmap_copy_counts: counts is NULL");
    if (H->nq) GFFX_KEEP_HIP(H, hipMemcpy(counts, H->d_counts.p, H->nq * (H->T + 1) * 4, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_copy_class(gffx_hip_classmap *H, uint8_t *cls) {
    const int rc = classmap_results(H, "gffx_hip_classmap_copy_class");
    if (rc) return rc;
    if (H->nq && !cls) return fail(GFFX_E_INVALID, "gffx_hip_classmap_copy_class: cls is NULL");
    if (H->nq) GFFX_KEEP_HIP(H, hipMemcpy(cls, H->d_class.p, H->nq, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_last_kernel_ms(gffx_hip_classmap *H, double *ms) {
    const int rc = classmap_results(H, "gffx_hip_classmap_last_kernel_ms");
    if (rc) return rc;
    if (!ms) return fail(GFFX_E_INVALID, "gffx_hip_classmap_last_kernel_ms: ms is NULL");
    *ms = H->kernel_ms;
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_stage_ms(const gffx_hip_classmap *H, double *ms /* 6 */) {
    if (!H || !ms) return fail(GFFX_E_INVALID, "gffx_hip_classmap_stage_ms: NULL argument");
    for (int s = 0; s < 6; ++s) ms[s] = H->stage_ms[s];
    return GFFX_OK;
}
