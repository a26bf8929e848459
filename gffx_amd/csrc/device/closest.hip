// closest.hip -- `gffx closest`: the roots nearest to every region, and how far away (the rule: closest_core.hpp).
// A handle belongs to one index and lives on the index's device with a stream of its own.
//   at _create (once per handle, nothing of it on the host):
//   k_closest_keys      position i -> the W = 3 record {seqid, end, position} (the seqid by a search over chr_meta)
//   DeviceSort          stably by (seqid, end): equal ends keep ascending position (radix_sort.hpp)
//   k_closest_unpack    the END TABLE e_end[], e_pos[]; seqid c's slice is [chr_meta[c].x, chr_meta[c].y), as in start[] / aux[]
//   per run, regions in INPUT order, the launch structure of k_join_count / k_join_emit (join_a_kernels.hpp):
//   k_closest_count     one region per thread, a contiguous chunk of regions per block: the count and the gap of every region, one
//                       partial sum per block (no atomics on the output)
//   k_closest_emit      block base = the sum of the preceding blocks' partial sums, a block scan per 256-region tile gives every
//                       region its CSR offset; the answer is found again and its triples stored in ascending position
// Per region: ONE bin record gives p = #{start < qe} (locate); at most ONE aux record gives the largest end over [first, p) --
// a root overlaps iff it exceeds qs.  With an overlap (and without IGNORE_OVERLAPS) the answer is Join A's sweep, stored in
// reverse; otherwise the run of equal starts at p and / or the run of equal ends before j = #{end <= qs} = p - (overlapping
// roots), which needs no search (closest_core.hpp: nearest; with IGNORE_OVERLAPS the sweep counts them).  The host sizes the
// triples from the count pass's total before the emit pass is enqueued.
// Roofline bound: latency of dependent gathers from the L2-resident index (like Join A).
#include <algorithm>
#include <cstring>
#include <memory>

#include "engine_private.hpp"
#include "closest_core.hpp"
#include "handle_status.hpp"
#include "join_a_kernels.hpp"
#include "radix_sort.hpp"
#include "regions_store.hpp"

namespace gffx {

constexpr uint32_t kClosestMaxBlocks = 2048;  // (the direct strategy's default: 8 resident 256-thread blocks per CU)

struct ClosestOut {
    uint32_t *counts;         // nq
    uint32_t *gaps;           // nq
    u64 *block_sums;          // n_blocks
    u64 *offsets;             // nq + 1
    uint32_t *triples;        // 3 * capacity
    u64 capacity;             // pairs
    uint32_t *err;            // bit 0: a region with chr >= n_chr
};

struct EndTable {
    const uint32_t *e_end, *e_pos;
};

__global__ __launch_bounds__(256) void k_closest_keys(const uint4 *chr_meta, uint32_t n_chr, const uint4 *aux, uint32_t n_roots, uint32_t *rec) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_roots) return;
    // the seqid of position i: the first c with chr_meta[c].y > i (y ascends with c; chr_meta[n_chr - 1].y == n_roots > i)
    const uint32_t c = closest::first_gt(0u, n_chr - 1u, i, [&](uint32_t k) { return chr_meta[k].y; });
    rec[3ull * i] = c;
    rec[3ull * i + 1] = aux[i].x;
    rec[3ull * i + 2] = i;
}

__global__ __launch_bounds__(256) void k_closest_unpack(const uint32_t *rec, uint32_t n_roots, uint32_t *e_end, uint32_t *e_pos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_roots) return;
    e_end[i] = rec[3ull * i + 1];
    e_pos[i] = rec[3ull * i + 2];
}

// What answers a region of a seqid with roots: its overlaps (the sweep from p) or the runs of `near`
struct ClosestPlan {
    bool over;
    uint32_t p;
    closest::Nearest near;
};

__device__ __forceinline__ ClosestPlan closest_plan(const IndexView &ix, const EndTable &et, const uint4 meta, uint32_t qs, uint32_t qe, uint32_t flags) {
    ClosestPlan pl;
    bool dead;
    pl.p = locate(ix, meta, qs, qe, &dead);
    // clamp: nothing the bin directory says may lead outside the seqid's slice
    pl.p = min(max(pl.p, meta.x), meta.y);
    pl.over = false;
    if (!dead && pl.p > meta.x) {  // (dead: the bin record alone said that nothing before p reaches past qs)
        const uint4 a = ix.aux[pl.p - 1];
        pl.over = max(a.x, a.y) > qs;
    }
    if (pl.over && !(flags & closest::kIgnoreOverlaps)) return pl;
    uint32_t n_over = 0;
    if (pl.over && !(flags & closest::kRightOnly)) {  // IGNORE_OVERLAPS: the overlapping roots only say where the LEFT roots end in the end table
        uint32_t p = pl.p;
        sweep_kept<GFFX_MODE_OVERLAP, false>(
            p, meta.x, qs, qe, [&](uint32_t k) { return ix.aux[k]; }, [&](uint32_t k) { return ix.start[k]; },
            [&](uint32_t, uint32_t, const uint4 &) {
                ++n_over;
                return true;
            });
    }
    pl.over = false;
    pl.near = closest::nearest(
        meta.x, meta.y, pl.p, n_over, qs, qe, flags, [&](uint32_t i) { return ix.start[i]; }, [&](uint32_t j) { return et.e_end[j]; });
    return pl;
}

template <bool META_LDS>
__global__ __launch_bounds__(kJoinThreads) void k_closest_count(IndexView ix, EndTable et, const uint32_t *regions, u64 nq, u64 chunk, uint32_t flags,
                                                                ClosestOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *sh = reinterpret_cast<u64 *>(smem);  // 32 B
    const uint4 *cm = stage_meta<META_LDS>(ix, smem + 32);
    const u64 beg = (u64)blockIdx.x * chunk;
    u64 end = beg + chunk;
    if (end > nq) end = nq;
    u64 local = 0;
    bool bad = false;
    for (u64 i = beg + threadIdx.x; i < end; i += kJoinThreads) {
        const uint32_t chr = regions[3 * i], qs = regions[3 * i + 1], qe = regions[3 * i + 2];
        uint32_t cnt = 0, gap = 0;
        if (chr >= ix.n_chr) {
            bad = true;  // (nothing is read for the row)
        } else if (qs < qe) {
            const uint4 meta = cm[chr];
            if (meta.x != meta.y) {
                const ClosestPlan pl = closest_plan(ix, et, meta, qs, qe, flags);
                if (pl.over) {
                    uint32_t p = pl.p;
                    sweep_kept<GFFX_MODE_OVERLAP, false>(
                        p, meta.x, qs, qe, [&](uint32_t k) { return ix.aux[k]; }, [&](uint32_t k) { return ix.start[k]; },
                        [&](uint32_t, uint32_t, const uint4 &) {
                            ++cnt;
                            return true;
                        });
                } else {
                    cnt = pl.near.count();
                    gap = pl.near.gap;
                }
            }
        }
        out.counts[i] = cnt;
        out.gaps[i] = gap;
        local += cnt;
    }
    if (bad) atomicOr(out.err, 1u);
    const u64 tot = block_reduce_add(local, sh);
    if (threadIdx.x == 0) out.block_sums[blockIdx.x] = tot;
}

template <bool META_LDS>
__global__ __launch_bounds__(kJoinThreads) void k_closest_emit(IndexView ix, EndTable et, const uint32_t *regions, u64 nq, u64 chunk, uint32_t flags,
                                                               ClosestOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *sh64 = reinterpret_cast<u64 *>(smem);                 // 32 B
    uint32_t *sh32 = reinterpret_cast<uint32_t *>(smem + 32);  // 16 B
    const uint4 *cm = stage_meta<META_LDS>(ix, smem + 48);
    const u64 beg = (u64)blockIdx.x * chunk;
    u64 end = beg + chunk;
    if (end > nq) end = nq;
    u64 part = 0;
    for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kJoinThreads) part += out.block_sums[j];
    u64 base = block_reduce_add(part, sh64);
    auto store = [&](u64 o, uint32_t pos) {  // the triple of the root at `pos` (inside the seqid's slice) as pair o
        if (o < out.capacity) {
            const uint4 a = ix.aux[pos];
            uint32_t *t = out.triples + 3ull * o;
            t[0] = a.w;
            t[1] = ix.start[pos];
            t[2] = a.x;
        }
    };
    for (u64 tile = beg; tile < end; tile += kJoinThreads) {
        const u64 i = tile + threadIdx.x;
        const bool live = i < end;
        const uint32_t cnt = live ? out.counts[i] : 0u;
        uint32_t tile_total;
        const uint32_t excl = block_exclusive_scan(cnt, sh32, &tile_total);
        const u64 pos = base + excl;
        if (live) out.offsets[i] = pos;
        if (cnt) {  // (a counted region has chr < n_chr, qs < qe and a seqid with roots)
            const uint32_t chr = regions[3 * i], qs = regions[3 * i + 1], qe = regions[3 * i + 2];
            const uint4 meta = cm[chr];
            const ClosestPlan pl = closest_plan(ix, et, meta, qs, qe, flags);
            if (pl.over) {
                uint32_t p = pl.p, done = 0;  // the sweep descends: pair cnt - 1 first
                sweep_kept<GFFX_MODE_OVERLAP, false>(
                    p, meta.x, qs, qe, [&](uint32_t k) { return ix.aux[k]; }, [&](uint32_t k) { return ix.start[k]; },
                    [&](uint32_t k, uint32_t, const uint4 &) {
                        ++done;
                        store(pos + (cnt - done), k);
                        return done < cnt;
                    });
            } else {
                uint32_t done = 0;
                for (uint32_t j = pl.near.l0; j < pl.near.l1 && done < cnt; ++j) {
                    const uint32_t k = et.e_pos[j];
                    if (k >= meta.x && k < meta.y) store(pos + done, k);  // (the table is the handle's own; the test costs nothing)
                    ++done;
                }
                for (uint32_t k = pl.near.r0; k < pl.near.r1 && done < cnt; ++k) store(pos + done++, k);
            }
        }
        base += tile_total;
    }
    if (end == nq && beg < nq && threadIdx.x == 0) out.offsets[nq] = base;
}

}  // namespace gffx

struct gffx_hip_closest : gffx::HandleStatus {
    static constexpr const char *kName = "closest", *kNoun = "object";
    const gffx_hip_index *ix = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};  // count: 0 .. 1, emit: 2 .. 3
    hipEvent_t build[2] = {};
    uint64_t max_q = 0, nq = 0;
    uint32_t *d_regions = nullptr;  // _run_host: the regions' copy
    uint32_t *d_counts = nullptr, *d_gaps = nullptr;
    u64 *d_offsets = nullptr, *d_block_sums = nullptr;
    uint32_t *d_err = nullptr;
    DevArr<uint32_t> triples;  // 3 words per pair
    uint32_t *e_end = nullptr, *e_pos = nullptr;  // the end table, n_roots each
    u64 *h_sums = nullptr;     // pinned: the blocks' partial sums, then the error word
    uint32_t n_blocks = 0;
    uint64_t chunk = 0, total = 0;
    bool ran = false, waited = false;
    double kernel_ms = 0, build_ms = 0;
    uint64_t grows = 0;
};

namespace {

// the end table: sorted on the device, once
int closest_build(gffx_hip_closest *H) {
    const gffx_hip_index *ix = H->ix;
    const uint32_t n = ix->n_roots;
    int rc;
    if ((rc = dev_alloc(&H->e_end, n)) || (rc = dev_alloc(&H->e_pos, n))) return rc;
    if (!n) return GFFX_OK;
    SortPlan plan{};
    // by (seqid, end): the four bytes of the end, then as many bytes of the seqid as n_chr needs
    int seq_bytes = 1;
    while (seq_bytes < 4 && (ix->n_chr > (1u << (8 * seq_bytes)))) seq_bytes++;
    for (int b = 0; b < 4; ++b) plan.word[plan.n_passes] = 1, plan.shift[plan.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < seq_bytes; ++b) plan.word[plan.n_passes] = 0, plan.shift[plan.n_passes++] = (uint8_t)(8 * b);
    uint32_t *buf[2] = {nullptr, nullptr}, *work = nullptr, *sorted = nullptr;
    auto release = [&]() {
        for (uint32_t *p : {buf[0], buf[1], work})
            if (p) (void)hipFree(p);
    };
    if ((rc = dev_alloc(&buf[0], 3 * (size_t)n)) || (rc = dev_alloc(&buf[1], 3 * (size_t)n)) ||
        (rc = dev_alloc(&work, DeviceSort::work_words(n, plan.n_passes)))) {
        release();
        return rc;
    }
    const uint32_t grid = (n + 255u) / 256u;
    rc = [&]() -> int {
        GFFX_HIP_TRY(hipMemsetAsync(H->d_err, 0, 4, H->stream));
        GFFX_HIP_TRY(hipEventRecord(H->build[0], H->stream));
        hipLaunchKernelGGL(k_closest_keys, dim3(grid), dim3(256), 0, H->stream, ix->d_chr_meta, ix->n_chr, ix->d_aux, n, buf[0]);
        GFFX_HIP_TRY(hipGetLastError());
        const int src = DeviceSort::run<3>(H->stream, buf[0], buf[1], n, plan, ix->n_chr, work, H->d_err, &sorted);
        if (src) return src;
        hipLaunchKernelGGL(k_closest_unpack, dim3(grid), dim3(256), 0, H->stream, sorted, n, H->e_end, H->e_pos);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(H->build[1], H->stream));
        uint32_t err = 0;
        GFFX_HIP_TRY(hipMemcpyAsync(&err, H->d_err, 4, hipMemcpyDeviceToHost, H->stream));
        GFFX_HIP_TRY(hipStreamSynchronize(H->stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, H->build[0], H->build[1]) == hipSuccess) H->build_ms = ms;
        if (err & 4u) return fail(GFFX_E_HIP, "gffx_hip_closest_create: the device sort timed out waiting for an earlier tile");
        if (err & 2u) return fail(GFFX_E_INVALID, "gffx_hip_closest_create: the index's seqid records do not cover its roots");
        return GFFX_OK;
    }();
    if (rc) (void)hipStreamSynchronize(H->stream);  // (nothing may still read what is freed next)
    release();
    return rc;
}

// count pass, the pair buffer, emit pass; `regions`: nq device rows the stream may read from now on
int closest_run(gffx_hip_closest *H, const uint32_t *regions, uint64_t nq, uint32_t flags) {
    const gffx_hip_index *ix = H->ix;
    H->ran = H->waited = false;
    H->nq = nq;
    H->total = 0;
    H->kernel_ms = 0;
    const uint64_t tiles = (nq + kJoinThreads - 1) / kJoinThreads;
    const uint64_t tiles_per_block = std::max<uint64_t>(1, (tiles + kClosestMaxBlocks - 1) / kClosestMaxBlocks);
    H->chunk = tiles_per_block * kJoinThreads;
    H->n_blocks = (uint32_t)((nq + H->chunk - 1) / H->chunk);
    if (!nq) {
        GFFX_KEEP_HIP(H, hipMemsetAsync(H->d_offsets, 0, 8, H->stream));
        H->ran = true;
        return GFFX_OK;
    }
    const bool ml = meta_bytes(ix) <= kMetaLdsBytes;
    const uint32_t lds = ml ? meta_bytes(ix) : 0u;
    const EndTable et{H->e_end, H->e_pos};
    ClosestOut out{H->d_counts, H->d_gaps, H->d_block_sums, H->d_offsets, H->triples.p, (u64)(H->triples.cap / 3), H->d_err};
    GFFX_KEEP_HIP(H, hipMemsetAsync(H->d_err, 0, 4, H->stream));
    GFFX_KEEP_HIP(H, hipEventRecord(H->ev[0], H->stream));
    if (ml)
        hipLaunchKernelGGL(k_closest_count<true>, dim3(H->n_blocks), dim3(kJoinThreads), 32 + lds, H->stream, ix->view(), et, regions, (u64)nq, (u64)H->chunk,
                           flags, out);
    else
        hipLaunchKernelGGL(k_closest_count<false>, dim3(H->n_blocks), dim3(kJoinThreads), 32, H->stream, ix->view(), et, regions, (u64)nq, (u64)H->chunk,
                           flags, out);
    GFFX_KEEP_HIP(H, hipGetLastError());
    GFFX_KEEP_HIP(H, hipEventRecord(H->ev[1], H->stream));
    GFFX_KEEP_HIP(H, hipMemcpyAsync(H->h_sums, H->d_block_sums, (size_t)H->n_blocks * 8, hipMemcpyDeviceToHost, H->stream));
    GFFX_KEEP_HIP(H, hipMemcpyAsync(H->h_sums + kClosestMaxBlocks, H->d_err, 4, hipMemcpyDeviceToHost, H->stream));
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));
    if (*reinterpret_cast<const uint32_t *>(H->h_sums + kClosestMaxBlocks) & 1u)
        return fail(GFFX_E_CHR_RANGE, "gffx_hip_closest: a region has chr >= %u", ix->n_chr);  // (the run is void, the object stays usable)
    uint64_t total = 0;
    for (uint32_t b = 0; b < H->n_blocks; ++b) total += H->h_sums[b];
    if (3 * total > H->triples.cap) {
        const hipError_t e = H->triples.ensure((size_t)(3 * total));
        if (e != hipSuccess)
            return keep_failure(H, fail(e == hipErrorOutOfMemory ? GFFX_E_OOM : GFFX_E_HIP, "gffx_hip_closest: no room for %llu pairs: %s",
                                        (unsigned long long)total, hipGetErrorString(e)));
        H->grows++;
    }
    out.triples = H->triples.p;
    out.capacity = H->triples.cap / 3;
    GFFX_KEEP_HIP(H, hipEventRecord(H->ev[2], H->stream));
    if (ml)
        hipLaunchKernelGGL(k_closest_emit<true>, dim3(H->n_blocks), dim3(kJoinThreads), 48 + lds, H->stream, ix->view(), et, regions, (u64)nq, (u64)H->chunk,
                           flags, out);
    else
        hipLaunchKernelGGL(k_closest_emit<false>, dim3(H->n_blocks), dim3(kJoinThreads), 48, H->stream, ix->view(), et, regions, (u64)nq, (u64)H->chunk,
                           flags, out);
    GFFX_KEEP_HIP(H, hipGetLastError());
    GFFX_KEEP_HIP(H, hipEventRecord(H->ev[3], H->stream));
    H->total = total;
    H->ran = true;
    return GFFX_OK;
}

int closest_results(gffx_hip_closest *H, const char *who) {
    const int rc = enter_handle(H, who);
    if (rc) return rc;
    if (!H->ran || !H->waited) return fail(GFFX_E_STATE, "%s: no run has been waited for", who);
    return GFFX_OK;
}

// (looked at before the handle: the flags' rule needs no device)
int closest_check_flags(uint32_t flags, const char *who) {
    if (!closest::flags_ok(flags)) return fail(GFFX_E_INVALID, "%s: bad flags 0x%x (an unknown bit, or LEFT_ONLY with RIGHT_ONLY)", who, flags);
    return GFFX_OK;
}

int closest_check_nq(const gffx_hip_closest *H, uint64_t nq, const char *who) {
    if (nq > H->max_q) return fail(GFFX_E_INVALID, "%s: %llu regions exceed the handle's %llu", who, (unsigned long long)nq, (unsigned long long)H->max_q);
    return GFFX_OK;
}

}  // namespace

extern "C" void gffx_hip_closest_destroy(gffx_hip_closest *H) {
    if (!H) return;
    (void)hipSetDevice(H->device);
    if (H->stream) (void)hipStreamSynchronize(H->stream);
    for (void *p : {(void *)H->d_regions, (void *)H->d_counts, (void *)H->d_gaps, (void *)H->d_offsets, (void *)H->d_block_sums, (void *)H->d_err,
                    (void *)H->e_end, (void *)H->e_pos})
        if (p) (void)hipFree(p);
    if (H->h_sums) (void)hipHostFree(H->h_sums);
    for (hipEvent_t e : H->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : H->build)
        if (e) (void)hipEventDestroy(e);
    if (H->stream) (void)hipStreamDestroy(H->stream);
    delete H;
}

extern "C" int gffx_hip_closest_create(const gffx_hip_index *ix, uint64_t max_queries, gffx_hip_closest **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_closest_create: out is NULL");
    *out = nullptr;
    if (device_count_quiet() <= 0) return fail(GFFX_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (!ix) return fail(GFFX_E_INVALID, "gffx_hip_closest_create: index is NULL");
    if (max_queries >= (1ull << 40)) return fail(GFFX_E_INVALID, "gffx_hip_closest_create: max_queries too large");
    GFFX_HIP_TRY(hipSetDevice(ix->device));
    std::unique_ptr<gffx_hip_closest, void (*)(gffx_hip_closest *)> H(new gffx_hip_closest, gffx_hip_closest_destroy);
    H->ix = ix;
    H->device = ix->device;
    H->max_q = max_queries;
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : H->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    for (hipEvent_t &e : H->build) GFFX_HIP_TRY(hipEventCreate(&e));
    GFFX_HIP_TRY(hipHostMalloc((void **)&H->h_sums, (kClosestMaxBlocks + 1) * 8, hipHostMallocDefault));
    std::memset(H->h_sums, 0, (kClosestMaxBlocks + 1) * 8);
    int rc;
    if ((rc = dev_alloc(&H->d_regions, 3 * (size_t)max_queries)) || (rc = dev_alloc(&H->d_counts, (size_t)max_queries)) ||
        (rc = dev_alloc(&H->d_gaps, (size_t)max_queries)) || (rc = dev_alloc(&H->d_offsets, (size_t)max_queries + 1)) ||
        (rc = dev_alloc(&H->d_block_sums, (size_t)kClosestMaxBlocks)) || (rc = dev_alloc(&H->d_err, 1)))
        return rc;
    // (a first guess of one pair per region; a run that needs more grows the buffer between its two passes)
    const hipError_t e = H->triples.ensure(3 * std::max<size_t>((size_t)max_queries, 64));
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? GFFX_E_OOM : GFFX_E_HIP, "gffx_hip_closest_create: hipMalloc failed: %s", hipGetErrorString(e));
    if ((rc = closest_build(H.get()))) return rc;
    *out = H.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_run_host(gffx_hip_closest *H, const uint32_t *regions, uint64_t nq, uint32_t flags) {
    int rc = closest_check_flags(flags, "gffx_hip_closest_run_host");
    if (rc || (rc = enter_handle(H, "gffx_hip_closest_run_host")) || (rc = closest_check_nq(H, nq, "gffx_hip_closest_run_host"))) return rc;
    if (nq && !regions) return fail(GFFX_E_INVALID, "gffx_hip_closest_run_host: regions is NULL");
    // (closest_run waits for the count pass, which runs behind this copy: the caller's array is free when the call returns)
    if (nq) GFFX_KEEP_HIP(H, hipMemcpyAsync(H->d_regions, regions, nq * 12, hipMemcpyHostToDevice, H->stream));
    return closest_run(H, H->d_regions, nq, flags);
}

extern "C" int gffx_hip_closest_run_store(gffx_hip_closest *H, const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows, uint32_t flags) {
    int rc = closest_check_flags(flags, "gffx_hip_closest_run_store");
    if (rc || (rc = enter_handle(H, "gffx_hip_closest_run_store"))) return rc;
    if ((rc = closest_check_nq(H, n_rows, "gffx_hip_closest_run_store"))) return rc;
    const uint32_t *rows = nullptr;
    if ((rc = store_slot_rows(R, k, first, n_rows, H->device, "gffx_hip_closest_run_store", "index", &rows))) return rc;
    if (R->pending[k]) GFFX_KEEP_HIP(H, hipStreamWaitEvent(H->stream, R->copied[k], 0));
    return closest_run(H, rows, n_rows, flags);  // (the slot is read in place: no copy)
}

extern "C" int gffx_hip_closest_wait(gffx_hip_closest *H) {
    const int rc = enter_handle(H, "gffx_hip_closest_wait");
    if (rc) return rc;
    if (!H->ran) return fail(GFFX_E_STATE, "gffx_hip_closest_wait: nothing has been run");
    if (H->waited) return GFFX_OK;
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));
    if (H->nq) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, H->ev[0], H->ev[1]) == hipSuccess && hipEventElapsedTime(&b, H->ev[2], H->ev[3]) == hipSuccess) H->kernel_ms = (double)a + b;
    }
    H->waited = true;
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_total_pairs(gffx_hip_closest *H, uint64_t *pairs) {
    const int rc = closest_results(H, "gffx_hip_closest_total_pairs");
    if (rc) return rc;
    if (!pairs) return fail(GFFX_E_INVALID, "gffx_hip_closest_total_pairs: pairs is NULL");
    *pairs = H->total;
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_copy_counts(gffx_hip_closest *H, uint32_t *counts) {
    const int rc = closest_results(H, "gffx_hip_closest_copy_counts");
    if (rc) return rc;
    if (H->nq && !counts) return fail(GFFX_E_INVALID, "gffx_hip_closest_copy_counts: counts is NULL");
    if (H->nq) GFFX_KEEP_HIP(H, hipMemcpy(counts, H->d_counts, H->nq * 4, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_copy_gaps(gffx_hip_closest *H, uint32_t *gaps) {
    const int rc = closest_results(H, "gffx_hip_closest_copy_gaps");
    if (rc) return rc;
    if (H->nq && !gaps) return fail(GFFX_E_INVALID, "gffx_hip_closest_copy_gaps: gaps is NULL");
    if (H->nq) GFFX_KEEP_HIP(H, hipMemcpy(gaps, H->d_gaps, H->nq * 4, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_copy_offsets(gffx_hip_closest *H, uint64_t *offsets) {
    const int rc = closest_results(H, "gffx_hip_closest_copy_offsets");
    if (rc) return rc;
    if (!offsets) return fail(GFFX_E_INVALID, "gffx_hip_closest_copy_offsets: offsets is NULL");
    GFFX_KEEP_HIP(H, hipMemcpy(offsets, H->d_offsets, (H->nq + 1) * 8, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_copy_triples(gffx_hip_closest *H, uint32_t *triples) {
    const int rc = closest_results(H, "gffx_hip_closest_copy_triples");
    if (rc) return rc;
    if (H->total && !triples) return fail(GFFX_E_INVALID, "gffx_hip_closest_copy_triples: triples is NULL");
    if (H->total) GFFX_KEEP_HIP(H, hipMemcpy(triples, H->triples.p, H->total * 12, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_copy_end_table(gffx_hip_closest *H, uint32_t *e_end, uint32_t *e_pos) {
    const int rc = enter_handle(H, "gffx_hip_closest_copy_end_table");
    if (rc) return rc;
    const size_t n = H->ix->n_roots;
    if (n && e_end) GFFX_KEEP_HIP(H, hipMemcpy(e_end, H->e_end, n * 4, hipMemcpyDeviceToHost));
    if (n && e_pos) GFFX_KEEP_HIP(H, hipMemcpy(e_pos, H->e_pos, n * 4, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_last_kernel_ms(gffx_hip_closest *H, double *ms) {
    const int rc = closest_results(H, "gffx_hip_closest_last_kernel_ms");
    if (rc) return rc;
    if (!ms) return fail(GFFX_E_INVALID, "gffx_hip_closest_last_kernel_ms: ms is NULL");
    *ms = H->kernel_ms;
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_last_grid(const gffx_hip_closest *H, uint32_t *blocks, uint64_t *chunk) {
    if (!H) return fail(GFFX_E_INVALID, "gffx_hip_closest_last_grid: closest is NULL");
    if (blocks) *blocks = H->n_blocks;
    if (chunk) *chunk = H->chunk;
    return GFFX_OK;
}

extern "C" int gffx_hip_closest_stats(const gffx_hip_closest *H, double *build_ms, uint64_t *grows) {
    if (!H) return fail(GFFX_E_INVALID, "gffx_hip_closest_stats: closest is NULL");
    if (build_ms) *build_ms = H->build_ms;
    if (grows) *grows = H->grows;
    return GFFX_OK;
}
