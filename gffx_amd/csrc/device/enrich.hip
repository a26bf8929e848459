// enrich.hip -- `gffx enrich`: the permutation totals of regions against the classes of a finished class map (DESIGN 22;
// enrich_core.hpp has the definition, the random numbers and the placement rule).  The totals live on the class map object
// (classmap_private.hpp): two matrices of (n_perm + 1) x (T + 1) 64-bit sums -- bases and regions per class; row 0 the
// observed data -- and the count of unplaceable regions.  A run adds its regions to them; nothing is written per region.
//   k_classmap_perm_check  one thread per region: a row with chr >= n_seq marks the run (and the wait) -- the run is void
//   k_classmap_permute     a block holds a tile of kClassThreads regions in registers (one per thread, read once) and walks a
//                          GROUP of kPermGroup rows of the totals: per row it draws, places and answers the region with the two
//                          side-by-side searches of the region rule, and adds its non-zero bases and its class into the block's
//                          LDS accumulators [kPermGroup][T + 1] (integer LDS atomics on an address that is the same for the whole
//                          wave).  At the end the block adds its non-zero
//                          accumulators to the global matrices with 64-bit atomicAdd.  Grid: region tiles x row groups, the
//                          groups of a tile next to each other.  Integer sums: the order of the adds does not matter.
// Roofline bound: latency, like k_classmap_regions: ~2 log2(points per seqid) dependent loads per placement; the totals'
// atomics are (tiles x rows x (T + 1) x 2) 8-byte adds, three orders of magnitude below the loads of the searches.
#include <cstdlib>
#include <utility>

#include "classmap_private.hpp"
#include "enrich_core.hpp"
#include "regions_store.hpp"

namespace gffx {

#ifndef GFFX_PERM_GROUP
#define GFFX_PERM_GROUP 8
#endif
constexpr uint32_t kPermGroup = GFFX_PERM_GROUP;  // rows of the totals per block (16 and 32 measured: profiles/enrich_group.txt)
constexpr uint32_t kPermCells = kPermGroup * (classmap::kMaxLayers + 1);
// Blocks per launch: HIP refuses a launch with gridDim.x * blockDim.x >= 2^32, so 2^23 blocks of 256 threads at the most.
// GFFX_HIP_PERM_LAUNCH_BLOCKS (1 .. 2^23, read by _perm_begin) lowers it: the totals do not depend on it (tests take the
// path of several launches with it)
constexpr uint64_t kPermMaxBlocks = 1ull << 23;
static_assert(kPermMaxBlocks * kClassThreads < (1ull << 32), "a launch must stay below 2^32 threads");
constexpr uint32_t kPermCheckBlocks = 1u << 16;  // k_classmap_perm_check strides over the rows beyond these

__global__ __launch_bounds__(kClassThreads) void k_classmap_perm_check(const uint32_t *rows, u64 nq, uint32_t n_seq, uint32_t *ctl) {
    for (u64 i = (u64)blockIdx.x * kClassThreads + threadIdx.x; i < nq; i += (u64)gridDim.x * kClassThreads)
        if (rows[3 * i] >= n_seq) atomicOr(ctl, 1u), atomicOr(ctl + 1, 1u);
}

// Regions [tile0 * kClassThreads ..) of rows[0 .. 3 nq), region j being global row first_row + j, into the totals.  Block b:
// tile tile0 + b / n_groups, rows (b % n_groups) * kPermGroup .. of the totals.  ctl[0] != 0: the run is void
__global__ __launch_bounds__(kClassThreads) void k_classmap_permute(ClassMapView M, const uint32_t *rows, u64 nq, u64 first_row, const uint32_t *seq_len,
                                                                    uint32_t n_perm, u64 seed, u64 tile0, uint32_t n_groups, u64 *bases, u64 *regions, u64 *unplaced,
                                                                    const uint32_t *ctl) {
    __shared__ u64 s_bases[kPermCells];
    __shared__ uint32_t s_regions[kPermCells];
    __shared__ uint32_t s_unplaced;
    if (ctl[0]) return;  // (the same word for every thread of every block)
    const uint32_t T = M.T, T1 = T + 1;
    const u64 tile = tile0 + blockIdx.x / n_groups;
    const uint32_t p0 = (blockIdx.x % n_groups) * kPermGroup;
    const uint32_t n_rows = min(kPermGroup, n_perm + 1 - p0), cells = n_rows * T1;  // (p0 <= n_perm: n_groups covers n_perm + 1 rows)
    for (uint32_t x = threadIdx.x; x < cells; x += kClassThreads) s_bases[x] = 0ull, s_regions[x] = 0u;
    if (threadIdx.x == 0) s_unplaced = 0u;
    __syncthreads();
    const u64 j = tile * kClassThreads + threadIdx.x;
    if (j < nq) {
        const uint32_t c = rows[3 * j], qs = rows[3 * j + 1], qe = rows[3 * j + 2];
        if (c < M.n_seq) {  // (k_classmap_perm_check has voided a run with such a row: nothing is read for it here either)
            const u64 lo = M.p_off[c], hi = M.p_off[c + 1];
            const uint32_t L = seq_len[c];
            for (uint32_t r = 0; r < n_rows; ++r) {
                const uint32_t p = p0 + r;
                u64 *row_bases = s_bases + r * T1;
                uint32_t *row_regions = s_regions + r * T1;
                const enrich::Placement how = enrich::region_in_row(
                    M.p_pos, M.p_cls, M.cb, T, lo, hi, L, qs, qe, p == 0, enrich::perm_draw(enrich::perm_key(seed, p), first_row + j),
                    [&](uint32_t k, uint32_t n) { atomicAdd(row_bases + k, (u64)n); }, [&](uint32_t k) { atomicAdd(row_regions + k, 1u); });
                if (p == 0 && how == enrich::kUnplaceable) atomicAdd(&s_unplaced, 1u);  // (once per region: only row 0's block counts)
            }
        }
    }
    __syncthreads();
    const u64 at = (u64)p0 * T1;  // (a group's cells lie side by side in the matrices as in LDS)
    for (uint32_t x = threadIdx.x; x < cells; x += kClassThreads) {
        if (s_bases[x]) atomicAdd(bases + at + x, s_bases[x]);
        if (s_regions[x]) atomicAdd(regions + at + x, (u64)s_regions[x]);
    }
    if (threadIdx.x == 0 && s_unplaced) atomicAdd(unplaced, (u64)s_unplaced);
}

void classmap_perm_drop(gffx_hip_classmap *H) {
    for (void *p : {(void *)H->perm_totals, (void *)H->perm_len, (void *)H->perm_ctl})
        if (p) (void)hipFree(p);
    H->perm_totals = nullptr, H->perm_len = nullptr, H->perm_ctl = nullptr;
    for (auto &pr : H->perm_ev) H->perm_ev_free.push_back(pr.first), H->perm_ev_free.push_back(pr.second);
    H->perm_ev.clear();
    H->perm_open = H->perm_waited = false;
    H->n_perm = 0;
    H->perm_kernel_ms = 0;
}

}  // namespace gffx

using namespace gffx;

namespace {

uint64_t perm_cells(const gffx_hip_classmap *H) { return ((uint64_t)H->n_perm + 1) * (H->T + 1); }

int perm_ready(gffx_hip_classmap *H, const char *who) {
    const int rc = classmap_ready(H, who);
    if (rc) return rc;
    if (!H->perm_open) return fail(GFFX_E_STATE, "%s: call gffx_hip_classmap_perm_begin first", who);
    return GFFX_OK;
}

int perm_event(gffx_hip_classmap *H, hipEvent_t *e) {
    if (!H->perm_ev_free.empty()) {
        *e = H->perm_ev_free.back();
        H->perm_ev_free.pop_back();
        return GFFX_OK;
    }
    GFFX_HIP_TRY(hipEventCreate(e));
    return GFFX_OK;
}

// the rows lie on the device, ordered before what comes next on the object's stream
int perm_run(gffx_hip_classmap *H, const uint32_t *rows, uint64_t nq, uint64_t first_row) {
    H->perm_waited = false;
    if (!nq) return GFFX_OK;
    const ClassMapView M{H->p_off, H->p_pos, H->p_cls, H->cb, H->n_seq, H->T};
    const uint64_t cells = perm_cells(H);
    u64 *bases = H->perm_totals, *regions = bases + cells, *unplaced = regions + cells;
    const uint32_t n_groups = (H->n_perm + 1 + kPermGroup - 1) / kPermGroup;
    const uint64_t tiles = (nq + kClassThreads - 1) / kClassThreads, tiles_per_launch = std::max<uint64_t>(1, H->perm_launch_blocks / n_groups);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    GFFX_KEEP_TRY(H, perm_event(H, &e0));
    if (const int rc = perm_event(H, &e1)) {
        H->perm_ev_free.push_back(e0);  // (it stays the object's)
        return keep_failure(H, rc);
    }
    H->perm_ev.emplace_back(e0, e1);
    GFFX_KEEP_HIP(H, hipMemsetAsync(H->perm_ctl, 0, 4, H->stream));
    GFFX_KEEP_HIP(H, hipEventRecord(e0, H->stream));
    hipLaunchKernelGGL(k_classmap_perm_check, dim3((uint32_t)std::min<uint64_t>((nq + kClassThreads - 1) / kClassThreads, kPermCheckBlocks)), dim3(kClassThreads), 0, H->stream, rows, (u64)nq,
                       H->n_seq, H->perm_ctl);
    for (uint64_t t0 = 0; t0 < tiles; t0 += tiles_per_launch) {
        const uint64_t n = std::min(tiles_per_launch, tiles - t0);
        hipLaunchKernelGGL(k_classmap_permute, dim3((uint32_t)(n * n_groups)), dim3(kClassThreads), 0, H->stream, M, rows, (u64)nq, (u64)first_row,
                           (const uint32_t *)H->perm_len, H->n_perm, (u64)H->perm_seed, (u64)t0, n_groups, bases, regions, unplaced, (const uint32_t *)H->perm_ctl);
    }
    GFFX_KEEP_HIP(H, hipGetLastError());
    GFFX_KEEP_HIP(H, hipEventRecord(e1, H->stream));
    return GFFX_OK;
}

}  // namespace

extern "C" uint32_t gffx_hip_classmap_perm_group(void) { return kPermGroup; }

extern "C" int gffx_hip_classmap_perm_begin(gffx_hip_classmap *H, const uint32_t *seq_len, uint32_t n_perm, uint64_t seed) {
    const int rc = classmap_ready(H, "gffx_hip_classmap_perm_begin");
    if (rc) return rc;
    if (H->n_seq && !seq_len) return fail(GFFX_E_INVALID, "gffx_hip_classmap_perm_begin: seq_len is NULL");
    if (n_perm > enrich::kMaxPerms) return fail(GFFX_E_INVALID, "gffx_hip_classmap_perm_begin: %u permutations (at most %u are possible)", n_perm, enrich::kMaxPerms);
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));  // (no run adds to the totals that go away next)
    classmap_perm_drop(H);
    H->n_perm = n_perm, H->perm_seed = seed;
    H->perm_launch_blocks = kPermMaxBlocks;
    if (const char *e = std::getenv("GFFX_HIP_PERM_LAUNCH_BLOCKS")) {
        const long long v = std::atoll(e);
        if (v >= 1 && (uint64_t)v <= kPermMaxBlocks) H->perm_launch_blocks = (uint64_t)v;
    }
    const uint64_t words = 2 * perm_cells(H) + 1;
    GFFX_KEEP_TRY(H, dev_alloc_padded(&H->perm_totals, words));
    GFFX_KEEP_TRY(H, dev_alloc_padded(&H->perm_len, H->n_seq));
    GFFX_KEEP_TRY(H, dev_alloc_padded(&H->perm_ctl, 2));
    GFFX_KEEP_HIP(H, hipMemsetAsync(H->perm_totals, 0, words * 8, H->stream));
    GFFX_KEEP_HIP(H, hipMemsetAsync(H->perm_ctl, 0, 8, H->stream));
    if (H->n_seq) GFFX_KEEP_HIP(H, hipMemcpyAsync(H->perm_len, seq_len, (size_t)H->n_seq * 4, hipMemcpyHostToDevice, H->stream));
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));  // (the caller's lengths are free)
    H->perm_open = H->perm_waited = true;
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_perm_run_host(gffx_hip_classmap *H, const uint32_t *regions, uint64_t nq, uint64_t first_row) {
    const int rc = perm_ready(H, "gffx_hip_classmap_perm_run_host");
    if (rc) return rc;
    if (nq && !regions) return fail(GFFX_E_INVALID, "gffx_hip_classmap_perm_run_host: regions is NULL");
    if (nq) {
        // (growing frees the old array, which waits for the device: an earlier run has read it by then)
        GFFX_KEEP_TRY(H, classmap_ensure(H->perm_regions, 3 * nq, "the regions"));
        GFFX_KEEP_HIP(H, hipMemcpyAsync(H->perm_regions.p, regions, nq * 12, hipMemcpyHostToDevice, H->stream));
        GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));  // (the caller's array is free; the kernels below are not waited for)
    }
    return perm_run(H, H->perm_regions.p, nq, first_row);
}

extern "C" int gffx_hip_classmap_perm_run_store(gffx_hip_classmap *H, const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows, uint64_t first_row) {
    const int rc = perm_ready(H, "gffx_hip_classmap_perm_run_store");
    if (rc) return rc;
    const uint32_t *rows = nullptr;
    if (const int bad = store_slot_rows(R, k, first, n_rows, H->device, "gffx_hip_classmap_perm_run_store", "class map", &rows)) return bad;
    if (R->pending[k]) GFFX_KEEP_HIP(H, hipStreamWaitEvent(H->stream, R->copied[k], 0));
    return perm_run(H, rows, n_rows, first_row);  // (the slot is read in place: _perm_wait before it is appended to again)
}

extern "C" int gffx_hip_classmap_perm_wait(gffx_hip_classmap *H) {
    const int rc = perm_ready(H, "gffx_hip_classmap_perm_wait");
    if (rc) return rc;
    if (H->perm_waited) return GFFX_OK;
    uint32_t ctl[2] = {0, 0};
    GFFX_KEEP_HIP(H, hipMemcpyAsync(ctl, H->perm_ctl, 8, hipMemcpyDeviceToHost, H->stream));
    GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));
    H->perm_kernel_ms = 0;
    for (auto &pr : H->perm_ev) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) H->perm_kernel_ms += ms;
        H->perm_ev_free.push_back(pr.first), H->perm_ev_free.push_back(pr.second);
    }
    H->perm_ev.clear();
    H->perm_waited = true;
    if (ctl[1]) {
        GFFX_KEEP_HIP(H, hipMemsetAsync(H->perm_ctl, 0, 8, H->stream));
        GFFX_KEEP_HIP(H, hipStreamSynchronize(H->stream));
        // (the runs with such a row added nothing; the others stand, and the object stays usable)
        return fail(GFFX_E_CHR_RANGE, "gffx_hip_classmap_perm_wait: a region has chr >= %u: its run is void", H->n_seq);
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_perm_copy_totals(gffx_hip_classmap *H, uint64_t *bases, uint64_t *regions, uint64_t *unplaced) {
    const int rc = perm_ready(H, "gffx_hip_classmap_perm_copy_totals");
    if (rc) return rc;
    if (!H->perm_waited) return fail(GFFX_E_STATE, "gffx_hip_classmap_perm_copy_totals: call gffx_hip_classmap_perm_wait first");
    const uint64_t cells = perm_cells(H);
    if (bases) GFFX_KEEP_HIP(H, hipMemcpy(bases, H->perm_totals, cells * 8, hipMemcpyDeviceToHost));
    if (regions) GFFX_KEEP_HIP(H, hipMemcpy(regions, H->perm_totals + cells, cells * 8, hipMemcpyDeviceToHost));
    if (unplaced) GFFX_KEEP_HIP(H, hipMemcpy(unplaced, H->perm_totals + 2 * cells, 8, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_classmap_perm_last_kernel_ms(gffx_hip_classmap *H, double *ms) {
    const int rc = perm_ready(H, "gffx_hip_classmap_perm_last_kernel_ms");
    if (rc) return rc;
    if (!H->perm_waited) return fail(GFFX_E_STATE, "gffx_hip_classmap_perm_last_kernel_ms: call gffx_hip_classmap_perm_wait first");
    if (!ms) return fail(GFFX_E_INVALID, "gffx_hip_classmap_perm_last_kernel_ms: ms is NULL");
    *ms = H->perm_kernel_ms;
    return GFFX_OK;
}
