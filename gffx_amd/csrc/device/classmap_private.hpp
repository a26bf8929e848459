// classmap_private.hpp -- the class map object behind gffx_hip_classmap_* and what its two translation units share:
// classmap.hip (the build and `gffx annotate`'s per-region answers) and enrich.hip (the permutation totals of
// `gffx enrich`).  Not part of the C-ABI.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "gffx_device.hpp"
#include "handle_status.hpp"

struct gffx_hip_union;  // (union_private.hpp)

namespace gffx {

constexpr int kClassThreads = 256;
constexpr uint32_t kClassErrRange = 1u;  // a region with chr >= n_seq

struct ClassMapView {
    const u64 *p_off;  // n_seq + 1
    const uint32_t *p_pos;
    const uint8_t *p_cls;
    const u64 *cb;
    uint32_t n_seq, T;
};

}  // namespace gffx

struct gffx_hip_classmap : gffx::HandleStatus {
    static constexpr const char *kName = "classmap", *kNoun = "object";
    uint32_t n_seq = 0, T = 0;
    hipStream_t stream = nullptr;
    // _finish: 0 .. 1 toggles, 1 .. 2 sort, 2 .. 3 scan, 3 .. 4 count, 5 .. 6 emit + offsets, 6 .. 7 bases; a run: 8 .. 9
    hipEvent_t ev[10] = {};
    gffx_hip_union *U = nullptr;  // one union per (layer, seqid) under pseudo-seqids
    std::vector<uint32_t> pseudo;  // _add_rows_host: the rows as the union takes them
    bool finished = false;
    uint64_t n_points = 0;
    uint32_t *p_seq = nullptr, *p_pos = nullptr;
    uint8_t *p_cls = nullptr;
    gffx::u64 *cb = nullptr, *p_off = nullptr;
    uint32_t *ctl = nullptr;  // device words {err, 3 x pad, count (64 bits), 2 x pad}
    gffx::DevArr<uint32_t> d_regions, d_counts;
    gffx::DevArr<uint8_t> d_class;
    uint64_t nq = 0;
    bool ran = false, waited = false;
    double kernel_ms = 0;
    double stage_ms[6] = {0, 0, 0, 0, 0, 0};  // union, toggles, sort, scan, points, bases
    // ---- the permutation totals (enrich.hip); nothing of it is touched by the entry points of classmap.hip but _destroy and
    // _finish, which drop it: a new map needs a new _perm_begin
    bool perm_open = false;
    uint32_t n_perm = 0;
    uint64_t perm_seed = 0;
    uint64_t perm_launch_blocks = 0;     // blocks of k_classmap_permute per launch (_perm_begin sets it)
    gffx::u64 *perm_totals = nullptr;    // bases [(n_perm + 1) x (T + 1)], regions [the same], unplaced [1]
    uint32_t *perm_len = nullptr;        // n_seq
    uint32_t *perm_ctl = nullptr;        // device words {this run has a bad row, a run since the last _perm_wait had one}
    gffx::DevArr<uint32_t> perm_regions;  // _perm_run_host's copy of the rows (its own: `annotate`'s rows stay where they are)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> perm_ev;  // around the launches of every run since the last _perm_wait
    std::vector<hipEvent_t> perm_ev_free;
    double perm_kernel_ms = 0;
    bool perm_waited = false;
};

namespace gffx {

inline int classmap_ready(gffx_hip_classmap *H, const char *who) {
    const int rc = enter_handle(H, who);
    if (rc) return rc;
    if (!H->finished) return fail(GFFX_E_STATE, "%s: call gffx_hip_classmap_finish first", who);
    return GFFX_OK;
}

template <typename X>
int classmap_ensure(DevArr<X> &a, uint64_t n, const char *what) {
    const hipError_t e = a.ensure((size_t)std::max<uint64_t>(n, 4));
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? GFFX_E_OOM : GFFX_E_HIP, "gffx_hip_classmap: no room for %s: %s", what, hipGetErrorString(e));
    return GFFX_OK;
}

inline uint32_t classmap_grid(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// the permutation totals go away (enrich.hip): the object's stream is idle when this is called
void classmap_perm_drop(gffx_hip_classmap *H);

}  // namespace gffx
