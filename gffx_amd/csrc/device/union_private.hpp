// union_private.hpp -- the union builder's object (include/gffx_hip.h "union builder"; coverage.hip builds and serves it).
// Shared with profile.hip, whose gffx_hip_profile_union_at_least writes the spans "depth >= T" straight into rec_a on the
// device and hands the object to gffx_hip_union_finish.
#pragma once
#include <string>
#include <vector>

#include "gffx_device.hpp"
#include "handle_status.hpp"
#include "radix_sort.hpp"

struct gffx_hip_union : gffx::HandleStatus {
    static constexpr const char *kName = "union", *kNoun = "union";
    uint32_t n_seq = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t *rec_a = nullptr, *rec_b = nullptr;  // rec_a[0 .. n_spans) = the spans so far as {seqid, start, end} records
    uint64_t cap = 0, n_spans = 0;
    uint32_t *work = nullptr;
    uint64_t cap_work = 0;
    unsigned long long *tile_a = nullptr, *tile_b = nullptr;
    uint64_t cap_tiles = 0;
    uint32_t *ctl = nullptr;  // device words {err x 4, span count (64 bits), pad}
    uint32_t *h_stage = nullptr;  // pinned
    uint64_t cap_stage = 0;
    gffx::SortPlan plan{};
    double kernel_ms = 0.0;
    uint64_t rows_added = 0, folds = 0;
    // after _finish
    bool finished = false;
    std::vector<unsigned long long> u_off, pb;
    std::vector<uint32_t> us, ue;
    void *tables[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint32_t *d_seg[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t cap_seg = 0;
};
