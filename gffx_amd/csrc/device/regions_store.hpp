// regions_store.hpp -- device-resident store of BED regions filled chunk by chunk (include/gffx_hip.h "region stores").
#pragma once
#include <utility>

#include "gffx_device.hpp"

struct gffx_hip_regions {
    int device = 0;
    uint64_t cap_rows = 0, chunk_rows = 0, rows = 0;
    bool keep_all = false;
    uint32_t *d = nullptr;                        // AoS triples
    uint32_t *h_stage[2] = {nullptr, nullptr};    // pinned
    hipEvent_t copied[2] = {nullptr, nullptr};    // the last append from staging buffer k has completed
    bool pending[2] = {false, false};
    uint64_t last_first[2] = {0, 0}, last_n[2] = {0, 0};  // where the last append from buffer k went
    std::vector<std::pair<uint32_t, uint32_t>> last_sample[2];  // ... and {seqid, width} of ~4096 of its rows (AUTO's prior: judged against the
                                                                // index's per-seqid line widths when a batch takes the rows: the store knows no index)
    std::vector<uint64_t> last_sample_row[2];     // ... the row of the appended chunk every sampled entry is (a batch that takes a sub-range counts its own only)
    hipStream_t stream = nullptr;                 // copies
};

// Rows [first, first + n_rows) of the last append from staging buffer k, asked for by the entry point `who` of an object
// (`what`: "union", "class map", ...) that lives on `device`: *rows = where they lie in the store, or the call is refused.
// (The bound is written without first + n_rows, which wraps for a first near 2^64.)  The caller's stream still has to wait
// for copied[k] while pending[k].
inline int store_slot_rows(const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows, int device, const char *who, const char *what,
                           const uint32_t **rows) {
    if (!R || (k != 0 && k != 1)) return gffx::fail(GFFX_E_INVALID, "%s: bad argument", who);
    if (R->device != device) return gffx::fail(GFFX_E_INVALID, "%s: store and %s on different devices", who, what);
    if (first > R->last_n[k] || n_rows > R->last_n[k] - first) return gffx::fail(GFFX_E_INVALID, "%s: rows beyond the last append", who);
    *rows = R->d + 3 * (R->last_first[k] + first);
    return GFFX_OK;
}
