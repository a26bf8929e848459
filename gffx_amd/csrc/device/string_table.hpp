// string_table.hpp -- the device side of ids_core.hpp's string table: one thread's insert of a string, the launchers of the
// two kernels that build a table (string_table.hip) and the table of a handle that uploads its strings.  Shared by the ID
// table of `gffx extract` (ids.hip), the value and wanted tables of `gffx search` (search.hip) and the finish steps of
// `gffx index --gpu` (gff.hip: its tables stand over arenas it owns, so it calls the launchers).
#pragma once
#include "gffx_device.hpp"
#include "ids_core.hpp"

namespace gffx {
namespace ids {

enum class Keep { kLargest, kSmallest };  // which of the rows that share a string a slot's value ends as

constexpr uint32_t fill_value(Keep k) { return k == Keep::kLargest ? 0u : kNone; }

// string f = bytes[off[f], off[f + 1]) enters the table: an empty slot is claimed with ONE 64-bit compare-and-swap of
// (hash << 32) | f -- whoever wins, the slot's name is that thread's string from then on --; a slot whose hash and string
// equal the thread's takes atomicMax(val, f) or atomicMin(val, f).  So val (filled with fill_value(K)) ends as the largest or
// the smallest f of the string whatever the order the threads ran in, and since names only enter the table a lookup finds
// every name whatever slot of its chain it got.
template <Keep K>
__device__ inline void table_settle(uint32_t *v, uint32_t f) {
    if (K == Keep::kLargest)
        atomicMax(v, f);
    else
        atomicMin(v, f);
}

template <Keep K>
__device__ inline void table_insert_one(u64 *slot, uint32_t *val, const uint8_t *bytes, const u64 *off, uint32_t f, uint32_t mask,
                                        uint32_t hash_mask) {
    const u64 a = off[f], len = off[f + 1] - a;
    const uint32_t h = name_hash(bytes + a, len) & hash_mask;
    const u64 mine = ((u64)h << 32) | f;
    for (uint32_t i = h & mask, steps = 0; steps <= mask; i = (i + 1) & mask, ++steps) {  // (<= n slots are ever taken: it ends)
        u64 w = slot[i];
        if (w == kEmptyWord) {
            w = atomicCAS(&slot[i], kEmptyWord, mine);
            if (w == kEmptyWord) return table_settle<K>(&val[i], f);
        }
        if ((uint32_t)(w >> 32) != h) continue;
        const uint32_t rep = (uint32_t)w;
        const u64 ra = off[rep];
        if (off[rep + 1] - ra == len && name_equal(bytes + ra, bytes + a, len)) return table_settle<K>(&val[i], f);
    }
}

// k_table_fill on stream s, one thread per slot: every slot empty, every value fill_value(keep)
void launch_table_fill(hipStream_t s, u64 *slot, uint32_t *val, uint32_t slots, Keep keep);
// k_table_fill and k_table_insert (one thread per string, Keep::kLargest) on stream s: the table of strings [0, n)
void launch_table_build(hipStream_t s, u64 *slot, uint32_t *val, uint32_t slots, const uint8_t *bytes, const u64 *off, uint32_t n,
                        uint32_t hash_mask);

// the table of a handle over strings the caller gives: it owns the slots and a copy of the strings
struct StringTable {
    DevArr<u64> slot, off;
    DevArr<uint32_t> val;
    DevArr<uint8_t> bytes;
    uint32_t mask = 0, hash_mask = 0xFFFFFFFFu;

    // strings [0, n) = host_bytes[host_off[f], host_off[f + 1]) (ascending from 0: check_offsets) to the device and into a
    // table of table_slots(n) slots, whatever the arrays held or could hold before; `start`, unless NULL, is recorded between
    // the copies and the two kernels.  The caller's arrays are read when s has been synchronised.
    int build(hipStream_t s, uint64_t n, const uint8_t *host_bytes, const uint64_t *host_off, uint32_t hash_mask_, hipEvent_t start) {
        const uint32_t slots = table_slots(n);
        const uint64_t n_bytes = n ? host_off[n] : 0;
        mask = slots - 1;
        hash_mask = hash_mask_;
        GFFX_HIP_TRY(slot.ensure(slots));
        GFFX_HIP_TRY(val.ensure(slots));
        GFFX_HIP_TRY(bytes.ensure(n_bytes + kPad));
        GFFX_HIP_TRY(off.ensure(n + 1));
        GFFX_HIP_TRY(hipMemsetAsync(bytes.p + n_bytes, 0, kPad, s));
        if (n_bytes) GFFX_HIP_TRY(hipMemcpyAsync(bytes.p, host_bytes, n_bytes, hipMemcpyHostToDevice, s));
        if (n) {
            GFFX_HIP_TRY(hipMemcpyAsync(off.p, host_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
        } else {
            GFFX_HIP_TRY(hipMemsetAsync(off.p, 0, 8, s));
        }
        if (start) GFFX_HIP_TRY(hipEventRecord(start, s));
        launch_table_build(s, slot.p, val.p, slots, bytes.p, off.p, (uint32_t)n, hash_mask);
        return GFFX_OK;
    }
    Table table() const { return Table{slot.p, val.p, bytes.p, off.p, mask, hash_mask}; }
};

}  // namespace ids
}  // namespace gffx
