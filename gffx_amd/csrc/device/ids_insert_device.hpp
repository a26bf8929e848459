// ids_insert_device.hpp -- the device side of ids_core.hpp's string table: one thread's clear of a slot and one thread's
// insert of a string (k_ids_insert's scheme, described in ids.hip).  Shared by the ID table of `gffx extract` (ids.hip) and
// the value tables of `gffx search` (search.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "ids_core.hpp"

namespace gffx {
namespace ids {

__device__ inline void table_clear_one(u64 *slot, uint32_t *val, uint32_t i) {
    slot[i] = kEmptyWord;
    val[i] = 0;
}

// string f = bytes[off[f], off[f + 1]) enters the table: an empty slot is claimed with ONE 64-bit compare-and-swap of
// (hash << 32) | f; a slot whose hash and string equal the thread's takes atomicMax(val, f)
__device__ inline void table_insert_one(u64 *slot, uint32_t *val, const uint8_t *bytes, const u64 *off, uint32_t f, uint32_t mask,
                                        uint32_t hash_mask) {
    const u64 a = off[f], len = off[f + 1] - a;
    const uint32_t h = name_hash(bytes + a, len) & hash_mask;
    const u64 mine = ((u64)h << 32) | f;
    for (uint32_t i = h & mask, steps = 0; steps <= mask; i = (i + 1) & mask, ++steps) {  // (<= n slots are ever taken: it ends)
        u64 w = slot[i];
        if (w == kEmptyWord) {
            w = atomicCAS(&slot[i], kEmptyWord, mine);
            if (w == kEmptyWord) {
                atomicMax(&val[i], f);
                return;
            }
        }
        if ((uint32_t)(w >> 32) != h) continue;
        const uint32_t rep = (uint32_t)w;
        const u64 ra = off[rep];
        if (off[rep + 1] - ra == len && name_equal(bytes + ra, bytes + a, len)) {
            atomicMax(&val[i], f);
            return;
        }
    }
}

}  // namespace ids
}  // namespace gffx
