// enrich_core.hpp -- the rules of `gffx enrich` for the host (g++) and the device (hipcc): a permutation test of
// regions against the classes of a finished class map (classmap_core.hpp).
// Every region (c, qs, qe) has a global row i (its place in the input), every seqid a length L[c].  Row 0 of the totals is the
// observed data, row p = 1 .. N the p-th permutation: every region is moved to a random start on its own seqid,
//   r(p, i) = mix64(key(p) + GOLD * (i + 1)),  key(p) = mix64(seed + GOLD * p)     (mod 2^64; mix64: the splitmix64 finalizer)
//   w = qe - qs,  span = L[c] - w + 1,  s' = (r(p, i) * span) >> 64  (the high half of the 128-bit product),  [s', s' + w)
// A region with qs >= qe is EMPTY (class T, no bases, in every row); one with w > L[c] is UNPLACEABLE and stays where it is.
// s' is not exactly uniform: a start is drawn with probability floor or ceil of 2^64 / span over 2^64, a relative bias of at
// most span / 2^64 <= 2^-32.  It is documented, not corrected (no rejection loop: one draw per placement, whatever the span).
// B[p][k] = the sum of bases_k over the placed regions (64 bits), R[p][k] = the regions whose class is k, k = 0 .. T.  They are
// integer sums: any split of the regions into runs and any launch shape give the same matrices.
//
// Plain C++17 on flat pointers (GFFX_HD inline, no allocation, no HIP calls), like classmap_core.hpp: the same code runs in
// k_classmap_permute (enrich.hip) and in tools/enrich_check.cpp.
#pragma once
#include <cstdint>

#include "classmap_core.hpp"

namespace gffx {
namespace enrich {

typedef unsigned long long u64;

constexpr u64 kGold = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kMaxPerms = 1u << 20;

GFFX_HD inline u64 mix64(u64 z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

GFFX_HD inline u64 perm_key(u64 seed, uint32_t p) { return mix64(seed + kGold * p); }

GFFX_HD inline u64 perm_draw(u64 key, u64 row) { return mix64(key + kGold * (row + 1)); }

// the high 64 bits of a * b
GFFX_HD inline u64 mul_hi(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

enum Placement { kEmpty = 0, kUnplaceable = 1, kPlaced = 2 };

// THE PLACEMENT RULE.  *start = where the region [qs, qe) begins under `draw` on a seqid of length L (qs itself when it is not
// placed); its width stays.  span <= 2^32, so s' + w <= L fits 32 bits
GFFX_HD inline Placement place(u64 draw, uint32_t L, uint32_t qs, uint32_t qe, uint32_t *start) {
    *start = qs;
    if (qs >= qe) return kEmpty;
    const uint32_t w = qe - qs;
    if (w > L) return kUnplaceable;
    *start = (uint32_t)mul_hi(draw, (u64)(L - w) + 1);
    return kPlaced;
}

// One region in one row of the totals: row 0 (`observed`) takes it where it stands, a permutation where `draw` puts it.
// add_bases(k, n) for every class with n > 0 bases, add_class(k) once.  Returns how the region was placed (row 0: as a
// permutation would)
template <typename AddBases, typename AddClass>
GFFX_HD inline Placement region_in_row(const uint32_t *pos, const uint8_t *cls, const u64 *cb, uint32_t T, u64 lo, u64 hi, uint32_t L, uint32_t qs, uint32_t qe,
                                       bool observed, u64 draw, AddBases &&add_bases, AddClass &&add_class) {
    uint32_t s;
    const Placement how = place(draw, L, qs, qe, &s);
    if (observed) s = qs;
    const uint32_t e = how == kEmpty ? s : s + (qe - qs);
    add_class(classmap::region_bases_each(pos, cls, cb, T, lo, hi, s, e, [&](uint32_t k, uint32_t n) {
        if (n) add_bases(k, n);
    }));
    return how;
}

}  // namespace enrich
}  // namespace gffx
