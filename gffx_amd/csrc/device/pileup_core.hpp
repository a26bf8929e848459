// pileup_core.hpp -- the rule of `gffx coverage --mean-depth` for the host (g++) and the device (hipcc): the bases that a
// multiset of rows [s, e) lays on a segment [a, b) of the same seqid,
//      bases(a, b) = sum over the rows of max(0, min(e, b) - max(s, a))          
// without an array over the bases.  With the rows' starts and ends each sorted on their own and
//      B(x) = sum over {s < x} of (x - s)  -  sum over {e < x} of (x - e)
// a row with s < e adds min(e, x) - s to B(x) when s < x and nothing otherwise, so bases(a, b) = B(b) - B(a) for a < b.
// The inequalities are strict: a row that only touches the segment (e == a or s == b) adds nothing, and among equal keys the
// searches count exactly the keys < x.  Each sum is (count * x - prefix sum of the counted keys): every counted key is < x, so
// a bracket is never negative, and one fold stays below 2^28 rows x 2^32 -- everything is unsigned 64-bit.
//
// Plain C++17 on flat pointers (GFFX_HD inline, no allocation, no HIP calls): the same code runs in k_pileup_segments
// (pileup.hip) and in the sanitizer build of tools/pileup_check.cpp.  Every read is bounded by the range handed in.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace pileup {

typedef unsigned long long u64;

// One fold's keys.  starts / ends: the rows' coordinates, each array sorted by (seqid, coordinate) on its own (starts and
// ends need not stay paired); pre_s / pre_e: n + 1 exclusive prefix sums of the array (pre[k] = sum of keys [0, k)).
struct Keys {
    const uint32_t *starts, *ends;
    const u64 *pre_s, *pre_e;
};

// the first position p of [lo, hi) with keys[p] >= x, hi if none: p - lo = the keys of the range that are < x
GFFX_HD inline u64 lower_bound(const uint32_t *keys, u64 lo, u64 hi, uint32_t x) {
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// B(x) from the two (count, prefix sum) pairs: n_s starts < x that add up to sum_s, n_e ends < x that add up to sum_e
GFFX_HD inline u64 bases_below(uint32_t x, u64 n_s, u64 sum_s, u64 n_e, u64 sum_e) { return (n_s * x - sum_s) - (n_e * x - sum_e); }

// B(x) over the seqid's keys [lo, hi); [from_s, hi) and [from_e, hi) are where the searches begin (positions found for a
// smaller x, or lo); *at_s / *at_e: the positions found
GFFX_HD inline u64 bases_below_at(const Keys &K, u64 lo, u64 hi, u64 from_s, u64 from_e, uint32_t x, u64 *at_s, u64 *at_e) {
    const u64 ps = lower_bound(K.starts, from_s, hi, x), pe = lower_bound(K.ends, from_e, hi, x);
    *at_s = ps, *at_e = pe;
    return bases_below(x, ps - lo, K.pre_s[ps] - K.pre_s[lo], pe - lo, K.pre_e[pe] - K.pre_e[lo]);
}

// the bases the rows of the seqid whose keys are [lo, hi) lay on [a, b): four searches (those of b start where those of a ended)
GFFX_HD inline u64 segment_bases(const Keys &K, u64 lo, u64 hi, uint32_t a, uint32_t b) {
    if (a >= b || lo >= hi) return 0ull;
    u64 ps, pe, qs, qe;
    const u64 below_a = bases_below_at(K, lo, hi, lo, lo, a, &ps, &pe);
    return bases_below_at(K, lo, hi, ps, pe, b, &qs, &qe) - below_a;
}

}  // namespace pileup
}  // namespace gffx
