// closest_core.hpp -- the rule of `gffx closest` for the host (g++) and the device (hipcc): the roots of a seqid that lie nearest
// to a region, and how far away.
//
// Coordinates are 0-based and half-open.  A root [fs, fe) with fe >= fs (the index domain) falls into exactly ONE class with
// respect to a region [qs, qe), qs < qe:
//      OVER    fs < qe && fe > qs      gap 0
//      LEFT    fe <= qs                gap qs - fe + 1
//      RIGHT   fs >= qe                gap fs - qe + 1
// (LEFT and RIGHT exclude each other: fe <= qs < qe <= fs contradicts fe >= fs; a root that is neither has fe > qs and fs < qe.)
// Adjacent intervals have gap 1, as in bedtools.  The gap fits 32 bits: a LEFT root has fe >= 0 and qs <= 2^32 - 2, a RIGHT
// root fs <= 2^32 - 1 and qe >= 1.  The flags restrict the candidates: IGNORE_OVERLAPS removes OVER, LEFT_ONLY removes RIGHT,
// RIGHT_ONLY removes LEFT.  The answer is every candidate of minimal gap in ascending index position.
//
// What the searches work on: the seqid's roots at positions [first, last) sorted stably by start, and the END TABLE of the same
// slice -- e_end[] ascending, e_pos[] the position each end came from, equal ends in ascending position.  With
//      p = #{start < qe}  (a position)          every root at or behind p is RIGHT, none before p is
//      j = #{end <= qs}   (an end-table index)  the entries before j are exactly the LEFT roots
// the nearest RIGHT roots are the run of equal starts at p, the nearest LEFT roots the run of equal ends before j.  j follows from
// p and the number of overlapping roots (nearest, below): the end table is indexed, never searched.  A LEFT root
// starts at or before its end <= qs < qe <= the start of any RIGHT root, so every LEFT position is below every RIGHT one: the
// LEFT run in end-table order followed by the RIGHT run IS ascending position.
//
// Plain C++17 on flat pointers and accessors (GFFX_HD inline, no allocation, no HIP calls): the same code runs in
// k_closest_count / k_closest_emit (closest.hip) and in the sanitizer build of tools/closest_check.cpp.  Every loop and every
// read is bounded by the slice [first, last) handed in; the region's own numbers never index anything.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace closest {

// (the values of enum gffx_closest_flags, include/gffx_hip.h)
constexpr uint32_t kIgnoreOverlaps = 1u, kLeftOnly = 2u, kRightOnly = 4u;

enum Class : uint32_t { kOver = 0, kLeft = 1, kRight = 2 };

// both _ONLY bits together, or an unknown bit: refused
GFFX_HD inline bool flags_ok(uint32_t flags) {
    return (flags & ~(kIgnoreOverlaps | kLeftOnly | kRightOnly)) == 0u && (flags & (kLeftOnly | kRightOnly)) != (kLeftOnly | kRightOnly);
}

// class of the root [fs, fe), fe >= fs, for the region [qs, qe), qs < qe
GFFX_HD inline Class class_of(uint32_t fs, uint32_t fe, uint32_t qs, uint32_t qe) {
    if (fs < qe && fe > qs) return kOver;
    return fe <= qs ? kLeft : kRight;
}

// gap of a root of the given class (no overflow: the header comment)
GFFX_HD inline uint32_t gap_of(Class c, uint32_t fs, uint32_t fe, uint32_t qs, uint32_t qe) {
    return c == kOver ? 0u : c == kLeft ? qs - fe + 1u : fs - qe + 1u;
}

// is a root of class c a candidate under the flags?
GFFX_HD inline bool candidate(Class c, uint32_t flags) {
    return c == kOver ? !(flags & kIgnoreOverlaps) : c == kLeft ? !(flags & kRightOnly) : !(flags & kLeftOnly);
}

// signed distance of an answered root: -gap for LEFT, +gap for RIGHT, 0 for OVER
GFFX_HD inline long long signed_distance(uint32_t fs, uint32_t fe, uint32_t qs, uint32_t qe, uint32_t gap) {
    const Class c = class_of(fs, fe, qs, qe);
    return c == kOver ? 0ll : c == kLeft ? -(long long)gap : (long long)gap;
}

// the first index i of [lo, hi) with key(i) >= x, hi if none (lo <= hi; key is read inside [lo, hi) only)
template <typename KEY>
GFFX_HD inline uint32_t first_ge(uint32_t lo, uint32_t hi, uint32_t x, KEY &&key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key(mid) < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the first index i of [lo, hi) with key(i) > x, hi if none: i - lo = the keys of the slice that are <= x
template <typename KEY>
GFFX_HD inline uint32_t first_gt(uint32_t lo, uint32_t hi, uint32_t x, KEY &&key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key(mid) <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// tie walks: the run of keys equal to key(i) that ends at i (walks down, never below lo) / that starts at i (up, never to hi)
template <typename KEY>
GFFX_HD inline uint32_t run_begin(uint32_t lo, uint32_t i, KEY &&key) {
    const uint32_t v = key(i);
    while (i > lo && key(i - 1) == v) --i;
    return i;
}
template <typename KEY>
GFFX_HD inline uint32_t run_end(uint32_t i, uint32_t hi, KEY &&key) {
    const uint32_t v = key(i);
    ++i;
    while (i < hi && key(i) == v) ++i;
    return i;
}

// The answer of a region that is NOT answered by its overlaps (there are none, or IGNORE_OVERLAPS): the LEFT run
// [l0, l1) of END-TABLE indices, then the RIGHT run [r0, r1) of POSITIONS, all at distance `gap`; both empty: no answer.
struct Nearest {
    uint32_t l0, l1, r0, r1, gap;
    GFFX_HD uint32_t count() const { return (l1 - l0) + (r1 - r0); }
};

// first <= p <= last, p = #{start < qe} as a position; qs < qe; flags_ok(flags).
// n_over: how many roots of the slice overlap the region.  j = #{end <= qs} then needs no search: a root that ends at or before qs
// starts at or before its end, below qe, so it sits before p; and the roots before p that do NOT end at or before qs are exactly
// the overlapping ones (start < qe, end > qs).  Hence j = p - n_over, as an end-table index of the same slice.
template <typename START, typename EEND>
GFFX_HD inline Nearest nearest(uint32_t first, uint32_t last, uint32_t p, uint32_t n_over, uint32_t qs, uint32_t qe, uint32_t flags,
                               START &&start_at, EEND &&e_end_at) {
    Nearest a{first, first, p, p, 0u};
    bool right = false, left = false;
    uint32_t gr = 0, gl = 0;
    if (!(flags & kLeftOnly) && p < last) {
        right = true;
        gr = start_at(p) - qe + 1u;  // start[p] >= qe
    }
    if (!(flags & kRightOnly)) {
        const uint32_t j = p - first >= n_over ? p - n_over : first;  // (clamped: whatever n_over is, j stays inside [first, p])
        // (the test of the end holds in the index domain fe >= fs; outside it, it keeps the gap from wrapping)
        if (j > first && e_end_at(j - 1u) <= qs) {
            left = true;
            gl = qs - e_end_at(j - 1u) + 1u;
            a.l1 = j;
        }
    }
    if (left && right) {
        if (gl < gr)
            right = false;
        else if (gr < gl)
            left = false;
    }
    if (left) {
        a.l0 = run_begin(first, a.l1 - 1u, e_end_at);
        a.gap = gl;
    } else {
        a.l1 = a.l0;
    }
    if (right) {
        a.r1 = run_end(p, last, start_at);
        a.gap = gr;
    }
    return a;
}

}  // namespace closest
}  // namespace gffx
