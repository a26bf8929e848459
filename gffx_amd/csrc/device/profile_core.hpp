// profile_core.hpp -- the rules of the per-base depth profile (`gffx coverage --thresholds / --bedgraph`) for the
// host (g++) and the device (hipcc).  For the rows [s, e) of a seqid, depth(x) = #{rows with s <= x < e}.  The CANONICAL
// profile of a seqid is the list of points (pos_i, d_i), pos strictly ascending, d_i the depth on [pos_i, pos_{i+1}),
// d_i != d_{i-1} (d_{-1} = 0), the last depth 0; a seqid without rows has no points.
// A row is two events (s, +1) and (e, -1), a point (pos_i, d_i) of an earlier profile one event (pos_i, d_i - d_{i-1}).  With
// the events sorted by (seqid, position), the depth behind a position is the sum of the deltas of all events up to the last
// one at that position -- the TAIL of its run of equal keys --, and the position is a point iff that depth differs from the
// depth behind the previous tail.  A seqid's deltas add up to zero, so the sum needs no restart at a seqid border.
// Deltas and depths are uint32_t in two's complement: a true depth lies in 0 .. 2^32 - 1 (a profile holds at most 2^32 - 1
// rows), sums inside a run may wrap, and the sum at a tail is the true depth modulo 2^32, which is the true depth.
//
// Plain C++17 on flat pointers (GFFX_HD inline, no allocation, no HIP calls): the same code runs in the kernels of
// profile.hip and in the sanitizer build of tools/profile_check.cpp.  Every read is bounded by the range handed in.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace profile {

typedef unsigned long long u64;

GFFX_HD inline u64 event_key(uint32_t seqid, uint32_t pos) { return ((u64)seqid << 32) | pos; }

// the event with `key` is the tail of its run of equal keys: no event follows it, or the next one has another key
GFFX_HD inline bool is_tail(u64 key, bool has_next, u64 next_key) { return !has_next || next_key != key; }

// THE POINT RULE.  An event with `key`, the key behind it, the running depth before its run of equal keys (= the depth behind
// the previous tail, 0 before the first) and behind its run (the inclusive sum at the run's tail): is a point written here,
// and with which depth?
GFFX_HD inline bool point_here(u64 key, bool has_next, u64 next_key, uint32_t depth_before_run, uint32_t depth_after_run, uint32_t *depth) {
    *depth = depth_after_run;
    return is_tail(key, has_next, next_key) && depth_after_run != depth_before_run;
}

// THE THRESHOLD RULE over the points of a seqid.  d_prev: the depth of the point before (ignored at the seqid's first point)
GFFX_HD inline bool span_opens(uint32_t T, bool first, uint32_t d_prev, uint32_t d) { return d >= T && (first || d_prev < T); }
GFFX_HD inline bool span_closes(uint32_t T, bool first, uint32_t d_prev, uint32_t d) { return d < T && !first && d_prev >= T; }

// are (pos, d) and the point before it (same seqid unless `first`) a legal step of a canonical profile?  last: no point of
// the seqid follows
GFFX_HD inline bool canonical_step(bool first, uint32_t pos_prev, uint32_t d_prev, uint32_t pos, uint32_t d, bool last) {
    if (first ? d == 0u : (pos <= pos_prev || d == d_prev)) return false;
    return !last || d == 0u;
}

// depth at x from the points [lo, hi) of one seqid (pos ascending): one search for the last point with pos <= x
GFFX_HD inline uint32_t depth_at(const uint32_t *pos, const uint32_t *depth, u64 lo, u64 hi, uint32_t x) {
    u64 a = lo, b = hi;
    while (a < b) {  // first point with pos > x
        const u64 mid = a + ((b - a) >> 1);
        if (pos[mid] <= x)
            a = mid + 1;
        else
            b = mid;
    }
    return a == lo ? 0u : depth[a - 1];
}

}  // namespace profile
}  // namespace gffx
