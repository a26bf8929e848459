// classmap_core.hpp -- the rules of `gffx annotate` for the host (g++) and the device (hipcc).
// T layers of intervals [s, e) per seqid, in priority order.  class(x) = the smallest k such that an interval of layer k
// covers base x, or T ("none").  The CLASS MAP of a seqid is the canonical list of points (pos_i, class_i): pos strictly
// ascending, class_i the class on [pos_i, pos_{i+1}), class_i != class_{i-1}, the first class not T, the last class T; a
// seqid without intervals has no points.
// Every layer is first made disjoint (one union per (layer, seqid)); a span {k, s, e} is then two TOGGLE events (s, 1 << k)
// and (e, 1 << k).  With the events sorted by (seqid, position), the mask of covering layers behind a position is the XOR of
// all toggles up to the last event at that position -- the TAIL of its run of equal keys --, and the position is a point iff
// the class of that mask differs from the class behind the previous tail.  A seqid's toggles XOR to zero (every span opens and
// closes its bit), so the scan needs no restart at a seqid border.
// cb[i * T + k] = the bases of class k on all points before point i (64 bits, over all seqids; differences are only taken
// inside one seqid).  F_k(x) = cb[j * T + k] + (class_j == k ? x - pos_j : 0) for the last point j of the seqid with
// pos_j <= x, and cb of the seqid's first point when x lies before it: the bases of class k on [0, x) plus those of the
// earlier seqids, a constant that drops out of bases_k = F_k(qe) - F_k(qs) of a region [qs, qe).
//
// Plain C++17 on flat pointers (GFFX_HD inline, no allocation, no HIP calls): the same code runs in the kernels of
// classmap.hip and in the host builds of tools/classmap_check.cpp (the sanitizer build and the timed one).  The command,
// host/annotate.cpp, goes through the C-ABI only.  Every read is bounded by the range handed in.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace classmap {

typedef unsigned long long u64;

constexpr uint32_t kMaxLayers = 32;

// the class of a mask of covering layers: its lowest set bit, or T for none
GFFX_HD inline uint32_t class_of_mask(uint32_t mask, uint32_t T) { return mask ? (uint32_t)__builtin_ctz(mask) : T; }

GFFX_HD inline u64 event_key(uint32_t seqid, uint32_t pos) { return ((u64)seqid << 32) | pos; }

// the event with `key` is the tail of its run of equal keys: no event follows it, or the next one has another key
GFFX_HD inline bool is_tail(u64 key, bool has_next, u64 next_key) { return !has_next || next_key != key; }

// THE POINT RULE.  An event with `key`, the key behind it, the mask before its run of equal keys (= behind the previous tail,
// 0 before the first) and behind its run (the inclusive XOR at the run's tail): is a point written here, and with which class?
GFFX_HD inline bool point_here(u64 key, bool has_next, u64 next_key, uint32_t mask_before_run, uint32_t mask_after_run, uint32_t T, uint32_t *cls) {
    *cls = class_of_mask(mask_after_run, T);
    return is_tail(key, has_next, next_key) && *cls != class_of_mask(mask_before_run, T);
}

// are (pos, cls) and the point before it (same seqid unless `first`) a legal step of a canonical class map?  last: no point
// of the seqid follows
GFFX_HD inline bool canonical_step(bool first, uint32_t pos_prev, uint32_t cls_prev, uint32_t pos, uint32_t cls, bool last, uint32_t T) {
    if (cls > T) return false;
    if (first ? cls == T : (pos <= pos_prev || cls == cls_prev)) return false;
    return !last || cls == T;
}

// the bases a point stands for: up to the next point of its seqid (the last point of a seqid has class T and stands for none)
GFFX_HD inline uint32_t point_len(uint32_t pos, bool next_in_seqid, uint32_t next_pos) { return next_in_seqid ? next_pos - pos : 0u; }

// THE BOUNDED SEARCH, twice side by side: *a = the first point of [lo, hi) with pos > x1, *b = the same for x2 (hi if there is
// none); the point before it, if it is >= lo, is the last one with pos <= x.  Both halve the same range in one loop, so the
// load of one does not wait for the load of the other; a search that has ended reads a point of the range once more
GFFX_HD inline void first_after_pair(const uint32_t *pos, u64 lo, u64 hi, uint32_t x1, uint32_t x2, u64 *a, u64 *b) {
    u64 a0 = lo, a1 = hi, b0 = lo, b1 = hi;
    while (a0 < a1 || b0 < b1) {  // (entered only with lo < hi: hi - 1 is a point of the range)
        const u64 ma = a0 + ((a1 - a0) >> 1), mb = b0 + ((b1 - b0) >> 1);
        const uint32_t pa = pos[ma < hi ? ma : hi - 1], pb = pos[mb < hi ? mb : hi - 1];
        if (a0 < a1) {
            if (pa <= x1)
                a0 = ma + 1;
            else
                a1 = ma;
        }
        if (b0 < b1) {
            if (pb <= x2)
                b0 = mb + 1;
            else
                b1 = mb;
        }
    }
    *a = a0, *b = b0;
}

// F_k(x) + the bases of class k on the seqids before this one, from a = the first point with pos > x.  The
// constant drops out of every difference inside the seqid; a seqid without points (lo == hi) reads nothing
GFFX_HD inline u64 bases_before(const uint32_t *pos, const uint8_t *cls, const u64 *cb, uint32_t T, u64 lo, u64 hi, u64 a, uint32_t x, uint32_t k) {
    if (lo == hi) return 0ull;
    if (a == lo) return cb[lo * T + k];  // (x lies before the first point)
    const u64 j = a - 1;
    return cb[j * T + k] + (cls[j] == k ? (u64)(x - pos[j]) : 0ull);
}

// THE REGION RULE over the points [lo, hi) of the region's seqid: each(k, bases_k) for every k = 0 .. T of a region with
// qs < qe (zeros included; k ascending), returns the region's class (the smallest k < T with bases_k > 0, or T).  qs >= qe calls
// nothing and returns T.  Two searches whatever T is.
template <typename Each>
GFFX_HD inline uint32_t region_bases_each(const uint32_t *pos, const uint8_t *cls, const u64 *cb, uint32_t T, u64 lo, u64 hi, uint32_t qs, uint32_t qe,
                                          Each &&each) {
    uint32_t best = T;
    if (qs >= qe) return best;
    u64 a, b;
    first_after_pair(pos, lo, hi, qs, qe, &a, &b);
    uint32_t rest = qe - qs;
    for (uint32_t k = 0; k < T; ++k) {
        const uint32_t n = (uint32_t)(bases_before(pos, cls, cb, T, lo, hi, b, qe, k) - bases_before(pos, cls, cb, T, lo, hi, a, qs, k));
        each(k, n);
        rest -= n;
        if (n && best == T) best = k;
    }
    each(T, rest);
    return best;
}

// ... with the counts in memory: out[0 .. T] = bases_k (qs >= qe gives zeros and T)
GFFX_HD inline uint32_t region_bases(const uint32_t *pos, const uint8_t *cls, const u64 *cb, uint32_t T, u64 lo, u64 hi, uint32_t qs, uint32_t qe,
                                     uint32_t *out) {
    if (qs >= qe)
        for (uint32_t k = 0; k <= T; ++k) out[k] = 0u;
    return region_bases_each(pos, cls, cb, T, lo, hi, qs, qe, [out](uint32_t k, uint32_t n) { out[k] = n; });
}

}  // namespace classmap
}  // namespace gffx
