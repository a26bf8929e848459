// search_core.hpp -- the rules of `gffx search` that the host (g++) and the device (hipcc) share: one step and the match
// loop of the DFA that host/regex_dfa.cpp compiles, the (value class, root) pair set, and the test of one line of a hit
// block (reference: commands/search.rs:55-252, utils/common.rs:289-465; file:line relative to the reference's src/).  The
// hash, the string compare, the table lookup, the bounded parent chase and the slices of a GFF line are ids_core.hpp's.
//
// As there: plain C++17 on flat pointers, no allocation, no HIP calls; the same code runs in the kernels of search.hip and
// in the sanitizer build of tools/search_check.cpp.  Every read is bounded by the value's or the line's length and every
// state index by the table; nothing asserts, aborts or traps on a condition the input decides.
//
// The keep set as integers.  The reference hands write_gff_output_filtered, per root r, the set of matched value STRINGS
// that some fid with root r carries (search.rs:209-218), and keeps a line of block r iff the bytes after the first
// `<name>=` in column 9 are in that set.  Here every distinct `.atn` string is a value class -- the LARGEST aid that holds
// the string, which is what ids::table_find returns from a table built over `.atn` -- and the device keeps a set of
// (class, root) pairs: one per matched fid with a valid root.  A line's value X is in the reference's set of r iff X is a
// string of `.atn` and (class(X), r) is in the pair set: exact also where `.atn` repeats a string, since the string, not
// the aid, keys both.
#pragma once
#include <cstdint>

#include "ids_core.hpp"

namespace gffx {
namespace search {

using ids::u64;

constexpr uint32_t kAccept = 0;  // the DFA's accepting state: absorbing

struct Dfa {
    const uint8_t *cls;     // 256: byte -> column
    const uint16_t *trans;  // n_states x n_classes; the last column is the end of the text
    uint32_t n_states, n_classes, init;
};

// one transition; a state or a column the table does not have (never from a table of regex_dfa.cpp) ends in the start state
GFFX_HD inline uint32_t dfa_step(const Dfa &d, uint32_t s, uint32_t col) {
    if (s >= d.n_states || col >= d.n_classes) return d.init < d.n_states ? d.init : kAccept;
    return d.trans[(u64)s * d.n_classes + col];
}

// is_match: the bytes, then the end-of-text symbol; the accepting state is absorbing, so the walk ends where it is reached
GFFX_HD inline bool dfa_match(const Dfa &d, const uint8_t *p, u64 n) {
    if (d.n_states == 0 || d.n_classes == 0) return false;
    uint32_t s = d.init;
    if (s == kAccept) return true;
    for (u64 i = 0; i < n; ++i) {
        s = dfa_step(d, s, d.cls[p[i]]);
        if (s == kAccept) return true;
    }
    return dfa_step(d, s, d.n_classes - 1) == kAccept;
}

// ---- the (class, root) pair set: open addressing, linear probing, one 64-bit word per slot, kEmptyWord = empty ----------
GFFX_HD inline u64 pair_word(uint32_t cls, uint32_t root) { return ((u64)cls << 32) | root; }
GFFX_HD inline uint32_t pair_hash(u64 w) {
    w ^= w >> 33;
    w *= 0xff51afd7ed558ccdull;
    w ^= w >> 33;
    return (uint32_t)w;
}
GFFX_HD inline bool pair_find(const u64 *slot, uint32_t mask, uint32_t cls, uint32_t root) {
    const u64 w = pair_word(cls, root);
    for (uint32_t i = pair_hash(w) & mask, steps = 0; steps <= mask; i = (i + 1) & mask, ++steps) {
        const u64 x = slot[i];
        if (x == w) return true;
        if (x == ids::kEmptyWord) return false;
    }
    return false;
}

// write_gff_output_filtered's test of one line (common.rs:418-431) for `gffx search`: line[0, len) (with its line ending)
// lies in the block of `root`; kept iff it is no '#' line, passes -T, and the value after the first `<key>=` behind the
// eighth TAB is a string of the value table whose class forms a pair with root.  (The reference also wants the value and
// the type to be valid UTF-8: the table's strings and the -T strings are, and other bytes cannot compare equal to them.)
GFFX_HD inline bool keep_line_value(const ids::Table &values, const u64 *pairs, uint32_t pair_mask, const ids::Types &types,
                                    const uint8_t *key, uint32_t key_len, const uint8_t *line, u64 len, uint32_t root) {
    if (len && line[0] == '#') return false;
    const u64 n = ids::body_len(line, len);
    u64 a = 0, z = 0;
    if (types.on) {
        if (!ids::type_slice(line, n, &a, &z)) return false;
        if (!ids::type_allowed(types, line + a, z - a)) return false;
    }
    if (!ids::attr_value_slice(line, n, key, key_len, &a, &z)) return false;
    const uint32_t c = ids::table_find(values, line + a, z - a);
    if (c == ids::kNone || root == ids::kNone) return false;
    return pair_find(pairs, pair_mask, c, root);
}

}  // namespace search
}  // namespace gffx
