// ids_core.hpp -- the rules of `gffx extract` that the host (g++) and the device (hipcc) share: the hash and the compare of a
// feature ID string, the lookup in the ID table, the bounded parent chase, the column-3 slice of a GFF line and the value
// after the first `<key>=` in its ninth column (reference: commands/extract.rs:37-162, index_loader/fts.rs:16-31,
// index_loader/prt.rs:54-72, utils/common.rs:289-465; file:line relative to the reference's src/).
//
// Everything in the first part is plain C++17 on flat pointers (GFFX_HD inline, no allocation, no HIP calls), so the same code
// runs in the kernels of ids.hip and in the sanitizer build of tools/extract_check.cpp.  The text is untrusted and the device
// must never fault on it: every read is bounded by the name's or the line's length, every loop by the line, the table or
// the number of parent words, and nothing asserts, aborts or traps on a condition the input decides.
//
// The table: open addressing, linear probing, a power of two >= 2 * n slots (so a probe always ends at an empty slot).  A
// slot is one 64-bit word, (hash << 32) | a representative fid whose string is the slot's name, and a 32-bit value, the
// LARGEST fid that has that string: fts.rs:16-22 inserts the lines in order, so the last `.fts` line of a string wins.
// Names only ever enter the table, so whatever the order in which they entered, a name sits on its probe chain with no
// empty slot before it and a lookup finds it: results do not depend on the insertion order.
//
// DEVIATION (prt.rs:54-72): a parent cycle that no root closes never ends in the reference's resolve_root.  chase_root ends
// after n steps (n = the number of parent words; a chain without a cycle has at most n nodes) and reports the fid as
// invalid, like an out-of-range child or parent.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace ids {

typedef unsigned long long u64;

constexpr uint32_t kNone = 0xFFFFFFFFu;            // a name that is not in the table; a fid without a valid root
constexpr u64 kEmptyWord = 0xFFFFFFFFFFFFFFFFull;  // an empty slot (a representative fid is < 2^32 - 1)
constexpr u64 kPad = 16;                           // bytes behind the last name / the text of a chunk

// FNV-1a (32 bit) of the name, as sam_core.hpp's
GFFX_HD inline uint32_t name_hash(const uint8_t *p, u64 n) {
    uint32_t h = 2166136261u;
    for (u64 i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// the low k bits of the hash (k >= 32: all of them).  k < 32 is a test hook: it forces names onto few probe chains.
GFFX_HD inline uint32_t hash_mask_of(int hash_bits) {
    return hash_bits < 0 || hash_bits >= 32 ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
}

// a[0, n) == b[0, n); eight bytes at a time, never a byte beyond n
GFFX_HD inline bool name_equal(const uint8_t *a, const uint8_t *b, u64 n) {
    u64 i = 0;
    for (; i + 8 <= n; i += 8) {
        u64 x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y) return false;
    }
    for (; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

struct Table {
    const u64 *slot;       // (hash << 32) | representative fid; kEmptyWord: empty
    const uint32_t *val;   // the largest fid with the slot's name
    const uint8_t *bytes;  // the names back to back
    const u64 *off;        // name f = bytes[off[f], off[f + 1])
    uint32_t mask;         // slots - 1
    uint32_t hash_mask;
};

GFFX_HD inline uint32_t table_slots(u64 n) {
    uint32_t slots = 2;
    while (slots < 2 * n) slots <<= 1;
    return slots;
}

// the fid of the LAST name equal to name[0, len) (fts.rs:16-31), or kNone
GFFX_HD inline uint32_t table_find(const Table &t, const uint8_t *name, u64 len) {
    const uint32_t h = name_hash(name, len) & t.hash_mask;
    for (uint32_t i = h & t.mask, steps = 0; steps <= t.mask; i = (i + 1) & t.mask, ++steps) {
        const u64 w = t.slot[i];
        if (w == kEmptyWord) return kNone;
        if ((uint32_t)(w >> 32) != h) continue;
        const uint32_t rep = (uint32_t)w;
        const u64 a = t.off[rep];
        if (t.off[rep + 1] - a != len) continue;
        if (name_equal(t.bytes + a, name, len)) return t.val[i];
    }
    return kNone;
}

// prt.rs:54-72 with the bound: the root of fid, or kNone (fid >= n, a parent >= n, or no root within n steps)
GFFX_HD inline uint32_t chase_root(const uint32_t *prt, uint32_t n, uint32_t fid) {
    uint32_t cur = fid;
    for (uint32_t steps = 0; steps < n; ++steps) {
        if (cur >= n) return kNone;
        const uint32_t p = prt[cur];
        if (p == cur) return cur;
        if (p >= n) return kNone;
        cur = p;
    }
    return kNone;  // n == 0, or a cycle
}

// common.rs:350-357: the line without its final '\n' and then without a '\r' before it
GFFX_HD inline u64 body_len(const uint8_t *line, u64 len) {
    if (len && line[len - 1] == '\n') --len;
    if (len && line[len - 1] == '\r') --len;
    return len;
}

// common.rs:364-377: column 3 = body[*a, *z); false: fewer than three TABs
GFFX_HD inline bool type_slice(const uint8_t *body, u64 len, u64 *a, u64 *z) {
    u64 p = 0, tab[3];
    for (int k = 0; k < 3; ++k) {
        while (p < len && body[p] != '\t') ++p;
        if (p >= len) return false;
        tab[k] = p++;
    }
    *a = tab[1] + 1;
    *z = tab[2];
    return true;
}

// common.rs:389-409: the attribute field is everything after the eighth TAB; the value starts after the FIRST occurrence of
// the bytes key[0, key_len) '=' in it (so `geneID=x;ID=y` yields x for the key ID) and ends at the next ';' or at the end of
// the body.  false: fewer than eight TABs, or no `<key>=`.
GFFX_HD inline bool attr_value_slice(const uint8_t *body, u64 len, const uint8_t *key, uint32_t key_len, u64 *a, u64 *z) {
    u64 p = 0;
    for (int tabs = 0; tabs < 8; ++tabs) {
        while (p < len && body[p] != '\t') ++p;
        if (p >= len) return false;
        ++p;
    }
    const u64 need = (u64)key_len + 1;
    for (; p + need <= len; ++p) {
        if (body[p + key_len] != '=') continue;
        uint32_t k = 0;
        while (k < key_len && body[p + k] == key[k]) ++k;
        if (k < key_len) continue;
        u64 e = p + need;
        *a = e;
        while (e < len && body[e] != ';') ++e;
        *z = e;
        return true;
    }
    return false;
}

struct Types {  // -T: the allowed column-3 strings (split at ',', trimmed, empty ones dropped: common.rs:306-311)
    const uint8_t *bytes;
    const uint32_t *off;  // type k = bytes[off[k], off[k + 1])
    uint32_t n;
    int on;  // -T was given (an empty set then keeps nothing)
};

GFFX_HD inline bool type_allowed(const Types &t, const uint8_t *ty, u64 len) {
    for (uint32_t k = 0; k < t.n; ++k)
        if (t.off[k + 1] - t.off[k] == len && name_equal(t.bytes + t.off[k], ty, len)) return true;
    return false;
}

GFFX_HD inline bool bit_set(const uint32_t *bits, uint32_t i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// write_gff_output_filtered's test of one line (common.rs:418-431), the keep set as integers: line[0, len) (with its line
// ending) lies in the block of `root`; kept iff it is no '#' line, passes -T, and the value after `<key>=` is a name of the
// table whose (last) fid f was requested and has fid_root[f] == root.  (The reference also wants the value and the type to
// be valid UTF-8: the table's names and the -T strings are, and other bytes cannot compare equal to them.)
GFFX_HD inline bool keep_line(const Table &t, const uint32_t *requested, const uint32_t *fid_root, const Types &types,
                              const uint8_t *key, uint32_t key_len, const uint8_t *line, u64 len, uint32_t root) {
    if (len && line[0] == '#') return false;
    const u64 n = body_len(line, len);
    u64 a = 0, z = 0;
    if (types.on) {
        if (!type_slice(line, n, &a, &z)) return false;
        if (!type_allowed(types, line + a, z - a)) return false;
    }
    if (!attr_value_slice(line, n, key, key_len, &a, &z)) return false;
    const uint32_t f = table_find(t, line + a, z - a);
    if (f == kNone || root == kNone) return false;
    return bit_set(requested, f) && fid_root[f] == root;
}

}  // namespace ids
}  // namespace gffx

// ---- host only: the table built in order, with the device's hash and probing ------------------------------------------------
#include <vector>

namespace gffx {
namespace ids {

inline void table_build_host(u64 n, const uint8_t *bytes, const u64 *off, int hash_bits, std::vector<u64> *slot,
                             std::vector<uint32_t> *val) {
    const uint32_t slots = table_slots(n), mask = slots - 1, hm = hash_mask_of(hash_bits);
    slot->assign(slots, kEmptyWord);
    val->assign(slots, 0);
    for (u64 f = 0; f < n; ++f) {
        const u64 len = off[f + 1] - off[f];
        const uint32_t h = name_hash(bytes + off[f], len) & hm;
        for (uint32_t i = h & mask;; i = (i + 1) & mask) {
            const u64 w = (*slot)[i];
            if (w == kEmptyWord) {
                (*slot)[i] = ((u64)h << 32) | f;
                (*val)[i] = (uint32_t)f;
                break;
            }
            const uint32_t rep = (uint32_t)w;
            if ((uint32_t)(w >> 32) == h && off[rep + 1] - off[rep] == len && name_equal(bytes + off[rep], bytes + off[f], len)) {
                if ((*val)[i] < f) (*val)[i] = (uint32_t)f;
                break;
            }
        }
    }
}

}  // namespace ids
}  // namespace gffx
