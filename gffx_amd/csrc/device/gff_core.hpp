// gff_core.hpp -- the rules of one GFF3 line for `gffx index`, shared by the host (g++) and the device (hipcc): what
// index_builder.cpp's line loop decides (reference: index_builder/core.rs:71-138; file:line relative to the reference's src/)
// restated for one line text[0, len) without its '\n'.
//
// Everything in the first part is plain C++17 on flat pointers (GFFX_HD inline, no allocation, no HIP calls), so the same code
// runs in k_gff_rows (gff.hip) and in the sanitizer build of tools/gff_check.cpp.  The text is untrusted and the device must
// never fault on it: every read is bounded by the line's length, every loop by the line or the skip list, and failures come
// back as a status -- nothing asserts, aborts or traps on a condition the input decides.
//
// The checks, in the reference's order (the first that fails decides):
//   1. an empty line, or a first byte '#' (tested before any trimming): kBlank                                   core.rs:78-80
//   2. not valid UTF-8 (the rule of text.cpp utf8_valid: no overlong forms, no surrogates, <= U+10FFFF): kBadUtf8      :82
//   3. Unicode White_Space trimmed at both ends (text.cpp unicode_ws_len's set); empty then: kBlank                 :82-85
//   4. not exactly 9 TAB-separated fields in the trimmed line: kColumns                                             :87-90
//   5. column 3 equals a skip string byte for byte: kSkipType                                                       :92-97
//   6. columns 4 / 5 by parse_u32_rust (optional '+', decimal digits, <= 2^32 - 1), else kDigits                   :99-100
//   7. end == 0: kZeroEnd; start > end swapped; the row is [start ? start - 1 : 0, end)                           :103-109
//   8. ID = the leftmost match of ID=([^;\s]+) over the WHOLE trimmed line; none: kNoId                           :111-115
//   9. Parent the same with `Parent` (optional)                                                                   :117-119
//  10. the attribute value = the leftmost match of <key>=([^;]+): it runs to the next ';' or the end of the trimmed line and
//      may hold TABs and spaces; the row is flagged `warn` when it holds ' ' or ','                              :121-134
// "Leftmost match" is what a regex search does: every occurrence of the key's bytes followed by '=' is tried from the left, an
// empty value makes the search go on from the next byte (`ID=;ID=z` yields z), and the key is not anchored to an attribute's
// start (`geneID=x;ID=y` yields x; a key inside column 2 counts).  ids::attr_value_slice is NOT this rule (it is common.rs's).
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace gff {

typedef unsigned long long u64;

enum Status : int {
    kRow = 0,       // a feature row: Rec is filled
    kBlank = 1,     // empty, a '#' line, or only white space
    kSkipType = 2,  // column 3 is one of the skip strings (Rec::type_a / type_z are set)
    kZeroEnd = 3,   // end == 0
    // errors, in the order of the checks (the numbers are gffx_hip_gff_error's kinds)
    kBadUtf8 = 4,
    kColumns = 5,
    kDigits = 6,
    kNoId = 7,
};
constexpr int kFirstError = kBadUtf8;

GFFX_HD inline const char *status_name(int s) {
    switch (s) {
        case kRow: return "row";
        case kBlank: return "blank";
        case kSkipType: return "skipped_type";
        case kZeroEnd: return "zero_end";
        case kBadUtf8: return "BAD_UTF8";
        case kColumns: return "COLUMNS";
        case kDigits: return "DIGITS";
        case kNoId: return "NO_ID";
        default: return "unknown";
    }
}

struct Rec {        // slices are offsets into the line; [a, a) = absent
    u64 a, z;       // the trimmed line
    u64 type_a, type_z;
    u64 seq_a, seq_z;
    u64 id_a, id_z;
    u64 par_a, par_z;    // par_z == par_a: no Parent
    u64 attr_a, attr_z;  // attr_z == attr_a: no attribute value
    uint32_t start, end;
    uint32_t warn;
};

struct SkipList {  // the skip strings: string k = bytes[off[k], off[k + 1]) (an empty one is a member like any other)
    const uint8_t *bytes;
    const uint32_t *off;
    uint32_t n;
};

// text.cpp utf8_valid
GFFX_HD inline bool utf8_valid(const uint8_t *s, u64 n) {
    u64 i = 0;
    while (i < n) {
        const uint8_t c = s[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        u64 need;
        uint32_t lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) {
            need = 1;
        } else if (c >= 0xE0 && c <= 0xEF) {
            need = 2;
            if (c == 0xE0) lo = 0xA0;
            if (c == 0xED) hi = 0x9F;
        } else if (c >= 0xF0 && c <= 0xF4) {
            need = 3;
            if (c == 0xF0) lo = 0x90;
            if (c == 0xF4) hi = 0x8F;
        } else {
            return false;
        }
        if (n - i <= need) return false;  // the continuation bytes sit at i + 1 .. i + need
        if (s[i + 1] < lo || s[i + 1] > hi) return false;
        for (u64 k = 2; k <= need; ++k)
            if ((s[i + k] & 0xC0) != 0x80) return false;
        i += need + 1;
    }
    return true;
}

// text.cpp unicode_ws_len: the byte length of the White_Space char at p[0, n), 0 if there is none.
// U+0009-000D, 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000
GFFX_HD inline uint32_t ws_len(const uint8_t *p, u64 n) {
    if (n == 0) return 0;
    if ((p[0] >= 0x09 && p[0] <= 0x0D) || p[0] == 0x20) return 1;
    if (p[0] < 0xC2) return 0;
    if (n >= 2 && p[0] == 0xC2 && (p[1] == 0x85 || p[1] == 0xA0)) return 2;
    if (n >= 3) {
        if (p[0] == 0xE1 && p[1] == 0x9A && p[2] == 0x80) return 3;
        if (p[0] == 0xE2 && p[1] == 0x80 && ((p[2] >= 0x80 && p[2] <= 0x8A) || p[2] == 0xA8 || p[2] == 0xA9 || p[2] == 0xAF)) return 3;
        if (p[0] == 0xE2 && p[1] == 0x81 && p[2] == 0x9F) return 3;
        if (p[0] == 0xE3 && p[1] == 0x80 && p[2] == 0x80) return 3;
    }
    return 0;
}

// text.cpp trim_unicode_ws: text[*a, *z) without the White_Space chars at both ends
GFFX_HD inline void trim_ws(const uint8_t *text, u64 len, u64 *a_out, u64 *z_out) {
    u64 a = 0, z = len;
    while (a < z) {
        const uint32_t w = ws_len(text + a, z - a);
        if (!w) break;
        a += w;
    }
    while (a < z) {
        uint32_t w = 0;
        for (uint32_t k = 1; k <= 3 && k <= z - a; ++k)
            if (ws_len(text + z - k, k) == k) {
                w = k;
                break;
            }
        if (!w) break;
        z -= w;
    }
    *a_out = a;
    *z_out = z;
}

// text.cpp parse_u32_rust: an optional '+', then one or more decimal digits, at most 2^32 - 1
GFFX_HD inline bool parse_u32(const uint8_t *p, u64 n, uint32_t *out) {
    u64 i = 0;
    if (n && p[0] == '+') i = 1;
    if (i == n) return false;
    u64 v = 0;
    for (; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        v = v * 10 + (u64)(p[i] - '0');
        if (v > 0xFFFFFFFFull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// the leftmost match of <key>=([^;\s]+) (stop_at_ws) or <key>=([^;]+) in text[a, z): true and the value text[*va, *vz)
GFFX_HD inline bool capture(const uint8_t *text, u64 a, u64 z, const uint8_t *key, uint32_t key_len, bool stop_at_ws, u64 *va, u64 *vz) {
    const u64 need = (u64)key_len + 1;  // the key and '='
    for (u64 p = a; z - p > need && p < z; ++p) {  // (a value needs one byte more)
        if (text[p + key_len] != '=') continue;
        uint32_t k = 0;
        while (k < key_len && text[p + k] == key[k]) ++k;
        if (k < key_len) continue;
        const u64 q0 = p + need;
        u64 q = q0;
        while (q < z && text[q] != ';' && !(stop_at_ws && ws_len(text + q, z - q))) ++q;
        if (q > q0) {
            *va = q0;
            *vz = q;
            return true;
        }
    }
    return false;
}

GFFX_HD inline bool skip_member(const SkipList &s, const uint8_t *ty, u64 len) {
    for (uint32_t k = 0; k < s.n; ++k) {
        const uint32_t a = s.off[k], n = s.off[k + 1] - a;
        if (n != len) continue;
        u64 i = 0;
        while (i < len && s.bytes[a + i] == ty[i]) ++i;
        if (i == len) return true;
    }
    return false;
}

// one line text[0, len) without its '\n'
GFFX_HD inline int gff_record(const uint8_t *text, u64 len, const uint8_t *key, uint32_t key_len, const SkipList &skip, Rec *r) {
    if (len == 0 || text[0] == '#') return kBlank;
    if (!utf8_valid(text, len)) return kBadUtf8;
    u64 a, z;
    trim_ws(text, len, &a, &z);
    r->a = a;
    r->z = z;
    if (a == z) return kBlank;
    u64 tab[8];
    uint32_t nt = 0;
    for (u64 p = a; p < z; ++p)
        if (text[p] == '\t') {
            if (nt < 8) tab[nt] = p;
            ++nt;
        }
    if (nt != 8) return kColumns;
    r->seq_a = a;
    r->seq_z = tab[0];
    r->type_a = tab[1] + 1;
    r->type_z = tab[2];
    if (skip_member(skip, text + r->type_a, r->type_z - r->type_a)) return kSkipType;
    uint32_t s1 = 0, e1 = 0;
    const bool s_ok = parse_u32(text + tab[2] + 1, tab[3] - tab[2] - 1, &s1);
    const bool e_ok = parse_u32(text + tab[3] + 1, tab[4] - tab[3] - 1, &e1);
    if (!s_ok || !e_ok) return kDigits;
    if (e1 == 0) return kZeroEnd;
    if (s1 > e1) {
        const uint32_t t = s1;
        s1 = e1;
        e1 = t;
    }
    r->start = s1 ? s1 - 1 : 0;
    r->end = e1;
    const uint8_t id_key[2] = {'I', 'D'};
    if (!capture(text, a, z, id_key, 2, true, &r->id_a, &r->id_z)) return kNoId;
    const uint8_t par_key[6] = {'P', 'a', 'r', 'e', 'n', 't'};
    if (!capture(text, a, z, par_key, 6, true, &r->par_a, &r->par_z)) r->par_a = r->par_z = 0;
    r->warn = 0;
    if (capture(text, a, z, key, key_len, false, &r->attr_a, &r->attr_z)) {
        for (u64 p = r->attr_a; p < r->attr_z; ++p)
            if (text[p] == ' ' || text[p] == ',') r->warn = 1;
    } else {
        r->attr_a = r->attr_z = 0;
    }
    return kRow;
}

}  // namespace gff
}  // namespace gffx

// ---- host only: the finish steps of gff.hip restated in order (tools/gff_check.cpp `build`) ----------------------------------
#ifndef __HIP_DEVICE_COMPILE__
#include <vector>

#include "ids_core.hpp"

namespace gffx {
namespace gff {

// first[r] = the lowest row whose string equals row r's (eligible rows only; the others: ids::kNone).  The probing is the
// table's (ids_core.hpp), the kept value the LOWEST row, as gff.hip's atomicMin keeps it.
inline void first_rows_host(u64 n, const uint8_t *bytes, const u64 *off, const uint8_t *eligible, int hash_bits, std::vector<uint32_t> *first) {
    const uint32_t slots = ids::table_slots(n), mask = slots - 1, hm = ids::hash_mask_of(hash_bits);
    std::vector<u64> slot(slots, ids::kEmptyWord);
    std::vector<uint32_t> val(slots, ids::kNone);
    for (u64 f = 0; f < n; ++f) {
        if (!eligible[f]) continue;
        const u64 len = off[f + 1] - off[f];
        const uint32_t h = ids::name_hash(bytes + off[f], len) & hm;
        for (uint32_t i = h & mask;; i = (i + 1) & mask) {
            const u64 w = slot[i];
            if (w == ids::kEmptyWord) {
                slot[i] = ((u64)h << 32) | f;
                val[i] = (uint32_t)f;
                break;
            }
            const uint32_t rep = (uint32_t)w;
            if ((uint32_t)(w >> 32) == h && off[rep + 1] - off[rep] == len && ids::name_equal(bytes + off[rep], bytes + off[f], len)) {
                if (val[i] > f) val[i] = (uint32_t)f;
                break;
            }
        }
    }
    const ids::Table t{slot.data(), val.data(), bytes, off, mask, hm};
    first->assign(n, ids::kNone);
    for (u64 f = 0; f < n; ++f)
        if (eligible[f]) (*first)[f] = ids::table_find(t, bytes + off[f], off[f + 1] - off[f]);
}

}  // namespace gff
}  // namespace gffx
#endif
