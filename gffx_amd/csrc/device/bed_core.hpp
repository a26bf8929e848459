// bed_core.hpp -- the rules of one BED line for the host (g++) and the device (hipcc), in the two dialects the commands
// speak.  The two host parsers are the specification:
//   kIntersect  host/bed_parse.cpp parse_bed_chunk     (reference: commands/intersect.rs:201-230)
//   kDepth      host/depth.cpp parse_rows_chunk        (reference: commands/depth.rs:450-495, commands/coverage.rs:230-256)
//
// Everything here is plain C++17 on flat byte pointers (GFFX_HD inline, no allocation, no HIP calls), so the same code runs in
// k_bed_rows (bed.hip) and in the sanitizer build of tools/bed_check.cpp.  The input is untrusted and the device must never
// fault on it: every read is bounded by the line's length, every loop by the line or the table, and failures come back as a
// status -- nothing asserts, aborts or traps on a condition the input decides.
//
// kIntersect: the line is a piece between '\n' (without it).  In this order:
//   1. empty, or first byte '#': skipped (kEmpty / kComment)
//   2. the WHOLE line is not valid UTF-8 (overlong forms, surrogates, > U+10FFFF are invalid): malformed, kBadUtf8
//   3. fields are split on u8::is_ascii_whitespace -- space, \t, \x0C, \r (and \n, which a line does not hold); \x0B is not
//      one.  Fewer than three: skipped (kFewFields)
//   4. field 1 is no name of the table: skipped (kNoSeq) -- before the coordinates are looked at
//   5. fields 2 and 3 by lexical_core::parse::<u32>: an optional '+', at least one digit, the whole field, <= 4294967295,
//      leading zeros allowed; else malformed, kBadCoordinate
//   6. the row is kept whatever start and end are (start >= end too)
// kDepth: the line keeps its '\n' (the last line of a file may have none).  In this order:
//   1. empty, or first byte '#': skipped
//   2. fields are split on \t and space only.  Fewer than three: skipped (kFewFields)
//   3. one of the first three fields is not valid UTF-8: skipped (kFieldUtf8)
//   4. field 2 by str::parse::<u32> (the same number rule as above), field 3 the same after str::trim_end (Unicode White_Space:
//      \t \n \x0B \x0C \r space U+0085 U+00A0 U+1680 U+2000-200A U+2028 U+2029 U+202F U+205F U+3000); unparsable: skipped
//      (kCoordinate); start >= end: skipped (kNoInterval)
//   5. field 1 is no name of the table: skipped (kNoSeq)
//   nothing is malformed.
// Names are looked up in sam_core.hpp's hashed table (sam::Names: FNV-1a, linear probing); entry i is seqid number i.
#pragma once
#include <cstdint>

#include "gff_core.hpp"  // utf8_valid, ws_len (the rules of host/text.cpp)
#include "sam_core.hpp"  // sam::Names, names_find

namespace gffx {
namespace bed {

typedef unsigned long long u64;

enum Dialect : int { kIntersect = 0, kDepth = 1 };

// why bed_record() said kSkip (Row::skip).  Tally: kNoSeq counts as no_seq, every other one as skipped.
enum Skip : int { kEmpty = 1, kComment = 2, kFewFields = 3, kFieldUtf8 = 4, kCoordinate = 5, kNoInterval = 6, kNoSeq = 7 };
// why bed_record() said kMalformed (Row::reason); kIntersect only
enum Reason : int { kNone = 0, kBadUtf8 = 1, kBadCoordinate = 2 };

GFFX_HD inline const char *skip_name(int s) {
    switch (s) {
        case kEmpty: return "empty";
        case kComment: return "comment";
        case kFewFields: return "fewfields";
        case kFieldUtf8: return "fieldutf8";
        case kCoordinate: return "coordinate";
        case kNoInterval: return "nointerval";
        case kNoSeq: return "noseq";
        default: return "unknown";
    }
}
GFFX_HD inline const char *reason_name(int r) {
    switch (r) {
        case kNone: return "ok";
        case kBadUtf8: return "utf8";
        case kBadCoordinate: return "coordinate";
        default: return "unknown";
    }
}

struct Row {
    uint32_t seq, start, end;
    int32_t reason;  // kMalformed: a Reason
    int32_t skip;    // kSkip: a Skip
};

// The shortest line bed_record() keeps: three one-byte fields and two separators ("a 1 2").
constexpr u64 kMinKeptLine = 5;
// The most lines bed_record() can keep in n bytes of text: each but the last takes kMinKeptLine bytes and a '\n'.  k_bed_rows'
// output buffer is sized by it, so it must never be an underestimate.
GFFX_HD inline u64 max_kept_lines(u64 n) { return (n + 1) / (kMinKeptLine + 1); }

// the separators inside a line: kIntersect u8::is_ascii_whitespace, kDepth TAB and space
GFFX_HD inline bool is_sep(uint8_t c, int dialect) {
    if (c == ' ' || c == '\t') return true;
    return dialect == kIntersect && (c == '\x0C' || c == '\r' || c == '\n');
}

// [+]digits, the whole of s[a, z), <= UINT32_MAX (lexical_core::parse::<u32> and str::parse::<u32> agree on this)
GFFX_HD inline bool parse_u32(const uint8_t *s, u64 a, u64 z, uint32_t *out) {
    if (a < z && s[a] == '+') ++a;
    if (a >= z) return false;
    u64 v = 0;
    for (; a < z; ++a) {
        const uint32_t d = (uint32_t)s[a] - '0';
        if (d > 9) return false;
        v = v * 10 + d;
        if (v > 0xFFFFFFFFull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// str::trim_end on the valid UTF-8 s[a, z): the new z
GFFX_HD inline u64 trim_end(const uint8_t *s, u64 a, u64 z) {
    while (z > a) {
        const uint8_t c = s[z - 1];
        if (c == ' ' || (c >= 0x09 && c <= 0x0D)) {
            --z;
            continue;
        }
        u64 cut = 0;
        for (u64 k = 2; k <= 3 && k <= z - a; ++k)
            if (gff::ws_len(s + z - k, k) == k) {
                cut = k;
                break;
            }
        if (!cut) break;
        z -= cut;
    }
    return z;
}

// line[0, len): one line -- kIntersect without its '\n', kDepth with it (when the file has one there).
// kKeep: row->seq / start / end.  kSkip: row->skip says why.  kMalformed: row->reason says why.
GFFX_HD inline int bed_record(const uint8_t *line, u64 len, int dialect, const sam::Names &names, Row *row) {
    row->seq = 0xFFFFFFFFu;
    row->start = row->end = 0;
    row->reason = kNone;
    row->skip = 0;
    if (len == 0) {
        row->skip = kEmpty;
        return bgzf::kSkip;
    }
    if (line[0] == '#') {
        row->skip = kComment;
        return bgzf::kSkip;
    }
    if (dialect == kIntersect && !gff::utf8_valid(line, len)) {
        row->reason = kBadUtf8;
        return bgzf::kMalformed;
    }
    u64 fa[3] = {0, 0, 0}, fz[3] = {0, 0, 0};
    int nf = 0;
    u64 i = 0;
    while (i < len && nf < 3) {
        while (i < len && is_sep(line[i], dialect)) ++i;
        if (i >= len) break;
        fa[nf] = i;
        while (i < len && !is_sep(line[i], dialect)) ++i;
        fz[nf++] = i;
    }
    if (nf < 3) {
        row->skip = kFewFields;
        return bgzf::kSkip;
    }
    const bool name_fits = fz[0] - fa[0] <= 0xFFFFFFFFull;
    if (dialect == kIntersect) {
        if (!name_fits || !sam::names_find(names, line + fa[0], (uint32_t)(fz[0] - fa[0]), &row->seq)) {
            row->seq = 0xFFFFFFFFu;
            row->skip = kNoSeq;
            return bgzf::kSkip;
        }
        if (!parse_u32(line, fa[1], fz[1], &row->start) || !parse_u32(line, fa[2], fz[2], &row->end)) {
            row->reason = kBadCoordinate;
            return bgzf::kMalformed;
        }
        return bgzf::kKeep;
    }
    for (int f = 0; f < 3; ++f)
        if (!gff::utf8_valid(line + fa[f], fz[f] - fa[f])) {
            row->skip = kFieldUtf8;
            return bgzf::kSkip;
        }
    if (!parse_u32(line, fa[1], fz[1], &row->start) || !parse_u32(line, fa[2], trim_end(line, fa[2], fz[2]), &row->end)) {
        row->skip = kCoordinate;
        return bgzf::kSkip;
    }
    if (row->start >= row->end) {
        row->skip = kNoInterval;
        return bgzf::kSkip;
    }
    if (!name_fits || !sam::names_find(names, line + fa[0], (uint32_t)(fz[0] - fa[0]), &row->seq)) {
        row->seq = 0xFFFFFFFFu;
        row->skip = kNoSeq;
        return bgzf::kSkip;
    }
    return bgzf::kKeep;
}

}  // namespace bed
}  // namespace gffx
