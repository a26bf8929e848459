// sam_core.hpp -- the SAM text front end for the host (g++) and the device (hipcc): where the header ends, what one alignment
// line contributes to `gffx depth` / `gffx coverage`, and the table that turns a reference NAME into a seqid number.
//
// A SAM file (SAM spec §1.3, §1.4) is text: header lines that begin with '@', then one alignment per line, eleven mandatory
// TAB-separated fields  QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL  and optional tags.  The reference reads
// .sam through the reader it uses for .bam (commands/depth.rs:588-591, commands/coverage.rs:520-541), so a line yields what
// the BAM record of the same alignment yields (bgzf_core.hpp bam_record): tid, pos = POS - 1, end = bam_endpos.
//
// Everything in the first part is plain C++17 on flat byte pointers (GFFX_HD inline, no allocation, no HIP calls), so the same
// code runs in k_sam_rows (sam.hip) and in the sanitizer build of tools/sam_check.cpp.  The input is untrusted and the device
// must never fault on it: every read is bounded by the line's length, every loop by the line or the table, and failures come
// back as a status -- nothing asserts, aborts or traps on a condition the input decides.
//
// Only fields 2, 3, 4 and 6 (FLAG, RNAME, POS, CIGAR) are interpreted.  DEVIATION: htslib also parses fields 5 and 7 to 11 and
// the tags and rejects, among others, a SEQ whose length differs from the CIGAR's query length; here those fields only have to
// exist (ten TABs), their content is not validated.
//
// ASSUMPTION (restated from memory of htslib's sam.c sam_parse1, whose source is not at hand; tools/pin_against_reference.py
// lists them among what a real `gffx` run would pin):
//   1. a record without flag 0x4 whose CIGAR is `*` ("mapped query must have a CIGAR; treated as unmapped") is treated as
//      unmapped: it is dropped and counted with the unmapped ones.  (The BAM reader keeps a mapped record without CIGAR ops
//      with end = pos + 1: bam_read1 has no such rule.)
//   2. a CIGAR operation length of 2^28 or more is an error (BAM packs the length into 28 bits).
//   3. an RNAME that no @SQ line names gets a warning and tid -1: the read counts as one without a reference and is dropped.
// The end is bam_endpos as bgzf_core.hpp:501 restates it: pos + the summed lengths of M/D/N/=/X, a sum of 0 counting as 1.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD, kOk / kTruncated, kKeep / kSkip / kMalformed

namespace gffx {
namespace sam {

typedef unsigned long long u64;

// why sam_record() said kMalformed (Row::reason)
enum Reason : int {
    kNone = 0,
    kFewFields = 1,  // fewer than 11 TAB-separated fields (an empty line too)
    kBadFlag = 2,    // FLAG is not 1 to 5 decimal digits <= 65535 without a leading zero (`0x10`, `016`, `70000`)
    kBadPos = 3,     // POS is not 1 to 18 decimal digits
    kBadCigar = 4,   // CIGAR is neither `*` nor <digits><op in MIDNSHP=XB>..., or a length is 2^28 or more
};

GFFX_HD inline const char *status_name(int reason) {
    switch (reason) {
        case kNone: return "ok";
        case kFewFields: return "fewer than 11 fields";
        case kBadFlag: return "FLAG is not a decimal number up to 65535";
        case kBadPos: return "POS is not a number of 1 to 18 decimal digits";
        case kBadCigar: return "CIGAR is neither * nor <length><op> pairs with op in MIDNSHP=XB and length < 2^28";
        default: return "unknown status";
    }
}

// ---- header -------------------------------------------------------------------------------------------------------------
// Header lines are the leading lines that begin with '@'.  kOk: *header_bytes = the offset of the first line that does not.
// kTruncated: text[0, n) ends inside the header -- inside a header line, or right after one (the next line may be another).
// (A file that is all header is a kTruncated stream at its end: the caller then takes n.)
GFFX_HD inline int sam_header_scan(const uint8_t *text, u64 n, u64 *header_bytes) {
    u64 p = 0;
    while (p < n) {
        if (text[p] != '@') {
            *header_bytes = p;
            return bgzf::kOk;
        }
        while (p < n && text[p] != '\n') ++p;
        if (p == n) return bgzf::kTruncated;
        ++p;
    }
    return bgzf::kTruncated;
}

// ---- names table --------------------------------------------------------------------------------------------------------
// Open addressing, linear probing, a power of two >= 2 * n_ref slots (so a probe always ends at an empty slot).
struct NameEntry {
    uint32_t hash;     // FNV-1a (32 bit) of the name
    uint32_t off;      // the name's offset in Names::bytes; kEmptySlot: empty
    uint32_t len;
    uint32_t ref_seq;  // the index's seqid number of this reference; UINT32_MAX: the index has no such seqid
};
constexpr uint32_t kEmptySlot = 0xFFFFFFFFu;

struct Names {
    const NameEntry *table;
    const uint8_t *bytes;
    uint32_t mask;  // slots - 1
};

GFFX_HD inline uint32_t fnv1a(const uint8_t *p, uint32_t n) {
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// true: *ref_seq = the entry's value.  false: no @SQ line has this name.
GFFX_HD inline bool names_find(const Names &t, const uint8_t *name, uint32_t len, uint32_t *ref_seq) {
    const uint32_t h = fnv1a(name, len);
    for (uint32_t i = h & t.mask, steps = 0; steps <= t.mask; i = (i + 1) & t.mask, ++steps) {
        const NameEntry e = t.table[i];
        if (e.off == kEmptySlot) return false;
        if (e.hash != h || e.len != len) continue;
        const uint8_t *q = t.bytes + e.off;
        uint32_t k = 0;
        while (k < len && q[k] == name[k]) ++k;
        if (k == len) {
            *ref_seq = e.ref_seq;
            return true;
        }
    }
    return false;
}

// ---- one alignment line -------------------------------------------------------------------------------------------------
struct Row {
    uint32_t seq;    // seqid number of RNAME (UINT32_MAX: `*`, a name without @SQ line, or one the index does not have)
    uint32_t start, end;
    uint32_t flag;
    int32_t reason;  // kMalformed: a Reason
    int32_t skip;    // kSkip: a Skip
};
enum Skip : int { kUnmapped = 1, kNoSeq = 2, kNoInterval = 3 };  // flag 0x4 or `*` CIGAR; no seqid; pos < 0 or end <= pos

// scans from *p to the next TAB: true, *end = its offset, *p = one past it; false: the line has no further TAB
GFFX_HD inline bool field_end(const uint8_t *line, u64 len, u64 *p, u64 *end) {
    u64 i = *p;
    while (i < len && line[i] != '\t') ++i;
    if (i >= len) return false;
    *end = i;
    *p = i + 1;
    return true;
}

constexpr uint32_t kMaxCigarLen = 1u << 28;
constexpr u64 kMaxRlen = 1ull << 40;  // the reference length saturates here (the end is clamped to UINT32_MAX anyway)

// The shortest line sam_record() keeps: ten TABs, one digit of FLAG, one of POS, one digit and one op of CIGAR -- fields 1, 5
// and 7 to 11 may be empty, and so may RNAME when an @SQ line has the empty name (`SN:`).  "\t0\t\t1\t\t1M\t\t\t\t\t".
constexpr u64 kMinKeptLine = 14;
// The most lines sam_record() can keep in n bytes of text: each but the last takes kMinKeptLine bytes and a '\n'.  k_sam_rows'
// output buffer is sized by it, so it must never be an underestimate.
GFFX_HD inline u64 max_kept_lines(u64 n) { return (n + 1) / (kMinKeptLine + 1); }

// line[0, len): one line without its '\n' (a '\r' before it stays in the last field, which is not interpreted).
// kKeep: row->seq / start / end are the row the reference pushes (depth.rs:335-364).  kSkip: row->skip says why.
// kMalformed: row->reason says why.  All four fields are checked before any of them decides a skip, as a parser that reads
// the whole line before the caller looks at the flag does.
GFFX_HD inline int sam_record(const uint8_t *line, u64 len, const Names &names, Row *row) {
    row->seq = 0xFFFFFFFFu;
    row->start = row->end = row->flag = 0;
    row->reason = kNone;
    row->skip = 0;
    // fields 1 to 6: t1 .. t6 = the offsets of the TABs that end them
    u64 p = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0;
    if (!field_end(line, len, &p, &t1) || !field_end(line, len, &p, &t2) || !field_end(line, len, &p, &t3) ||
        !field_end(line, len, &p, &t4) || !field_end(line, len, &p, &t5) || !field_end(line, len, &p, &t6)) {
        row->reason = kFewFields;
        return bgzf::kMalformed;
    }
    // FLAG
    const u64 fa = t1 + 1, fz = t2;
    if (fz == fa || fz - fa > 5 || (line[fa] == '0' && fz - fa > 1)) {
        row->reason = kBadFlag;
        return bgzf::kMalformed;
    }
    uint32_t flag = 0;
    for (u64 i = fa; i < fz; ++i) {
        const uint32_t d = (uint32_t)line[i] - '0';
        if (d > 9) {
            row->reason = kBadFlag;
            return bgzf::kMalformed;
        }
        flag = flag * 10 + d;
    }
    if (flag > 65535) {
        row->reason = kBadFlag;
        return bgzf::kMalformed;
    }
    row->flag = flag;
    // POS
    const u64 pa = t3 + 1, pz = t4;
    if (pz == pa || pz - pa > 18) {
        row->reason = kBadPos;
        return bgzf::kMalformed;
    }
    int64_t pos = 0;
    for (u64 i = pa; i < pz; ++i) {
        const uint32_t d = (uint32_t)line[i] - '0';
        if (d > 9) {
            row->reason = kBadPos;
            return bgzf::kMalformed;
        }
        pos = pos * 10 + d;
    }
    pos -= 1;
    // CIGAR
    const u64 ca = t5 + 1, cz = t6;
    const bool star = cz - ca == 1 && line[ca] == '*';
    u64 rlen = 0;
    if (!star) {
        if (cz == ca) {
            row->reason = kBadCigar;
            return bgzf::kMalformed;
        }
        uint32_t v = 0;
        bool digits = false;
        for (u64 i = ca; i < cz; ++i) {
            const uint8_t c = line[i];
            const uint32_t d = (uint32_t)c - '0';
            if (d <= 9) {
                v = v * 10 + d;  // (< 10 * 2^28: no overflow)
                digits = true;
                if (v >= kMaxCigarLen) {
                    row->reason = kBadCigar;
                    return bgzf::kMalformed;
                }
                continue;
            }
            const bool ref = c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X';
            const bool other = c == 'I' || c == 'S' || c == 'H' || c == 'P' || c == 'B';
            if (!digits || !(ref || other)) {
                row->reason = kBadCigar;
                return bgzf::kMalformed;
            }
            if (ref && rlen < kMaxRlen) rlen += v;
            v = 0;
            digits = false;
        }
        if (digits) {  // a length without an operation
            row->reason = kBadCigar;
            return bgzf::kMalformed;
        }
    }
    // fields 7 to 11 exist: four more TABs
    u64 t = 0;
    if (!field_end(line, len, &p, &t) || !field_end(line, len, &p, &t) || !field_end(line, len, &p, &t) ||
        !field_end(line, len, &p, &t)) {
        row->reason = kFewFields;
        return bgzf::kMalformed;
    }
    // RNAME
    const u64 ra = t2 + 1, rz = t3;
    const bool no_name = rz - ra == 1 && line[ra] == '*';
    if (!no_name && rz - ra <= 0xFFFFFFFFull) (void)names_find(names, line + ra, (uint32_t)(rz - ra), &row->seq);
    if (flag & 0x4) {
        row->skip = kUnmapped;
        return bgzf::kSkip;
    }
    if (star) {
        row->skip = kUnmapped;
        return bgzf::kSkip;
    }
    if (row->seq == 0xFFFFFFFFu) {
        row->skip = kNoSeq;
        return bgzf::kSkip;
    }
    if (pos < 0) {
        row->skip = kNoInterval;
        return bgzf::kSkip;
    }
    if (rlen == 0) rlen = 1;
    const int64_t end = pos + (int64_t)rlen;
    if (end <= pos) {
        row->skip = kNoInterval;
        return bgzf::kSkip;
    }
    row->start = pos > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)pos;
    row->end = end > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)end;
    return bgzf::kKeep;
}

}  // namespace sam
}  // namespace gffx

// ---- host only: the @SQ names of a header and the table built from them ---------------------------------------------------
#include <string>
#include <vector>

namespace gffx {
namespace sam {

// the SN: values of the @SQ lines of header[0, n), in order (the order defines the tid)
inline std::vector<std::string> sq_names(const uint8_t *header, u64 n) {
    std::vector<std::string> out;
    for (u64 p = 0; p < n;) {
        u64 e = p;
        while (e < n && header[e] != '\n') ++e;
        u64 z = e;
        if (z > p && header[z - 1] == '\r') --z;
        if (z - p >= 4 && header[p] == '@' && header[p + 1] == 'S' && header[p + 2] == 'Q' && header[p + 3] == '\t') {
            for (u64 a = p + 4; a < z;) {  // TAB-separated TAG:VALUE fields
                u64 b = a;
                while (b < z && header[b] != '\t') ++b;
                if (b - a >= 3 && header[a] == 'S' && header[a + 1] == 'N' && header[a + 2] == ':') {
                    out.emplace_back(reinterpret_cast<const char *>(header + a + 3), (size_t)(b - a - 3));
                    break;
                }
                a = b + 1;
            }
        }
        p = e + 1;
    }
    return out;
}

// names[name_off[i], name_off[i + 1]) = reference i's name, ref_seq[i] its value.  Returns -1 when built, else the index of
// a name that an earlier reference has already (htslib's header parser fails on a duplicate SN).
inline long names_build(uint32_t n_ref, const uint8_t *names, const uint64_t *name_off, const uint32_t *ref_seq,
                        std::vector<NameEntry> *table) {
    uint32_t slots = 2;
    while (slots < 2ull * n_ref) slots <<= 1;
    table->assign(slots, NameEntry{0, kEmptySlot, 0, 0xFFFFFFFFu});
    const uint32_t mask = slots - 1;
    for (uint32_t r = 0; r < n_ref; ++r) {
        const uint8_t *nm = names + name_off[r];
        const uint32_t len = (uint32_t)(name_off[r + 1] - name_off[r]);
        const uint32_t h = fnv1a(nm, len);
        uint32_t i = h & mask;
        for (; (*table)[i].off != kEmptySlot; i = (i + 1) & mask) {
            const NameEntry &e = (*table)[i];
            if (e.hash == h && e.len == len && std::char_traits<char>::compare(reinterpret_cast<const char *>(names + e.off),
                                                                               reinterpret_cast<const char *>(nm), len) == 0)
                return (long)r;
        }
        (*table)[i] = NameEntry{h, (uint32_t)name_off[r], len, ref_seq[r]};
    }
    return -1;
}

}  // namespace sam
}  // namespace gffx
