// effect_text.hpp -- the text side of `gffx effect` that the command (effect.cpp) and the one-core check tool
// (tools/effect_check.cpp) share, so that their outputs are the same bytes: the variants file, the grouping of member lines into
// numbered transcripts, the table's lines and the summary.  Plain C++17 on string_views, no HIP; device/effect_core.hpp has the
// rules and the record.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../device/effect_core.hpp"
#include "feature_rows.hpp"

namespace gffx::commands::effect_text {

typedef unsigned long long u64;

// ---- the variants file: plain text, lines end at '\n' (a '\r' before it taken off); empty lines and '#' lines are skipped;
// every other line needs 5 TAB-separated fields CHROM POS ID REF ALT, POS 1 to 10 decimal digits in 1 .. 2^32 - 1.  ALT is split
// at ','; a piece is TAKEN when REF and the piece are each one byte of ACGTNacgtn, else it is counted as not an SNV.
struct Allele {
    std::string_view chrom;
    uint32_t x;
    uint8_t ref, alt;
};
struct VcfPart {
    std::vector<Allele> alleles;
    u64 not_snv = 0, lines = 0;  // lines: the '\n' of the part
    u64 bad_line = 0;            // the first line in error, counted from 1 inside the part; 0: none
    const char *bad = nullptr;
};
inline bool is_base(char c) { return std::strchr("ACGTNacgtn", c) != nullptr && c != 0; }

// the lines that BEGIN in text[lo, hi) (lo is a line start): what both parsers share -- line ends, '#' and empty lines, the five
// fields, POS, the split of ALT at ','.  piece(CHROM, POS, REF, the piece) is called for every piece of every good line.
template <class Part, class OnPiece>
inline void scan_vcf_part(std::string_view text, size_t lo, size_t hi, Part &P, OnPiece &&piece) {
    u64 line_no = 0;
    for (size_t ls = lo; ls < hi;) {
        size_t le = text.find('\n', ls);
        const bool terminated = le != std::string_view::npos;
        if (!terminated) le = text.size();
        ++line_no;
        P.lines += terminated;
        std::string_view line = text.substr(ls, le - ls);
        ls = le + 1;
        if (terminated && !line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (line.empty() || line[0] == '#') continue;
        std::string_view f[5];
        size_t at = 0;
        int n = 0;
        for (; n < 5; ++n) {
            size_t tab = line.find('\t', at);
            if (tab == std::string_view::npos) {
                f[n++] = line.substr(at);
                break;
            }
            f[n] = line.substr(at, tab - at);
            at = tab + 1;
        }
        if (n < 5) {
            if (!P.bad_line) P.bad_line = line_no, P.bad = "fewer than 5 TAB-separated fields (CHROM POS ID REF ALT)";
            continue;
        }
        u64 pos = 0;
        bool ok = !f[1].empty() && f[1].size() <= 10;
        for (char c : f[1]) {
            ok = ok && c >= '0' && c <= '9';
            pos = pos * 10 + (u64)(c - '0');
        }
        if (!ok || pos < 1 || pos > 0xFFFFFFFFull) {
            if (!P.bad_line) P.bad_line = line_no, P.bad = "POS is not a number in 1 .. 4294967295";
            continue;
        }
        for (size_t a = 0; a <= f[4].size();) {
            size_t c = f[4].find(',', a);
            if (c == std::string_view::npos) c = f[4].size();
            piece(f[0], (uint32_t)pos, f[3], f[4].substr(a, c - a));
            a = c + 1;
        }
    }
}
inline VcfPart parse_vcf_part(std::string_view text, size_t lo, size_t hi) {
    VcfPart P;
    scan_vcf_part(text, lo, hi, P, [&](std::string_view chrom, uint32_t pos, std::string_view ref, std::string_view alt) {
        if (ref.size() == 1 && is_base(ref[0]) && alt.size() == 1 && is_base(alt[0])) P.alleles.push_back(Allele{chrom, pos, (uint8_t)ref[0], (uint8_t)alt[0]});
        else ++P.not_snv;
    });
    return P;
}

// where part k of n begins: the first line start at or behind size * k / n
inline size_t part_begin(std::string_view text, size_t k, size_t n) {
    if (k == 0) return 0;
    if (k >= n) return text.size();
    const size_t at = text.size() / n * k;
    if (at == 0) return 0;
    const size_t nl = text.find('\n', at - 1);
    return nl == std::string_view::npos ? text.size() : nl + 1;
}

// ---- transcripts: a member line belongs to every name of its Parent value; transcripts are numbered by first appearance; seqid
// and strand are the first member's; the phase is that of the leading CDS segment (the smallest (start, line order) on plus,
// the largest on minus)
struct Member {
    uint32_t seqid;  // the caller's number of the line's seqid (what "mixed" compares)
    uint32_t fa;     // the sequence number of the genome, UINT32_MAX when the FASTA lacks the seqid
    uint32_t start0, end;
    uint8_t kind;  // 0 CDS, 1 exon
    bool minus;
    char phase;
    std::string_view parent;
};
struct Transcripts {
    std::vector<uint32_t> rows;  // 5 per row: transcript, fa, start - 1, end, kind
    std::vector<uint8_t> flags;
    std::vector<std::string_view> names;
    std::vector<char> strand;
    u64 orphans = 0, mixed = 0;
};
inline Transcripts group_members(const std::vector<Member> &members) {
    struct Lead {
        uint32_t seqid, start0;
        bool minus, mixed, has_cds;
        char phase;
    };
    Transcripts T;
    std::vector<Lead> lead;
    std::unordered_map<std::string_view, uint32_t> by_name;
    for (const Member &m : members) {
        bool any = false;
        feature_rows::for_each_parent(m.parent, [&](std::string_view name) {
            any = true;
            const auto [it, fresh] = by_name.emplace(name, (uint32_t)T.names.size());
            if (fresh) {
                T.names.push_back(name);
                lead.push_back(Lead{m.seqid, 0u, m.minus, false, false, '.'});
            }
            Lead &l = lead[it->second];
            if (l.seqid != m.seqid || l.minus != m.minus) l.mixed = true;
            // (members come in line order: a later CDS with the same start follows in the order, so it leads on minus only)
            if (m.kind == 0 && (!l.has_cds || (l.minus ? m.start0 >= l.start0 : m.start0 < l.start0))) l.start0 = m.start0, l.phase = m.phase, l.has_cds = true;
            T.rows.insert(T.rows.end(), {it->second, m.fa, m.start0, m.end, (uint32_t)m.kind});
        });
        T.orphans += !any;
    }
    for (const Lead &l : lead) {
        T.mixed += l.mixed;
        T.flags.push_back((uint8_t)((l.minus ? effect::kFlagMinus : 0u) | (seq::phase_skip((uint8_t)l.phase) << 1) | (l.mixed ? effect::kFlagDropped : 0u)));
        T.strand.push_back(l.minus ? '-' : '+');
    }
    return T;
}

// ---- the table
inline const char *kHeader = "#chrom\tpos\tref\talt\ttranscript\tstrand\tclass\tcds_pos\tcodons\taa_pos\taa\tref_match\n";

struct Summary {
    u64 alleles[effect::kClasses] = {}, pairs[effect::kClasses] = {};
    std::string text() const {
        std::string s;
        char num[64];
        for (uint32_t c = 0; c < effect::kClasses; ++c) {
            s += effect::class_name(c);
            s.append(num, std::snprintf(num, sizeof num, "\t%llu\t%llu\n", alleles[c], pairs[c]));
        }
        return s;
    }
};

inline char upper(uint8_t b) { return (char)(b >= 'a' && b <= 'z' ? b - 32 : b); }

// the lines of one allele: its n records in transcript order (n == 0: the intergenic line)
inline void format_allele(std::string &out, Summary &sum, const Allele &a, const effect::Record *rec, u64 n, uint8_t ref_match, const std::vector<std::string_view> &names,
                          const std::vector<char> &strand) {
    char num[96];
    std::string head(a.chrom);
    head.append(num, std::snprintf(num, sizeof num, "\t%u\t%c\t%c\t", a.x, (char)a.ref, (char)a.alt));
    if (n == 0) {
        out += head;
        out.append(num, std::snprintf(num, sizeof num, ".\t.\tintergenic\t.\t.\t.\t.\t%u\n", (unsigned)ref_match));
        ++sum.alleles[effect::kIntergenic], ++sum.pairs[effect::kIntergenic];
        return;
    }
    uint32_t seen = 0;
    for (u64 k = 0; k < n; ++k) {
        const effect::Record &r = rec[k];
        out += head;
        out.append(names[r.transcript]);
        out.push_back('\t');
        out.push_back(strand[r.transcript]);
        out.push_back('\t');
        out += effect::class_name(r.cls);
        if (effect::is_coding(r.cls))
            out.append(num, std::snprintf(num, sizeof num, "\t%llu\t%c%c%c>%c%c%c\t%llu\t%c>%c\t%u\n", r.q + 1, upper(r.codon_ref[0]), upper(r.codon_ref[1]),
                                          upper(r.codon_ref[2]), upper(r.codon_alt[0]), upper(r.codon_alt[1]), upper(r.codon_alt[2]), r.c + 1, (char)r.aa_ref, (char)r.aa_alt,
                                          (unsigned)r.ref_match));
        else
            out.append(num, std::snprintf(num, sizeof num, "\t.\t.\t.\t.\t%u\n", (unsigned)r.ref_match));
        ++sum.pairs[r.cls];
        if (!(seen >> r.cls & 1u)) ++sum.alleles[r.cls], seen |= 1u << r.cls;
    }
}

// ---- --indels: REF and a piece of 1 .. 65 535 bytes of ACGTNacgtn each, trimmed (effect::trim): d reference
// bases from x0 on, m alternate bytes.  The genome is not consulted: nothing is left-aligned.  Left out and counted, each kind
// on its own: a piece (or a REF) that is empty or holds another byte ('*', '.', symbolic, breakend); a REF or piece longer than
// 65 535 bytes; a piece equal to REF; a pure insertion in front of base 1.
constexpr size_t kMaxAlleleBytes = 65535;
struct AlleleAny {
    std::string_view chrom, ref, alt;  // the file's own REF and piece: what the table prints
    uint32_t pos, pfx, d, m;           // x0 = pos + pfx (64 bits: it may pass 2^32 - 1); R' = ref[pfx, pfx + d), A' = alt[pfx, pfx + m)
    unsigned long long x0() const { return (unsigned long long)pos + pfx; }
    bool snv() const { return d == 1 && m == 1; }
};
struct VcfPartAny {
    std::vector<AlleleAny> alleles;
    u64 other = 0, too_long = 0, same = 0, ins_at_1 = 0, lines = 0, bad_line = 0;
    const char *bad = nullptr;
};
inline bool all_bases(std::string_view s) {
    if (s.empty()) return false;
    for (char c : s)
        if (!is_base(c)) return false;
    return true;
}
inline VcfPartAny parse_vcf_part_any(std::string_view text, size_t lo, size_t hi) {
    VcfPartAny P;
    scan_vcf_part(text, lo, hi, P, [&](std::string_view chrom, uint32_t pos, std::string_view ref, std::string_view piece) {
        if (!all_bases(ref) || !all_bases(piece)) {
            ++P.other;
            return;
        }
        if (ref.size() > kMaxAlleleBytes || piece.size() > kMaxAlleleBytes) {
            ++P.too_long;
            return;
        }
        const effect::Trimmed t = effect::trim(reinterpret_cast<const uint8_t *>(ref.data()), (uint32_t)ref.size(), reinterpret_cast<const uint8_t *>(piece.data()), (uint32_t)piece.size());
        if (t.d == 0 && t.m == 0) ++P.same;
        else if (t.d == 0 && (u64)pos + t.pfx == 1) ++P.ins_at_1;
        else P.alleles.push_back(AlleleAny{chrom, ref, piece, pos, t.pfx, t.d, t.m});
    });
    return P;
}
// the four warnings of --indels, in this order
inline void warn_left_out(u64 other, u64 too_long, u64 same, u64 ins_at_1) {
    if (other) std::fprintf(stderr, "[WARN] %llu alleles are not sequences of ACGTN (*, ., symbolic, breakend or another byte) and were left out\n", other);
    if (too_long) std::fprintf(stderr, "[WARN] %llu alleles have a REF or an ALT longer than 65535 bytes and were left out\n", too_long);
    if (same) std::fprintf(stderr, "[WARN] %llu alleles are equal to REF and were left out\n", same);
    if (ins_at_1) std::fprintf(stderr, "[WARN] %llu alleles are insertions in front of a sequence's first base and were left out\n", ins_at_1);
}

// the device's row of an allele (6 words: sequence number, x0, d, m, the 64-bit offset of R' then A' in the arena), its bytes
// appended to the arena.  An allele whose footprint passes 2^32 - 1 lies beyond every sequence: it goes as one on no sequence.
inline void append_row_any(std::vector<uint32_t> &rows, std::vector<uint8_t> &arena, const AlleleAny &a, uint32_t fa) {
    const u64 x0 = a.x0(), top = a.d ? x0 + a.d - 1 : x0, off = arena.size();
    const bool beyond = top > 0xFFFFFFFFull;
    rows.insert(rows.end(), {beyond ? 0xFFFFFFFFu : fa, beyond ? 2u : (uint32_t)x0, a.d, a.m, (uint32_t)off, (uint32_t)(off >> 32)});
    arena.insert(arena.end(), a.ref.begin() + a.pfx, a.ref.begin() + a.pfx + a.d);
    arena.insert(arena.end(), a.alt.begin() + a.pfx, a.alt.begin() + a.pfx + a.m);
}

struct SummaryAll {
    u64 alleles[effect::kClassesAll] = {}, pairs[effect::kClassesAll] = {};
    std::string text() const {
        std::string s;
        char num[64];
        for (uint32_t c = 0; c < effect::kClassesAll; ++c) {
            s += effect::class_name(c);
            s.append(num, std::snprintf(num, sizeof num, "\t%llu\t%llu\n", alleles[c], pairs[c]));
        }
        return s;
    }
    void add(const SummaryAll &o) {
        for (uint32_t c = 0; c < effect::kClassesAll; ++c) alleles[c] += o.alleles[c], pairs[c] += o.pairs[c];
    }
};

// rule 3 was reached: a non-SNV allele's cds_pos (and, but for partial_codon, aa_pos) are printed
inline bool any_in_cds(uint32_t cls) { return cls == effect::kPartialCodon || effect::is_coding(cls) || (cls >= effect::kFrameshift && cls <= effect::kInframeDeletion); }

// the lines of one --indels allele: POS, REF and the piece as the file has them; an SNV's lines are format_allele's, byte for byte
inline void format_allele_any(std::string &out, SummaryAll &sum, const AlleleAny &a, const effect::Record *rec, u64 n, uint8_t ref_match,
                              const std::vector<std::string_view> &names, const std::vector<char> &strand) {
    char num[96];
    std::string head(a.chrom);
    head.append(num, std::snprintf(num, sizeof num, "\t%u\t", a.pos));
    head.append(a.ref);
    head.push_back('\t');
    head.append(a.alt);
    head.push_back('\t');
    if (n == 0) {
        out += head;
        out.append(num, std::snprintf(num, sizeof num, ".\t.\tintergenic\t.\t.\t.\t.\t%u\n", (unsigned)ref_match));
        ++sum.alleles[effect::kIntergenic], ++sum.pairs[effect::kIntergenic];
        return;
    }
    uint32_t seen = 0;
    const bool snv = a.snv();
    for (u64 k = 0; k < n; ++k) {
        const effect::Record &r = rec[k];
        out += head;
        out.append(names[r.transcript]);
        out.push_back('\t');
        out.push_back(strand[r.transcript]);
        out.push_back('\t');
        out += effect::class_name(r.cls);
        if (snv && effect::is_coding(r.cls))
            out.append(num, std::snprintf(num, sizeof num, "\t%llu\t%c%c%c>%c%c%c\t%llu\t%c>%c\t%u\n", r.q + 1, upper(r.codon_ref[0]), upper(r.codon_ref[1]),
                                          upper(r.codon_ref[2]), upper(r.codon_alt[0]), upper(r.codon_alt[1]), upper(r.codon_alt[2]), r.c + 1, (char)r.aa_ref, (char)r.aa_alt,
                                          (unsigned)r.ref_match));
        else if (!snv && r.cls == effect::kPartialCodon)
            out.append(num, std::snprintf(num, sizeof num, "\t%llu\t.\t.\t.\t%u\n", r.q + 1, (unsigned)r.ref_match));
        else if (!snv && any_in_cds(r.cls))
            out.append(num, std::snprintf(num, sizeof num, "\t%llu\t.\t%llu\t.\t%u\n", r.q + 1, r.c + 1, (unsigned)r.ref_match));
        else
            out.append(num, std::snprintf(num, sizeof num, "\t.\t.\t.\t.\t%u\n", (unsigned)r.ref_match));
        ++sum.pairs[r.cls];
        if (!(seen >> r.cls & 1u)) ++sum.alleles[r.cls], seen |= 1u << r.cls;
    }
}

}  // namespace gffx::commands::effect_text
