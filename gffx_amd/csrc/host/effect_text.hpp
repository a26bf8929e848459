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

// the lines that BEGIN in text[lo, hi) (lo is a line start)
inline VcfPart parse_vcf_part(std::string_view text, size_t lo, size_t hi) {
    VcfPart P;
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
        const bool ref_ok = f[3].size() == 1 && is_base(f[3][0]);
        for (size_t a = 0; a <= f[4].size();) {
            size_t c = f[4].find(',', a);
            if (c == std::string_view::npos) c = f[4].size();
            if (ref_ok && c - a == 1 && is_base(f[4][a])) P.alleles.push_back(Allele{f[0], (uint32_t)pos, (uint8_t)f[3][0], (uint8_t)f[4][a]});
            else ++P.not_snv;
            a = c + 1;
        }
    }
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

}  // namespace gffx::commands::effect_text
