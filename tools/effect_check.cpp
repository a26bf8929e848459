// effect_check.cpp -- device/effect_core.hpp and host/effect_text.hpp on the host, without a GPU (tests/test_effect_cpu.py builds
// it under ASan + UBSan and holds its answers to tests/_effect_definition.py); built without the sanitizers it is
// effect_host_baseline, the one-core yardstick of tools/effect_bench.py: the same rules, one thread.  Every array the rules read
// is an exact-size heap copy, so a read past an end is the sanitizer's.
//
//   effect_check --classes            the class names in summary order
//   effect_check --rules FILE         a case in numbers; lines of FILE:
//                                       S LEN BASES    a sequence of LEN bases, BASES its first ones ("-": none are given; a
//                                                      case then asks for nothing that reads a base beyond them)
//                                       T FLAGS        a transcript (minus | phase << 1 | 8), numbered in order
//                                       R T SEQ START0 END KIND    a member row
//                                       A SEQ X REF ALT            an allele
//                                     prints per transcript "t DROPPED FIRST LAST", per allele "a PAIRS REF_MATCH" and per pair
//                                     "p TRANSCRIPT CLASS Q C K CODON_REF CODON_ALT AA_REF AA_ALT" ('-' where a class leaves them)
//   effect_check --vcf FILE PARTS     the variants file in PARTS parts: "allele CHROM X REF ALT" lines, then "not_snv N", or
//                                     "error LINE WHAT"
//   effect_check --run GFF FASTA VCF CDS_TYPE EXON_TYPE OUT SUMMARY   the command on one core ("-": no summary); warnings and the
//                                     stage times to stderr
//   effect_check --run --indels GFF FASTA VCF CDS_TYPE EXON_TYPE OUT SUMMARY   the command with --indels
//   effect_check --all-classes        the 20 class names of --indels in summary order
//   effect_check --indel-rules FILE   as --rules, with alleles "I SEQ X0 REF ALT": trimmed already, "-" an empty string; per pair
//                                     "p TRANSCRIPT CLASS Q C K"; an allele of one base each way prints the line of --rules
//   effect_check --trim POS REF ALT   "X0 D M" of the trimming
//   effect_check --vcf-indels FILE PARTS   the variants file as --indels reads it: "allele CHROM POS REF ALT X0 D M" lines, then
//                                     "left_out OTHER TOO_LONG SAME INS_AT_1", or "error LINE WHAT"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../gffx_amd/csrc/device/effect_core.hpp"
#include "../gffx_amd/csrc/host/effect_text.hpp"
#include "../gffx_amd/csrc/host/feature_rows.hpp"

namespace ef = gffx::effect;
namespace et = gffx::commands::effect_text;
namespace sq = gffx::seq;
namespace fr = gffx::commands::feature_rows;
typedef unsigned long long u64;

static std::string slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {  // (no slack behind the last element)
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// the transcripts on the host: what effect.hip builds on the device, and the span lookup the engine's index gives there
struct Host {
    uint32_t n = 0, n_tr = 0, n_seq = 0;
    std::unique_ptr<uint32_t[]> start0, end, row_seq, pmax, seq_len;
    std::unique_ptr<u64[]> pre, seq_off;
    std::unique_ptr<uint8_t[]> arena;
    std::unique_ptr<ef::Transcript[]> tr;
    std::vector<uint8_t> dropped;
    std::vector<uint32_t> lo0, hi;
    // per sequence the kept transcripts by (span start, number) and the running maximum of their ends
    std::vector<std::vector<uint32_t>> by_lo, run_hi;

    // rows: 5 per row; bases[s]: the given bases of sequence s (at most len[s])
    void build(const std::vector<uint32_t> &rows, const std::vector<uint8_t> &flags, const std::vector<u64> &len, const std::vector<std::string> &bases) {
        n = (uint32_t)(rows.size() / 5), n_tr = (uint32_t)flags.size(), n_seq = (uint32_t)len.size();
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const uint32_t ka = 2 * rows[5 * a] + rows[5 * a + 4], kb = 2 * rows[5 * b] + rows[5 * b + 4];
            return ka != kb ? ka < kb : rows[5 * a + 2] < rows[5 * b + 2];
        });
        std::vector<uint32_t> s0(n), e(n), rs(n), key(n), sl(n_seq);
        std::vector<u64> p(n + 1, 0), so(n_seq + 1, 0);
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t *r = &rows[5 * order[j]];
            key[j] = 2 * r[0] + r[4], rs[j] = r[1], s0[j] = r[2], e[j] = r[3];
            p[j + 1] = p[j] + (r[3] - r[2]);
        }
        std::string all;
        for (uint32_t s = 0; s < n_seq; ++s) sl[s] = (uint32_t)len[s], so[s] = all.size(), all += bases[s];
        so[n_seq] = all.size();
        start0 = exact(s0), end = exact(e), row_seq = exact(rs), pre = exact(p), seq_len = exact(sl), seq_off = exact(so);
        pmax.reset(new uint32_t[n]);
        arena.reset(new uint8_t[all.size()]);
        std::memcpy(arena.get(), all.data(), all.size());
        tr.reset(new ef::Transcript[n_tr]);
        dropped.assign(n_tr, 1), lo0.assign(n_tr, 0), hi.assign(n_tr, 0);
        by_lo.assign(n_seq, {}), run_hi.assign(n_seq, {});
        for (uint32_t t = 0; t < n_tr; ++t) {
            const uint32_t f0 = (uint32_t)(std::lower_bound(key.begin(), key.end(), 2 * t) - key.begin());
            const uint32_t f1 = (uint32_t)(std::lower_bound(key.begin(), key.end(), 2 * t + 1) - key.begin());
            const uint32_t f2 = (uint32_t)(std::lower_bound(key.begin(), key.end(), 2 * t + 2) - key.begin());
            ef::Transcript o{};
            if (f2 > f0) {
                const bool ok = ef::build_transcript(start0.get(), end.get(), row_seq.get(), pre.get(), pmax.get(), f0, f1, f2, seq_len.get(), n_seq, &o, &lo0[t], &hi[t]);
                const bool keep = ok && !(flags[t] & ef::kFlagDropped);
                o.flags = flags[t] | (o.flags & ef::kFlagOverlap), o.base = keep ? seq_off[o.seq] : 0;
                dropped[t] = keep ? 0 : 1;
                if (keep) by_lo[o.seq].push_back(t);
            }
            tr[t] = o;
        }
        for (uint32_t s = 0; s < n_seq; ++s) {
            std::stable_sort(by_lo[s].begin(), by_lo[s].end(), [&](uint32_t a, uint32_t b) { return lo0[a] < lo0[b]; });
            uint32_t run = 0;
            for (uint32_t t : by_lo[s]) run_hi[s].push_back(run = std::max(run, hi[t]));
        }
    }
    bool served(uint32_t s, uint32_t x) const { return s < n_seq && x >= 1 && x <= seq_len[s]; }
    // the kept transcripts of sequence s whose span contains x, by number
    void hits(uint32_t s, uint32_t x, std::vector<uint32_t> &out) const {
        out.clear();
        if (!served(s, x)) return;
        const std::vector<uint32_t> &L = by_lo[s];
        size_t k = std::partition_point(L.begin(), L.end(), [&](uint32_t t) { return lo0[t] < x; }) - L.begin();
        while (k > 0 && run_hi[s][k - 1] >= x) {
            --k;
            if (hi[L[k]] >= x) out.push_back(L[k]);
        }
        std::sort(out.begin(), out.end());
    }
    // the kept transcripts of sequence s whose span meets [lo, hi], by number
    void hits_range(uint32_t s, u64 lo, u64 hi, std::vector<uint32_t> &out) const {
        out.clear();
        if (s >= n_seq || lo < 1 || hi > seq_len[s]) return;
        const std::vector<uint32_t> &L = by_lo[s];
        size_t k = std::partition_point(L.begin(), L.end(), [&](uint32_t t) { return lo0[t] < hi; }) - L.begin();
        while (k > 0 && run_hi[s][k - 1] >= lo) {
            --k;
            if (this->hi[L[k]] >= lo) out.push_back(L[k]);
        }
        std::sort(out.begin(), out.end());
    }
    ef::Record classify_any(uint32_t t, uint32_t x0, uint32_t d, uint32_t m, const uint8_t *ins, uint8_t rm) const {
        const ef::Rows rows{start0.get(), end.get(), pre.get(), pmax.get()};
        ef::Record r = d == 1 && m == 1 ? ef::classify(rows, tr[t], arena.get(), x0, ins[0]) : ef::classify_any(rows, tr[t], arena.get(), x0, d, m, ins);
        r.transcript = t, r.ref_match = rm;
        return r;
    }
    uint8_t ref_match_run(uint32_t s, u64 lo, u64 hi, u64 x0, const uint8_t *ref, uint32_t d) const {
        if (s >= n_seq || lo < 1 || hi > seq_len[s]) return 0;
        if (d == 0) return 1;
        if (seq_off[s] + x0 - 1 + d > seq_off[s + 1]) return 0;  // (bases that --indel-rules was not given)
        return ef::ref_match_run(ref, d, arena.get() + seq_off[s] + (x0 - 1));
    }
    ef::Record classify(uint32_t t, uint32_t x, uint8_t alt, uint8_t rm) const {
        const ef::Rows rows{start0.get(), end.get(), pre.get(), pmax.get()};
        ef::Record r = ef::classify(rows, tr[t], arena.get(), x, alt);
        r.transcript = t, r.ref_match = rm;
        return r;
    }
    // (a sequence's given bases may be fewer than its length: --rules)
    uint8_t ref_match(uint32_t s, uint32_t x, uint8_t ref) const {
        if (!served(s, x) || seq_off[s] + x > seq_off[s + 1]) return 0;
        return ef::ref_match(ref, arena[seq_off[s] + (x - 1)]);
    }
};

static int rules(const char *path) {
    std::istringstream in(slurp(path));
    std::vector<uint32_t> rows;
    std::vector<uint8_t> flags;
    std::vector<u64> len;
    std::vector<std::string> bases;
    struct A {
        uint32_t s, x;
        char ref, alt;
    };
    std::vector<A> alleles;
    std::string kind;
    while (in >> kind) {
        if (kind == "S") {
            u64 l;
            std::string b;
            in >> l >> b;
            len.push_back(l), bases.push_back(b == "-" ? "" : b);
        } else if (kind == "T") {
            unsigned f;
            in >> f;
            flags.push_back((uint8_t)f);
        } else if (kind == "R") {
            uint32_t r[5];
            in >> r[0] >> r[1] >> r[2] >> r[3] >> r[4];
            rows.insert(rows.end(), r, r + 5);
        } else if (kind == "A") {
            A a;
            in >> a.s >> a.x >> a.ref >> a.alt;
            alleles.push_back(a);
        } else {
            return 2;
        }
    }
    Host H;
    H.build(rows, flags, len, bases);
    for (uint32_t t = 0; t < H.n_tr; ++t) std::printf("t %u %u %u\n", (unsigned)H.dropped[t], H.lo0[t] + 1, H.hi[t]);
    std::vector<uint32_t> hit;
    for (const A &a : alleles) {
        H.hits(a.s, a.x, hit);
        const uint8_t rm = H.ref_match(a.s, a.x, (uint8_t)a.ref);
        std::printf("a %zu %u\n", hit.size(), (unsigned)rm);
        for (uint32_t t : hit) {
            const ef::Record r = H.classify(t, a.x, (uint8_t)a.alt, rm);
            if (ef::is_coding(r.cls))
                std::printf("p %u %s %llu %llu %u %c%c%c %c%c%c %c %c\n", t, ef::class_name(r.cls), r.q, r.c, (unsigned)r.k, r.codon_ref[0], r.codon_ref[1], r.codon_ref[2],
                            r.codon_alt[0], r.codon_alt[1], r.codon_alt[2], r.aa_ref, r.aa_alt);
            else
                std::printf("p %u %s %llu %llu %u - - - -\n", t, ef::class_name(r.cls), r.q, r.c, (unsigned)r.k);
        }
    }
    return 0;
}

static void print_pair(const ef::Record &r, bool snv) {
    if (snv && ef::is_coding(r.cls))
        std::printf("p %u %s %llu %llu %u %c%c%c %c%c%c %c %c\n", r.transcript, ef::class_name(r.cls), r.q, r.c, (unsigned)r.k, r.codon_ref[0], r.codon_ref[1], r.codon_ref[2],
                    r.codon_alt[0], r.codon_alt[1], r.codon_alt[2], r.aa_ref, r.aa_alt);
    else if (snv)
        std::printf("p %u %s %llu %llu %u - - - -\n", r.transcript, ef::class_name(r.cls), r.q, r.c, (unsigned)r.k);
    else
        std::printf("p %u %s %llu %llu %u\n", r.transcript, ef::class_name(r.cls), r.q, r.c, (unsigned)r.k);
}

static int indel_rules(const char *path) {
    std::istringstream in(slurp(path));
    std::vector<uint32_t> rows;
    std::vector<uint8_t> flags;
    std::vector<u64> len;
    std::vector<std::string> bases;
    struct A {
        uint32_t s, x0;
        std::string ref, alt;
    };
    std::vector<A> alleles;
    std::string kind;
    while (in >> kind) {
        if (kind == "S") {
            u64 l;
            std::string b;
            in >> l >> b;
            len.push_back(l), bases.push_back(b == "-" ? "" : b);
        } else if (kind == "T") {
            unsigned f;
            in >> f;
            flags.push_back((uint8_t)f);
        } else if (kind == "R") {
            uint32_t r[5];
            in >> r[0] >> r[1] >> r[2] >> r[3] >> r[4];
            rows.insert(rows.end(), r, r + 5);
        } else if (kind == "I") {
            A a;
            in >> a.s >> a.x0 >> a.ref >> a.alt;
            if (a.ref == "-") a.ref.clear();
            if (a.alt == "-") a.alt.clear();
            alleles.push_back(a);
        } else {
            return 2;
        }
    }
    Host H;
    H.build(rows, flags, len, bases);
    for (uint32_t t = 0; t < H.n_tr; ++t) std::printf("t %u %u %u\n", (unsigned)H.dropped[t], H.lo0[t] + 1, H.hi[t]);
    std::vector<uint32_t> hit;
    for (const A &a : alleles) {
        const uint32_t d = (uint32_t)a.ref.size(), m = (uint32_t)a.alt.size();
        const u64 lo = d ? (u64)a.x0 : (u64)a.x0 - 1, hi = d ? (u64)a.x0 + d - 1 : (u64)a.x0;
        // (exact-size copies: a read past R' or A' is the sanitizer's)
        const std::unique_ptr<uint8_t[]> ref = exact(std::vector<uint8_t>(a.ref.begin(), a.ref.end())), alt = exact(std::vector<uint8_t>(a.alt.begin(), a.alt.end()));
        H.hits_range(a.s, lo, hi, hit);
        const uint8_t rm = H.ref_match_run(a.s, lo, hi, a.x0, ref.get(), d);
        std::printf("a %zu %u\n", hit.size(), (unsigned)rm);
        for (uint32_t t : hit) print_pair(H.classify_any(t, a.x0, d, m, alt.get(), rm), d == 1 && m == 1);
    }
    return 0;
}

static int trim(const char *pos, const char *ref, const char *alt) {
    const ef::Trimmed t = ef::trim(reinterpret_cast<const uint8_t *>(ref), (uint32_t)std::strlen(ref), reinterpret_cast<const uint8_t *>(alt), (uint32_t)std::strlen(alt));
    std::printf("%llu %u %u\n", std::strtoull(pos, nullptr, 10) + t.pfx, t.d, t.m);
    return 0;
}

static int vcf_indels(const char *path, size_t parts) {
    const std::string text = slurp(path);
    u64 lines_before = 0, cnt[4] = {0, 0, 0, 0};
    std::vector<et::VcfPartAny> P;
    for (size_t p = 0; p < parts; ++p) P.push_back(et::parse_vcf_part_any(text, et::part_begin(text, p, parts), et::part_begin(text, p + 1, parts)));
    for (const et::VcfPartAny &part : P) {
        if (part.bad_line) {
            std::printf("error %llu %s\n", lines_before + part.bad_line, part.bad);
            return 1;
        }
        lines_before += part.lines;
    }
    for (const et::VcfPartAny &part : P) {
        for (const et::AlleleAny &a : part.alleles)
            std::printf("allele %.*s %u %.*s %.*s %llu %u %u\n", (int)a.chrom.size(), a.chrom.data(), a.pos, (int)a.ref.size(), a.ref.data(), (int)a.alt.size(), a.alt.data(), a.x0(),
                        a.d, a.m);
        cnt[0] += part.other, cnt[1] += part.too_long, cnt[2] += part.same, cnt[3] += part.ins_at_1;
    }
    std::printf("left_out %llu %llu %llu %llu\n", cnt[0], cnt[1], cnt[2], cnt[3]);
    return 0;
}

static int vcf(const char *path, size_t parts) {
    const std::string text = slurp(path);
    u64 lines_before = 0, not_snv = 0;
    std::vector<et::VcfPart> P;
    for (size_t p = 0; p < parts; ++p) P.push_back(et::parse_vcf_part(text, et::part_begin(text, p, parts), et::part_begin(text, p + 1, parts)));
    for (const et::VcfPart &part : P) {
        if (part.bad_line) {
            std::printf("error %llu %s\n", lines_before + part.bad_line, part.bad);
            return 1;
        }
        lines_before += part.lines;
    }
    for (const et::VcfPart &part : P) {
        for (const et::Allele &a : part.alleles) std::printf("allele %.*s %u %c %c\n", (int)a.chrom.size(), a.chrom.data(), a.x, a.ref, a.alt);
        not_snv += part.not_snv;
    }
    std::printf("not_snv %llu\n", not_snv);
    return 0;
}

static int run(int argc, char **argv) {
    const bool indels = argc == 10 && std::strcmp(argv[2], "--indels") == 0;
    if (indels) ++argv, --argc;
    if (argc != 9) return 2;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string gff = slurp(argv[2]), fasta = slurp(argv[3]), variants = slurp(argv[4]);
    const std::string cds_type = argv[5], exon_type = argv[6];
    if (fasta.size() >= 2 && (uint8_t)fasta[0] == 0x1f && (uint8_t)fasta[1] == 0x8b) return std::fprintf(stderr, "Error: compressed FASTA is not read: decompress \"%s\" first\n", argv[3]), 1;
    if (variants.size() >= 2 && (uint8_t)variants[0] == 0x1f && (uint8_t)variants[1] == 0x8b)
        return std::fprintf(stderr, "Error: compressed variants file is not read: decompress \"%s\" first\n", argv[4]), 1;
    const auto t1 = std::chrono::steady_clock::now();
    // the variants
    et::VcfPart V;
    et::VcfPartAny VA;
    if (indels) VA = et::parse_vcf_part_any(variants, 0, variants.size());
    else V = et::parse_vcf_part(variants, 0, variants.size());
    if (indels) V.bad_line = VA.bad_line, V.bad = VA.bad;
    if (V.bad_line) return std::fprintf(stderr, "Error: variants file %s, line %llu: %s\n", argv[4], V.bad_line, V.bad), 1;
    const auto t2 = std::chrono::steady_clock::now();
    // the genome
    std::vector<std::string> names, seqs;
    {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(fasta.data());
        const u64 N = fasta.size();
        std::unordered_map<std::string, int> seen;
        u64 line_no = 0;
        for (u64 ls = 0; ls < N;) {
            const void *e = std::memchr(p + ls, '\n', N - ls);
            const u64 le = e ? (u64)(static_cast<const uint8_t *>(e) - p) : N;
            const bool terminated = e != nullptr;
            const sq::LineClass c = sq::classify_line(p, ls, le, terminated, false);
            ++line_no;
            if (c.kind == sq::kLineHeader) {
                const u64 end = terminated && p[le - 1] == '\r' ? le - 1 : le;
                const std::string name(fasta, ls + 1, sq::name_end(p, ls, end) - ls - 1);
                if (name.empty()) return std::fprintf(stderr, "Error: FASTA file %s, line %llu: a '>' line without a sequence name\n", argv[3], line_no), 1;
                if (!seen.emplace(name, 1).second) return std::fprintf(stderr, "Error: FASTA file %s, line %llu: the sequence name \"%s\" is given twice\n", argv[3], line_no, name.c_str()), 1;
                names.push_back(name), seqs.emplace_back();
            } else if (c.kind == sq::kLineBases && c.kept) {
                if (names.empty()) return std::fprintf(stderr, "Error: FASTA file %s, line %llu: sequence data before the first '>' line\n", argv[3], line_no), 1;
                seqs.back().append(fasta, ls, c.kept);
            }
            ls = le + 1;
        }
    }
    std::unordered_map<std::string_view, uint32_t> fa_of;
    for (size_t i = 0; i < names.size(); ++i) fa_of.emplace(names[i], (uint32_t)i);
    const auto t3 = std::chrono::steady_clock::now();
    // the member lines and the seqids of the annotation
    std::unordered_map<std::string_view, uint32_t> seqid_num;
    std::vector<et::Member> members;
    const std::string_view text(gff);
    for (size_t ls = 0; ls < text.size();) {
        size_t le = text.find('\n', ls);
        if (le == std::string_view::npos) le = text.size();
        const std::string_view line = text.substr(ls, le - ls);
        const size_t line_start = ls;
        ls = le + 1;
        if (line.empty() || line[0] == '#') continue;
        std::string_view col[5];
        size_t at = 0, tabs = 0;
        for (size_t k = 0; k < line.size(); ++k) tabs += line[k] == '\t';
        int n = 0;
        for (; n < 5; ++n) {
            const size_t tab = line.find('\t', at);
            if (tab == std::string_view::npos) break;
            col[n] = line.substr(at, tab - at);
            at = tab + 1;
        }
        if (n < 5) continue;
        if (tabs >= 8) seqid_num.emplace(col[0], (uint32_t)seqid_num.size());
        const int kind = col[2] == cds_type ? 0 : col[2] == exon_type ? 1 : -1;
        if (kind < 0) continue;
        char *e1 = nullptr, *e2 = nullptr;
        const std::string a(col[3]), b(col[4]);
        const u64 s = std::strtoull(a.c_str(), &e1, 10), e = std::strtoull(b.c_str(), &e2, 10);
        if (a.empty() || b.empty() || *e1 || *e2 || s < 1 || s > e || e > 0xFFFFFFFFull) continue;
        const fr::SeqFields f = fr::read_seq_fields(text, line_start);
        const auto fa = fa_of.find(col[0]);
        const auto num = seqid_num.emplace(col[0], (uint32_t)seqid_num.size()).first->second;
        members.push_back(et::Member{num, fa == fa_of.end() ? 0xFFFFFFFFu : fa->second, (uint32_t)(s - 1), (uint32_t)e, (uint8_t)kind, f.si.minus, f.phase, f.parent});
    }
    const et::Transcripts T = et::group_members(members);
    const auto t4 = std::chrono::steady_clock::now();
    Host H;
    {
        std::vector<u64> len;
        for (const std::string &s : seqs) len.push_back(s.size());
        H.build(T.rows, T.flags, len, seqs);
    }
    u64 n_unservable = 0, no_chrom = 0;
    for (uint32_t t = 0; t < H.n_tr; ++t) n_unservable += H.dropped[t] && !(T.flags[t] & ef::kFlagDropped);
    if (indels) et::warn_left_out(VA.other, VA.too_long, VA.same, VA.ins_at_1);
    if (V.not_snv) std::fprintf(stderr, "[WARN] %llu alleles are not single-base substitutions and were left out\n", V.not_snv);
    if (T.orphans) std::fprintf(stderr, "[WARN] %llu features have no Parent and belong to no transcript\n", T.orphans);
    if (T.mixed) std::fprintf(stderr, "[WARN] %llu transcripts were dropped: their members lie on more than one seqid or strand\n", T.mixed);
    if (n_unservable) std::fprintf(stderr, "[WARN] %llu transcripts were dropped: a member lies on a seqid the FASTA file lacks or beyond its sequence\n", n_unservable);
    const auto t5 = std::chrono::steady_clock::now();
    // the pairs (the span lookup and the rules: what the pair pass and k_effect_pairs do on the device), then the table
    std::vector<uint32_t> hit;
    std::vector<ef::Record> recs;
    std::vector<u64> off{0};
    std::vector<uint8_t> rms;
    std::vector<et::Allele> taken;
    std::vector<et::AlleleAny> taken_any;
    for (const et::AlleleAny &a : VA.alleles) {
        if (!seqid_num.count(a.chrom)) {
            ++no_chrom;
            continue;
        }
        const auto fa = fa_of.find(a.chrom);
        const uint32_t s = fa == fa_of.end() ? 0xFFFFFFFFu : fa->second;
        const u64 x0 = a.x0(), lo = a.d ? x0 : x0 - 1, hi = a.d ? x0 + a.d - 1 : x0;
        const uint8_t *rp = reinterpret_cast<const uint8_t *>(a.ref.data()) + a.pfx, *ap = reinterpret_cast<const uint8_t *>(a.alt.data()) + a.pfx;
        H.hits_range(s, lo, hi, hit);
        const uint8_t rm = H.ref_match_run(s, lo, hi, x0, rp, a.d);
        for (uint32_t t : hit) recs.push_back(H.classify_any(t, (uint32_t)x0, a.d, a.m, ap, rm));
        off.push_back(recs.size()), rms.push_back(rm), taken_any.push_back(a);
    }
    for (const et::Allele &a : V.alleles) {
        if (!seqid_num.count(a.chrom)) {
            ++no_chrom;
            continue;
        }
        const auto fa = fa_of.find(a.chrom);
        const uint32_t s = fa == fa_of.end() ? 0xFFFFFFFFu : fa->second;
        H.hits(s, a.x, hit);
        const uint8_t rm = H.ref_match(s, a.x, a.ref);
        for (uint32_t t : hit) recs.push_back(H.classify(t, a.x, a.alt, rm));
        off.push_back(recs.size()), rms.push_back(rm), taken.push_back(a);
    }
    const auto t5b = std::chrono::steady_clock::now();
    std::string out = et::kHeader;
    et::Summary sum;
    et::SummaryAll sum_all;
    const u64 n_alleles = taken.size() + taken_any.size(), n_pairs = recs.size();
    for (u64 i = 0; i < taken.size(); ++i) et::format_allele(out, sum, taken[i], recs.data() + off[i], off[i + 1] - off[i], rms[i], T.names, T.strand);
    for (u64 i = 0; i < taken_any.size(); ++i) et::format_allele_any(out, sum_all, taken_any[i], recs.data() + off[i], off[i + 1] - off[i], rms[i], T.names, T.strand);
    if (no_chrom) std::fprintf(stderr, "[WARN] %llu alleles lie on a seqid the index does not have and were left out\n", no_chrom);
    const auto t6 = std::chrono::steady_clock::now();
    std::ofstream o(argv[7], std::ios::binary);
    o.write(out.data(), (std::streamsize)out.size());
    o.close();
    bool ok = (bool)o;
    if (std::strcmp(argv[8], "-") != 0) {
        std::ofstream so(argv[8], std::ios::binary);
        const std::string s = indels ? sum_all.text() : sum.text();
        so.write(s.data(), (std::streamsize)s.size());
        so.close();
        ok = ok && so;
    }
    const auto t7 = std::chrono::steady_clock::now();
    const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "read_ms %.3f vcf_ms %.3f fasta_ms %.3f features_ms %.3f build_ms %.3f pairs_ms %.3f format_ms %.3f write_ms %.3f total_ms %.3f alleles %llu pairs %llu\n",
                 ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5), ms(t5, t5b), ms(t5b, t6), ms(t6, t7), ms(t0, t7), n_alleles, n_pairs);
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "--classes") {
        for (uint32_t c = 0; c < ef::kClasses; ++c) std::printf("%s\n", ef::class_name(c));
        return 0;
    }
    if (mode == "--all-classes") {
        for (uint32_t c = 0; c < ef::kClassesAll; ++c) std::printf("%s\n", ef::class_name(c));
        return 0;
    }
    if (mode == "--rules" && argc == 3) return rules(argv[2]);
    if (mode == "--indel-rules" && argc == 3) return indel_rules(argv[2]);
    if (mode == "--trim" && argc == 5) return trim(argv[2], argv[3], argv[4]);
    if (mode == "--vcf-indels" && argc == 4) return vcf_indels(argv[2], (size_t)std::max(1, std::atoi(argv[3])));
    if (mode == "--vcf" && argc == 4) return vcf(argv[2], (size_t)std::max(1, std::atoi(argv[3])));
    if (mode == "--run") return run(argc, argv);
    std::fprintf(stderr, "usage: effect_check --classes | --all-classes | --rules FILE | --indel-rules FILE | --trim POS REF ALT | --vcf FILE PARTS | --vcf-indels FILE PARTS | --run [--indels] GFF FASTA VCF CDS_TYPE EXON_TYPE OUT SUMMARY\n");
    return 2;
}
