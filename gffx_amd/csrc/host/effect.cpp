// effect.cpp -- `gffx effect` above the C-ABI (an addition: the reference has no such command): what every
// single-base substitution of a variants file does to every transcript it hits.  device/effect_core.hpp has the definition,
// effect_text.hpp the text side that the check tool shares.  The index, the features and the genome are loaded as `gffx seq`
// loads them: the CDS and exon lines through layer_rows.hpp, strand, phase and Parent from the mapped text on -t threads, the
// FASTA packed on the device.  Grouping by Parent and the variants file are string work and stay here; the device gets numeric
// member rows once (gffx_hip_effect_create) and then chunks of GFFX_EFFECT_CHUNK_ROWS allele rows through two slots, so that
// chunk k is formatted (on -t threads) while chunk k + 1 is classified.  The class counts of --summary are summed here, from
// the records.  With --indels the variants are parsed into trimmed alleles of any length, a chunk is rows of six
// words and a byte arena (gffx_hip_effect_run_any_start), and the summary has 20 lines; without the flag nothing here changes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "effect_text.hpp"
#include "intersect_internal.hpp"
#include "layer_rows.hpp"
#include "table_output.hpp"

namespace gffx::commands::effect {

namespace {

namespace et = gffx::commands::effect_text;
namespace rules = gffx::effect;
using GenomeHandle = Handle<gffx_hip_genome, gffx_hip_genome_destroy>;
using EffectHandle = Handle<gffx_hip_effect, gffx_hip_effect_destroy>;

// GFFX_EFFECT_CHUNK_ROWS: a positive decimal number (at most 2^30 is taken); anything else is ignored
uint64_t chunk_rows_from_env() {
    const char *e = std::getenv("GFFX_EFFECT_CHUNK_ROWS");
    if (e && *e >= '0' && *e <= '9') {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end && !*end && v > 0) return std::min<unsigned long long>(v, 1ull << 30);
    }
    return 4ull << 20;
}

}  // namespace

void run(const EffectArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    const size_t threads = args.common.effective_threads();
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    timer.lap("Loading tree index");
    const MappedFile fasta = map_file_or(args.fasta, "Cannot open FASTA file: \"" + args.fasta + "\"");
    if (fasta.size() >= 2 && fasta.data()[0] == 0x1f && fasta.data()[1] == 0x8b) throw Error("compressed FASTA is not read: decompress \"" + args.fasta + "\" first");
    const MappedFile vcf = map_file_or(args.variants, "Cannot open variants file: \"" + args.variants + "\"");
    if (vcf.size() >= 2 && vcf.data()[0] == 0x1f && vcf.data()[1] == 0x8b) throw Error("compressed variants file is not read: decompress \"" + args.variants + "\" first");
    DeviceWarmup warm(args.device);

    // the variants, on -t threads: parts cut at line starts, the first error of the lowest part wins
    std::vector<et::Allele> alleles;
    std::vector<et::AlleleAny> alleles_any;  // --indels: these in place of alleles
    uint64_t not_snv = 0, no_chrom = 0, left_out[4] = {0, 0, 0, 0};
    if (args.indels) {
        const std::string_view text = vcf.view();
        const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, text.size() / (1u << 20) + 1));
        std::vector<et::VcfPartAny> part(parts);
        parallel_for(parts, parts, [&](size_t p) { part[p] = et::parse_vcf_part_any(text, et::part_begin(text, p, parts), et::part_begin(text, p + 1, parts)); });
        uint64_t lines_before = 0, total = 0;
        for (const et::VcfPartAny &P : part) {
            if (P.bad_line) throw Error("variants file " + args.variants + ", line " + std::to_string(lines_before + P.bad_line) + ": " + P.bad);
            lines_before += P.lines, total += P.alleles.size();
            left_out[0] += P.other, left_out[1] += P.too_long, left_out[2] += P.same, left_out[3] += P.ins_at_1;
        }
        alleles_any.reserve(total);
        for (et::VcfPartAny &P : part) alleles_any.insert(alleles_any.end(), P.alleles.begin(), P.alleles.end());
    } else {
        const std::string_view text = vcf.view();
        const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, text.size() / (1u << 20) + 1));
        std::vector<et::VcfPart> part(parts);
        parallel_for(parts, parts, [&](size_t p) { part[p] = et::parse_vcf_part(text, et::part_begin(text, p, parts), et::part_begin(text, p + 1, parts)); });
        uint64_t lines_before = 0, total = 0;
        for (const et::VcfPart &P : part) {
            if (P.bad_line) throw Error("variants file " + args.variants + ", line " + std::to_string(lines_before + P.bad_line) + ": " + P.bad);
            lines_before += P.lines, total += P.alleles.size(), not_snv += P.not_snv;
        }
        alleles.reserve(total);
        for (et::VcfPart &P : part) alleles.insert(alleles.end(), P.alleles.begin(), P.alleles.end());
    }
    timer.lap("Variants file");

    // the member lines, in file order
    const std::vector<std::string> types{args.cds_type, args.exon_type};
    std::vector<uint32_t> rows;  // (layer, seqid, start - 1, end); layer 0: CDS, 1: exon
    std::vector<feature_rows::SeqFields> fields;
    const MappedFile gff = map_file_or(args.common.input, "Cannot open GFF file: \"" + args.common.input + "\"");
    uint64_t skipped = 0;
    {
        std::vector<uint64_t> per_type(types.size(), 0), line_start;
        layer_rows::collect(args.common.input, types, index_data.seqid_to_num, threads, verbose, rows, per_type, skipped, nullptr, &line_start);
        const std::string_view text = gff.view();
        const size_t G = rows.size() / 4;
        fields.resize(G);
        const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, G / 4096 + 1));
        parallel_for(parts, parts, [&](size_t p) {
            for (size_t i = G * p / parts; i < G * (p + 1) / parts; ++i) fields[i] = feature_rows::read_seq_fields(text, line_start[i]);
        });
        layer_rows::report(args.common.input, types, per_type, "", nullptr, skipped);
    }
    const size_t G = rows.size() / 4;
    timer.lap("Features from the line table");

    // the genome: packed on the device
    warm.wait();
    GenomeHandle genome;
    if (gffx_hip_genome_create(args.device, 0, OutPtr(genome)) != GFFX_OK) hip_fail("gffx_hip_genome_create");
    if (gffx_hip_genome_reserve(genome.get(), fasta.size()) != GFFX_OK) hip_fail("gffx_hip_genome_reserve");
    if (gffx_hip_genome_feed(genome.get(), fasta.data(), fasta.size()) != GFFX_OK || gffx_hip_genome_finish(genome.get()) != GFFX_OK)
        throw Error("FASTA file " + args.fasta + ", " + gffx_hip_last_error());
    const uint32_t n_fa = gffx_hip_genome_n_seq(genome.get());
    std::vector<uint32_t> fa_of_seqid(index_data.num_to_seqid.size(), UINT32_MAX);
    {
        std::vector<uint8_t> names(std::max<uint64_t>(gffx_hip_genome_name_bytes(genome.get()), 1));
        std::vector<uint64_t> name_off(n_fa + 1);
        if (gffx_hip_genome_copy_names(genome.get(), names.data(), name_off.data()) != GFFX_OK) hip_fail("gffx_hip_genome_copy_names");
        for (uint32_t g = 0; g < n_fa; ++g) {
            const auto it = index_data.seqid_to_num.find(std::string(reinterpret_cast<const char *>(names.data()) + name_off[g], name_off[g + 1] - name_off[g]));
            if (it != index_data.seqid_to_num.end() && it->second < fa_of_seqid.size()) fa_of_seqid[it->second] = g;
        }
    }
    timer.lap("FASTA upload and pack");

    // the transcripts and the device's rows
    std::vector<et::Member> members(G);
    for (size_t i = 0; i < G; ++i)
        members[i] = et::Member{rows[4 * i + 1], fa_of_seqid[rows[4 * i + 1]], rows[4 * i + 2], rows[4 * i + 3], static_cast<uint8_t>(rows[4 * i]), fields[i].si.minus,
                                fields[i].phase,   fields[i].parent};
    const et::Transcripts T = et::group_members(members);
    const size_t R = T.flags.size();
    const uint64_t chunk = chunk_rows_from_env();
    EffectHandle eff;
    if (gffx_hip_effect_create(genome.get(), T.rows.size() / 5, T.rows.data(), R, T.flags.data(), std::max<uint64_t>(1, std::min<uint64_t>(chunk, args.indels ? alleles_any.size() : alleles.size())), OutPtr(eff)) !=
        GFFX_OK)
        hip_fail("gffx_hip_effect_create");
    std::vector<uint8_t> dropped(std::max<size_t>(R, 1), 0);
    if (gffx_hip_effect_copy_transcripts(eff.get(), dropped.data(), nullptr) != GFFX_OK) hip_fail("gffx_hip_effect_copy_transcripts");
    uint64_t n_unservable = 0, n_kept = 0;
    for (size_t r = 0; r < R; ++r) {
        n_unservable += dropped[r] && !(T.flags[r] & rules::kFlagDropped);
        n_kept += !dropped[r];
    }
    if (args.indels) et::warn_left_out(left_out[0], left_out[1], left_out[2], left_out[3]);
    if (not_snv) std::fprintf(stderr, "[WARN] %llu alleles are not single-base substitutions and were left out\n", (unsigned long long)not_snv);
    if (T.orphans) std::fprintf(stderr, "[WARN] %llu features have no Parent and belong to no transcript\n", (unsigned long long)T.orphans);
    if (T.mixed) std::fprintf(stderr, "[WARN] %llu transcripts were dropped: their members lie on more than one seqid or strand\n", (unsigned long long)T.mixed);
    if (n_unservable)
        std::fprintf(stderr, "[WARN] %llu transcripts were dropped: a member lies on a seqid the FASTA file lacks or beyond its sequence\n", (unsigned long long)n_unservable);
    timer.lap("Transcripts");

    // the alleles' rows; a CHROM the index does not know is left out
    std::vector<uint32_t> arows;
    std::vector<uint8_t> abytes;  // --indels: R' then A' of every row
    arows.reserve(args.indels ? 6 * alleles_any.size() : 3 * alleles.size());
    if (args.indels) {
        size_t kept = 0;
        std::string_view last;
        uint32_t last_fa = 0;
        bool last_known = false, have = false;
        for (const et::AlleleAny &a : alleles_any) {
            if (!have || a.chrom != last) {
                const auto it = index_data.seqid_to_num.find(std::string(a.chrom));
                last = a.chrom, have = true;
                last_known = it != index_data.seqid_to_num.end() && it->second < fa_of_seqid.size();
                last_fa = last_known ? fa_of_seqid[it->second] : 0;
            }
            if (!last_known) {
                ++no_chrom;
                continue;
            }
            et::append_row_any(arows, abytes, a, last_fa);
            alleles_any[kept++] = a;
        }
        alleles_any.resize(kept);
    } else {
        size_t kept = 0;
        std::string_view last;
        uint32_t last_fa = 0;
        bool last_known = false, have = false;
        for (const et::Allele &a : alleles) {
            if (!have || a.chrom != last) {
                const auto it = index_data.seqid_to_num.find(std::string(a.chrom));
                last = a.chrom, have = true;
                last_known = it != index_data.seqid_to_num.end() && it->second < fa_of_seqid.size();
                last_fa = last_known ? fa_of_seqid[it->second] : 0;
            }
            if (!last_known) {
                ++no_chrom;
                continue;
            }
            arows.insert(arows.end(), {last_fa, a.x, static_cast<uint32_t>(a.ref) | static_cast<uint32_t>(a.alt) << 8});
            alleles[kept++] = a;
        }
        alleles.resize(kept);
    }
    if (no_chrom) std::fprintf(stderr, "[WARN] %llu alleles lie on a seqid the index does not have and were left out\n", (unsigned long long)no_chrom);

    // the chunks: chunk k + 1 is classified while chunk k is formatted
    const uint64_t n = args.indels ? alleles_any.size() : alleles.size(), n_chunks = (n + chunk - 1) / chunk;
    // (--indels: a chunk's bytes are those from its first row's offset to the next chunk's; the rows go with offsets into them)
    const auto row_off = [&](uint64_t i) { return i < n ? (static_cast<uint64_t>(arows[6 * i + 4]) | static_cast<uint64_t>(arows[6 * i + 5]) << 32) : static_cast<uint64_t>(abytes.size()); };
    std::vector<uint32_t> chunk_rows[2];
    Output out(args.common.output);
    std::string buf = et::kHeader;
    et::Summary sum;
    et::SummaryAll sum_all;
    uint64_t n_pairs = 0;
    double format_ms = 0;
    const auto start = [&](uint64_t k) {
        const uint64_t lo = k * chunk, m = std::min(chunk, n - lo);
        if (args.indels) {
            const uint64_t b0 = row_off(lo), b1 = row_off(lo + m);
            std::vector<uint32_t> &rows6 = chunk_rows[k & 1];
            rows6.assign(arows.begin() + 6 * lo, arows.begin() + 6 * (lo + m));
            for (uint64_t i = 0; i < m; ++i) {
                const uint64_t rel = row_off(lo + i) - b0;
                rows6[6 * i + 4] = static_cast<uint32_t>(rel), rows6[6 * i + 5] = static_cast<uint32_t>(rel >> 32);
            }
            if (gffx_hip_effect_run_any_start(eff.get(), static_cast<int>(k & 1), rows6.data(), m, abytes.data() + b0, b1 - b0) != GFFX_OK) hip_fail("gffx_hip_effect_run_any_start");
            return;
        }
        if (gffx_hip_effect_run_start(eff.get(), static_cast<int>(k & 1), arows.data() + 3 * lo, m) != GFFX_OK) hip_fail("gffx_hip_effect_run_start");
    };
    if (n_chunks) start(0);
    for (uint64_t k = 0; k < n_chunks; ++k) {
        const uint64_t *off = nullptr;
        const uint8_t *rm = nullptr, *rec = nullptr;
        uint64_t pairs = 0;
        if (gffx_hip_effect_run_wait(eff.get(), static_cast<int>(k & 1), &off, &rm, &rec, &pairs) != GFFX_OK) hip_fail("gffx_hip_effect_run_wait");
        if (k + 1 < n_chunks) start(k + 1);
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t lo = k * chunk, m = std::min(chunk, n - lo);
        const rules::Record *records = reinterpret_cast<const rules::Record *>(rec);
        // the chunk's lines on -t threads, each part into a buffer and a summary of its own; written in order
        const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, m / 4096 + 1));
        std::vector<std::string> text(parts);
        std::vector<et::Summary> part_sum(parts);
        std::vector<et::SummaryAll> part_sum_all(args.indels ? parts : 0);
        parallel_for(parts, parts, [&](size_t p) {
            for (uint64_t i = m * p / parts; i < m * (p + 1) / parts; ++i) {
                if (args.indels) et::format_allele_any(text[p], part_sum_all[p], alleles_any[lo + i], records + off[i], off[i + 1] - off[i], rm[i], T.names, T.strand);
                else et::format_allele(text[p], part_sum[p], alleles[lo + i], records + off[i], off[i + 1] - off[i], rm[i], T.names, T.strand);
            }
        });
        for (size_t p = 0; p < parts; ++p) {
            if (buf.size() + text[p].size() >= (1u << 20)) {
                out.write(buf);
                buf.clear();
            }
            if (text[p].size() >= (1u << 20)) out.write(text[p]);
            else buf += text[p];
            for (uint32_t c = 0; c < rules::kClasses; ++c) sum.alleles[c] += part_sum[p].alleles[c], sum.pairs[c] += part_sum[p].pairs[c];
            if (args.indels) sum_all.add(part_sum_all[p]);
        }
        n_pairs += pairs;
        format_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    out.write(buf);
    out.close();
    if (args.summary) {
        Output s(args.summary);
        s.write(args.indels ? sum_all.text() : sum.text());
        s.close();
    }
    double build_ms = 0, pairs_ms = 0, classify_ms = 0;
    (void)gffx_hip_effect_stage_ms(eff.get(), &build_ms, &pairs_ms, &classify_ms);
    if (verbose)
        std::fprintf(stderr, "[INFO] effect: %zu member lines, %zu transcripts (%llu kept), %llu alleles, %llu pairs in %llu chunks: build kernels %.3f ms, pair kernels %.3f ms, classify kernels %.3f ms\n",
                     G, R, (unsigned long long)n_kept, (unsigned long long)n, (unsigned long long)n_pairs, (unsigned long long)n_chunks, build_ms, pairs_ms, classify_ms);
    timer.lap("Classify and write");
    g_run_stats.count("member_lines", static_cast<double>(G));
    g_run_stats.count("transcripts", static_cast<double>(R));
    g_run_stats.count("transcripts_kept", static_cast<double>(n_kept));
    g_run_stats.count("alleles", static_cast<double>(n));
    g_run_stats.count("alleles_not_snv", static_cast<double>(not_snv));
    if (args.indels) {
        g_run_stats.count("alleles_other_bytes", static_cast<double>(left_out[0]));
        g_run_stats.count("alleles_too_long", static_cast<double>(left_out[1]));
        g_run_stats.count("alleles_equal_to_ref", static_cast<double>(left_out[2]));
        g_run_stats.count("alleles_insertion_at_1", static_cast<double>(left_out[3]));
    }
    g_run_stats.count("alleles_no_seqid", static_cast<double>(no_chrom));
    g_run_stats.count("pairs", static_cast<double>(n_pairs));
    g_run_stats.count("chunks", static_cast<double>(n_chunks));
    g_run_stats.count("build_kernels_ms", build_ms);
    g_run_stats.count("pair_kernels_ms", pairs_ms);
    g_run_stats.count("classify_kernels_ms", classify_ms);
    g_run_stats.count("format_ms", format_ms);
    g_run_stats.write("effect", timer.total());
}

}  // namespace gffx::commands::effect
