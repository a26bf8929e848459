// seq.cpp -- `gffx seq` above the C-ABI (an addition: the reference has no such command): the bases under the lines
// of the -T types, or with -j the spliced sequence of every Parent, from a plain FASTA, optionally translated, as wrapped
// FASTA.  device/seq_core.hpp has the definition.  The FASTA goes to the device as it is (gffx_hip_genome_*: lines found,
// classified and packed into one arena there).  The features are taken as `meta` takes them (layer_rows.hpp), with strand, ID,
// phase and Parent read from the mapped text on -t threads (feature_rows.hpp).  Grouping by Parent is string work and stays
// here: the records are numbered by first appearance, the mixed ones dropped, the headers formatted; the device gets numeric
// rows (gffx_hip_seq_*), sorts them, sizes the bodies and emits them in slices of GFFX_SEQ_OUT_BYTES through two pinned
// buffers, so that slice k is written while slice k + 1 is produced.  The headers are interleaved while writing.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../device/seq_core.hpp"
#include "feature_rows.hpp"
#include "intersect_internal.hpp"
#include "layer_rows.hpp"
#include "table_output.hpp"

namespace gffx::commands::seq {

namespace {

using GenomeHandle = Handle<gffx_hip_genome, gffx_hip_genome_destroy>;
using SeqHandle = Handle<gffx_hip_seq, gffx_hip_seq_destroy>;

// GFFX_SEQ_OUT_BYTES: a positive decimal number (at most 1 GiB is taken); anything else is ignored
uint64_t slice_bytes_from_env() {
    const char *e = std::getenv("GFFX_SEQ_OUT_BYTES");
    if (e && *e >= '0' && *e <= '9') {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end && !*end && v > 0) return std::min<unsigned long long>(v, 1ull << 30);
    }
    return 256ull << 20;
}

struct Record {  // -j: what the header says of a Parent, and what decides its drop
    std::string_view name;
    uint32_t seq = 0, min_start = 0, max_end = 0, k = 0;
    char strand = '.';
    bool minus = false, mixed = false;
    // the first segment in the direction of transcription: the smallest (start, line order) on plus, the largest on minus
    uint32_t lead_start = 0;
    char lead_phase = '.';
};

}  // namespace

void run(const SeqArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    const size_t threads = args.common.effective_threads();
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    timer.lap("Loading tree index");
    const MappedFile fasta = map_file_or(args.fasta, "Cannot open FASTA file: \"" + args.fasta + "\"");
    if (fasta.size() >= 2 && fasta.data()[0] == 0x1f && fasta.data()[1] == 0x8b) throw Error("compressed FASTA is not read: decompress \"" + args.fasta + "\" first");
    DeviceWarmup warm(args.device);

    // the features, in file order
    std::vector<uint32_t> rows;  // (layer, seqid, start - 1, end)
    std::vector<feature_rows::SeqFields> fields;
    const MappedFile gff = map_file_or(args.common.input, "Cannot open GFF file: \"" + args.common.input + "\"");
    uint64_t skipped = 0;
    {
        std::vector<uint64_t> per_type(args.types.size(), 0), line_start;
        layer_rows::collect(args.common.input, args.types, index_data.seqid_to_num, threads, verbose, rows, per_type, skipped, nullptr, &line_start);
        const std::string_view text = gff.view();
        const size_t G = rows.size() / 4;
        fields.resize(G);
        const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, G / 4096 + 1));
        parallel_for(parts, parts, [&](size_t p) {
            for (size_t i = G * p / parts; i < G * (p + 1) / parts; ++i) fields[i] = feature_rows::read_seq_fields(text, line_start[i]);
        });
        layer_rows::report(args.common.input, args.types, per_type, "", nullptr, skipped);
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
    std::vector<uint32_t> fa_len(std::max<uint32_t>(n_fa, 1));
    std::vector<uint32_t> fa_of_seqid(index_data.num_to_seqid.size(), UINT32_MAX);
    {
        std::vector<uint8_t> names(std::max<uint64_t>(gffx_hip_genome_name_bytes(genome.get()), 1));
        std::vector<uint64_t> name_off(n_fa + 1), seq_off(n_fa + 1);
        if (gffx_hip_genome_copy_names(genome.get(), names.data(), name_off.data()) != GFFX_OK) hip_fail("gffx_hip_genome_copy_names");
        if (gffx_hip_genome_copy_seqs(genome.get(), seq_off.data(), fa_len.data()) != GFFX_OK) hip_fail("gffx_hip_genome_copy_seqs");
        for (uint32_t g = 0; g < n_fa; ++g) {
            const auto it = index_data.seqid_to_num.find(std::string(reinterpret_cast<const char *>(names.data()) + name_off[g], name_off[g + 1] - name_off[g]));
            if (it != index_data.seqid_to_num.end() && it->second < fa_of_seqid.size()) fa_of_seqid[it->second] = g;
        }
    }
    double lines_ms = 0, pack_ms = 0;
    (void)gffx_hip_genome_stage_ms(genome.get(), &lines_ms, &pack_ms);
    if (verbose)
        std::fprintf(stderr, "[INFO] seq: %u sequences, %llu bases from %zu bytes of FASTA: line kernels %.3f ms, pack kernels %.3f ms\n", n_fa,
                     (unsigned long long)gffx_hip_genome_n_bases(genome.get()), fasta.size(), lines_ms, pack_ms);
    timer.lap("FASTA upload and pack");

    // the records and the device's rows (record, sequence number, start - 1, end)
    uint64_t no_seq = 0, beyond = 0, orphans = 0, n_mixed = 0;
    std::vector<uint32_t> dev_rows;
    std::vector<uint8_t> rec_flags;
    std::vector<Record> recs;  // -j only
    dev_rows.reserve(rows.size());
    for (size_t i = 0; i < G; ++i) {
        const uint32_t fa = fa_of_seqid[rows[4 * i + 1]];
        if (fa == UINT32_MAX) ++no_seq;
        else if (rows[4 * i + 3] > fa_len[fa]) ++beyond;
    }
    if (!args.join) {
        rec_flags.resize(G);
        for (size_t i = 0; i < G; ++i) {
            dev_rows.insert(dev_rows.end(), {static_cast<uint32_t>(i), fa_of_seqid[rows[4 * i + 1]], rows[4 * i + 2], rows[4 * i + 3]});
            rec_flags[i] = static_cast<uint8_t>((fields[i].si.minus ? GFFX_SEQ_MINUS : 0) | (gffx::seq::phase_skip(static_cast<uint8_t>(fields[i].phase)) << 1));
        }
    } else {
        std::unordered_map<std::string_view, uint32_t> by_name;
        for (size_t i = 0; i < G; ++i) {
            const feature_rows::SeqFields &f = fields[i];
            const uint32_t seq = rows[4 * i + 1], start0 = rows[4 * i + 2], end = rows[4 * i + 3];
            bool any = false;
            feature_rows::for_each_parent(f.parent, [&](std::string_view name) {
                any = true;
                const auto [it, fresh] = by_name.emplace(name, static_cast<uint32_t>(recs.size()));
                if (fresh) {
                    Record r;
                    r.name = name, r.seq = seq, r.min_start = start0 + 1, r.max_end = end, r.strand = f.strand, r.minus = f.si.minus;
                    r.lead_start = start0, r.lead_phase = f.phase;
                    recs.push_back(r);
                }
                Record &r = recs[it->second];
                if (r.seq != seq || r.minus != f.si.minus) r.mixed = true;
                r.min_start = std::min(r.min_start, start0 + 1), r.max_end = std::max(r.max_end, end), ++r.k;
                // (members come in line order: a later one with the same start follows in the order, so it leads on minus only)
                if (r.minus ? start0 >= r.lead_start : start0 < r.lead_start) r.lead_start = start0, r.lead_phase = f.phase;
                dev_rows.insert(dev_rows.end(), {it->second, fa_of_seqid[seq], start0, end});
            });
            orphans += !any;
        }
        rec_flags.resize(recs.size());
        for (size_t r = 0; r < recs.size(); ++r) {
            n_mixed += recs[r].mixed;
            rec_flags[r] = static_cast<uint8_t>((recs[r].minus ? GFFX_SEQ_MINUS : 0) | (gffx::seq::phase_skip(static_cast<uint8_t>(recs[r].lead_phase)) << 1) |
                                                (recs[r].mixed ? GFFX_SEQ_DROPPED : 0));
        }
    }
    const size_t R = rec_flags.size();
    SeqHandle plan;
    if (gffx_hip_seq_create(genome.get(), dev_rows.size() / 4, dev_rows.data(), R, rec_flags.data(), args.translate ? 1 : 0, args.width, OutPtr(plan)) != GFFX_OK)
        hip_fail("gffx_hip_seq_create");
    std::vector<uint64_t> body_off(R + 1, 0);
    std::vector<uint8_t> dropped(std::max<size_t>(R, 1), 0);
    if (gffx_hip_seq_copy_offsets(plan.get(), body_off.data(), dropped.data()) != GFFX_OK) hip_fail("gffx_hip_seq_copy_offsets");
    uint64_t n_unservable = 0, n_out = 0;
    for (size_t r = 0; r < R; ++r) {
        n_unservable += dropped[r] && !(rec_flags[r] & GFFX_SEQ_DROPPED);
        n_out += !dropped[r];
    }
    if (no_seq) std::fprintf(stderr, "[WARN] %llu features lie on a seqid the FASTA file lacks\n", (unsigned long long)no_seq);
    if (beyond) std::fprintf(stderr, "[WARN] %llu features reach beyond the end of their sequence\n", (unsigned long long)beyond);
    if (args.join && orphans) std::fprintf(stderr, "[WARN] %llu features have no Parent and belong to no record\n", (unsigned long long)orphans);
    if (args.join && n_mixed) std::fprintf(stderr, "[WARN] %llu records were dropped: their members lie on more than one seqid or strand\n", (unsigned long long)n_mixed);
    if (args.join && n_unservable)
        std::fprintf(stderr, "[WARN] %llu records were dropped: a member lies on a seqid the FASTA file lacks or beyond its sequence\n", (unsigned long long)n_unservable);
    timer.lap("Plan");

    // the slices: slice k + 1 is produced while slice k is written, the headers interleaved
    const uint64_t total = body_off[R], slice = slice_bytes_from_env();
    const uint64_t n_slices = (total + slice - 1) / slice;
    Output out(args.common.output);
    std::string buf;
    const auto flush = [&](bool force) {
        if (!force && buf.size() < (1u << 20)) return;
        out.write(buf);
        buf.clear();
    };
    char num[96];
    const auto header = [&](size_t r) {
        buf.push_back('>');
        if (args.join) {
            const Record &x = recs[r];
            buf.append(x.name);
            buf.push_back(' ');
            buf.append(index_data.num_to_seqid[x.seq]);
            buf.append(num, std::snprintf(num, sizeof num, ":%u-%u(%c) segments=%u\n", x.min_start, x.max_end, x.strand, x.k));
        } else {
            buf.append(fields[r].si.id);
            buf.push_back(' ');
            buf.append(index_data.num_to_seqid[rows[4 * r + 1]]);
            buf.append(num, std::snprintf(num, sizeof num, ":%u-%u(%c)\n", rows[4 * r + 2] + 1, rows[4 * r + 3], fields[r].strand));
        }
    };
    size_t r = 0;          // the next record to open
    uint64_t cur_end = 0;  // where the open record's body ends
    double write_ms = 0;
    const auto start = [&](uint64_t k) {
        const uint64_t lo = k * slice, n = std::min(slice, total - lo);
        if (gffx_hip_seq_emit_start(plan.get(), static_cast<int>(k & 1), lo, n) != GFFX_OK) hip_fail("gffx_hip_seq_emit_start");
    };
    if (n_slices) start(0);
    for (uint64_t k = 0; k < n_slices; ++k) {
        const uint8_t *data = nullptr;
        if (gffx_hip_seq_emit_wait(plan.get(), static_cast<int>(k & 1), &data) != GFFX_OK) hip_fail("gffx_hip_seq_emit_wait");
        if (k + 1 < n_slices) start(k + 1);
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t lo = k * slice, hi = std::min(total, lo + slice);
        for (uint64_t p = lo; p < hi;) {
            if (p == cur_end) {
                while (r < R) {  // the headers up to the record that owns byte p
                    if (!dropped[r]) header(r);
                    cur_end = body_off[r + 1];
                    if (body_off[++r] > p) break;
                }
            }
            const uint64_t n = std::min(hi, cur_end) - p;
            buf.append(reinterpret_cast<const char *>(data) + (p - lo), n);
            p += n;
            flush(false);
        }
        write_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    for (; r < R; ++r)  // records without a body behind the last byte
        if (!dropped[r]) header(r);
    flush(true);
    out.close();
    double plan_ms = 0, emit_ms = 0;
    (void)gffx_hip_seq_stage_ms(plan.get(), &plan_ms, &emit_ms);
    if (verbose)
        std::fprintf(stderr, "[INFO] seq: %zu features, %zu records, %llu written, %llu body bytes in %llu slices: plan kernels %.3f ms, emit kernels %.3f ms\n", G, R,
                     (unsigned long long)n_out, (unsigned long long)total, (unsigned long long)n_slices, plan_ms, emit_ms);
    timer.lap("Emit and write");
    g_run_stats.count("features", static_cast<double>(G));
    g_run_stats.count("records", static_cast<double>(R));
    g_run_stats.count("records_written", static_cast<double>(n_out));
    g_run_stats.count("body_bytes", static_cast<double>(total));
    g_run_stats.count("slices", static_cast<double>(n_slices));
    g_run_stats.count("fasta_bytes", static_cast<double>(fasta.size()));
    g_run_stats.count("genome_bases", static_cast<double>(gffx_hip_genome_n_bases(genome.get())));
    g_run_stats.count("line_kernels_ms", lines_ms);
    g_run_stats.count("pack_kernels_ms", pack_ms);
    g_run_stats.count("plan_kernels_ms", plan_ms);
    g_run_stats.count("emit_kernels_ms", emit_ms);
    g_run_stats.count("write_ms", write_ms);
    g_run_stats.write("seq", timer.total());
}

}  // namespace gffx::commands::seq
