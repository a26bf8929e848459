// meta.cpp -- `gffx meta` above the C-ABI (an addition: the reference has no such command): the depth of the source
// rows around the features of a GFF file, column by column in the direction of transcription and summed over the features --
// the TSS profile, the scaled gene body.  The features are the lines of the -T types, taken as `annotate` takes its layer rows
// (layer_rows.hpp) plus their strand and ID from the text (feature_rows.hpp); device/meta_core.hpp has the rule of the columns.
// The source goes the way of `coverage -s`: read_source_rows, then batches through a region store per device, round robin with
// --gpus N; every device folds its batches into a pileup without segments whose second consumer holds the features
// (gffx_hip_pileup_meta_*).  Only B column totals per device come back (and the features x B matrix with --matrix); they are
// integers and are added here, so the output depends neither on the batch size nor on the device count nor on -t.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "feature_rows.hpp"
#include "genome_file.hpp"
#include "intersect_internal.hpp"
#include "layer_rows.hpp"
#include "source_read.hpp"
#include "table_output.hpp"

namespace gffx::commands::meta {

namespace {

// column j of the layout: its part and the offsets it spans (relative to the anchor, to the 5' end, in body columns, to the 3' end)
void append_column_label(std::string &s, const gffx_hip_meta_layout &y, uint64_t j) {
    char buf[96];
    const long long bin = y.bin, n_up = y.up / y.bin;
    const long long k = static_cast<long long>(j);
    if (y.mode == 0)
        s.append(buf, std::snprintf(buf, sizeof buf, "point\t%lld\t%lld", k * bin - y.up, (k + 1) * bin - y.up));
    else if (k < n_up)
        s.append(buf, std::snprintf(buf, sizeof buf, "up\t%lld\t%lld", k * bin - y.up, (k + 1) * bin - y.up));
    else if (k < n_up + y.body_bins)
        s.append(buf, std::snprintf(buf, sizeof buf, "body\t%lld\t%lld", k - n_up, k - n_up + 1));
    else
        s.append(buf, std::snprintf(buf, sizeof buf, "down\t%lld\t%lld", (k - n_up - y.body_bins) * bin, (k - n_up - y.body_bins + 1) * bin));
}

}  // namespace

void run(const MetaArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    const size_t threads = args.common.effective_threads();
    const gffx_hip_meta_layout &layout = args.layout;
    const uint64_t B = gffx_hip_pileup_meta_columns(&layout);
    // (what needs no device comes first: a bad -g file ends the run before the device is touched)
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    const uint32_t n_seq = static_cast<uint32_t>(index_data.num_to_seqid.size());
    timer.lap("Loading tree index");
    std::vector<uint32_t> seq_len;
    if (args.genome) seq_len = read_genome(*args.genome, index_data.num_to_seqid, index_data.seqid_to_num);
    DeviceWarmup warm(args.device);

    // the features, in file order
    std::vector<uint32_t> f_seq, f_start, f_end;
    std::vector<uint8_t> f_minus;
    std::vector<std::string> f_id;
    uint64_t skipped = 0, unstranded = 0;
    {
        std::vector<uint32_t> rows;
        std::vector<uint64_t> per_type(args.types.size(), 0), line_start;
        layer_rows::collect(args.common.input, args.types, index_data.seqid_to_num, threads, verbose, rows, per_type, skipped, nullptr, &line_start);
        const MappedFile gff = map_file_or(args.common.input, "Cannot open GFF file: \"" + args.common.input + "\"");
        const std::string_view text = gff.view();
        const size_t G = rows.size() / 4;
        f_seq.resize(G), f_start.resize(G), f_end.resize(G), f_minus.resize(G), f_id.resize(G);
        for (size_t i = 0; i < G; ++i) {
            const feature_rows::StrandId si = feature_rows::read_strand_id(text, line_start[i]);
            f_seq[i] = rows[4 * i + 1], f_start[i] = rows[4 * i + 2], f_end[i] = rows[4 * i + 3];
            f_minus[i] = si.minus ? 1 : 0;
            f_id[i].assign(si.id);
            unstranded += !si.stranded;
        }
        layer_rows::report(args.common.input, args.types, per_type, "", nullptr, skipped);
        if (unstranded)
            std::fprintf(stderr, "[WARN] %llu features have neither '+' nor '-' in column 7 and were taken as '+'\n", (unsigned long long)unstranded);
        if (verbose)
            std::fprintf(stderr, "[INFO] meta: %zu features, %llu columns; %llu lines skipped (a seqid the index does not know)\n", G, (unsigned long long)B,
                         (unsigned long long)skipped);
        if (verbose && !args.genome)
            std::fprintf(stderr, "[INFO] meta: no -g: columns are cut at 0 only, `length` counts bases beyond a chromosome's end\n");
    }
    const size_t G = f_seq.size();
    timer.lap("Features from the line table");

    const depth::SourceKind kind = depth::source_kind(args.source);
    const depth::SourceRows src = depth::read_source_rows(kind, args.source, index_data.seqid_to_num, threads, args.device, verbose, warm);
    if (verbose) std::fprintf(stderr, "[INFO] %zu %s rows kept\n", src.n_rows, depth::source_label(kind));
    timer.lap(depth::source_lap(kind, false));

    warm.wait();
    DeviceSet devs = DeviceSet::resolve(args.device, args.gpus);
    const size_t D = devs.size();
    const bool keep_matrix = args.matrix.has_value();
    struct PerDevice {
        RegionsHandle store;
        PileupHandle p;
        std::vector<uint64_t> col[3], matrix;  // bases, length, features
        uint64_t rows = 0, folds = 0;
        double fold_ms = 0, meta_ms = 0;
    };
    std::vector<PerDevice> pd(D);
    const size_t kBatch = source::batch_rows_from_env("GFFX_META_BATCH_ROWS");
    const size_t cap = std::max<size_t>(std::min(src.n_rows, kBatch), 1);
    parallel_for(D, D, [&](size_t d) {
        PerDevice &P = pd[d];
        if (gffx_hip_regions_create(devs[d], 0, cap, 0, OutPtr(P.store)) != GFFX_OK) hip_fail("gffx_hip_regions_create");
        if (gffx_hip_pileup_create(devs[d], n_seq, 0, nullptr, nullptr, nullptr, OutPtr(P.p)) != GFFX_OK) hip_fail("gffx_hip_pileup_create");
        if (gffx_hip_pileup_meta_set(P.p.get(), G, f_seq.data(), f_start.data(), f_end.data(), f_minus.data(), args.genome ? seq_len.data() : nullptr, &layout,
                                     keep_matrix ? 1 : 0) != GFFX_OK)
            hip_fail("gffx_hip_pileup_meta_set");
        // the batch resident in slot k into the pileup: returns when the rows are read, the fold goes on behind
        auto submit = [&](int k, size_t n) {
            if (gffx_hip_pileup_add_store(P.p.get(), P.store.get(), k, 0, n) != GFFX_OK) hip_fail("gffx_hip_pileup_add_store");
        };
        const size_t fill_threads = std::max<size_t>(1, std::min<size_t>(threads / D, 8));
        P.rows = depth::run_row_batches(src, P.store.get(), d, D, kBatch, fill_threads, submit, [](int) {});
        for (auto &c : P.col) c.assign(std::max<uint64_t>(B, 1), 0);
        if (keep_matrix) P.matrix.assign(std::max<uint64_t>(G * B, 1), 0);
        if (gffx_hip_pileup_meta_copy(P.p.get(), P.col[0].data(), P.col[1].data(), P.col[2].data(), keep_matrix ? P.matrix.data() : nullptr) != GFFX_OK)
            hip_fail("gffx_hip_pileup_meta_copy");
        if (gffx_hip_pileup_stats(P.p.get(), &P.fold_ms, nullptr, &P.folds) != GFFX_OK) hip_fail("gffx_hip_pileup_stats");
        if (gffx_hip_pileup_meta_ms(P.p.get(), &P.meta_ms) != GFFX_OK) hip_fail("gffx_hip_pileup_meta_ms");
    });
    // the devices' totals added as integers; length and features are the features' own: every device has the same
    uint64_t rows = 0, folds = 0;
    double fold_ms = 0, meta_ms = 0;
    for (size_t d = 0; d < D; ++d) {
        rows += pd[d].rows, folds += pd[d].folds, fold_ms += pd[d].fold_ms, meta_ms += pd[d].meta_ms;
        if (!d) continue;
        for (uint64_t j = 0; j < B; ++j) pd[0].col[0][j] += pd[d].col[0][j];
        if (keep_matrix)
            for (uint64_t x = 0; x < G * B; ++x) pd[0].matrix[x] += pd[d].matrix[x];
    }
    if (verbose)
        std::fprintf(stderr, "[INFO] meta: %llu rows in %llu folds on %zu devices: fold kernels %.3f ms, meta kernel %.3f ms\n", (unsigned long long)rows,
                     (unsigned long long)folds, D, fold_ms, meta_ms);
    timer.lap("Rows through the device");

    {
        Output out(args.common.output);
        std::string s = "#column\tpart\tfrom\tto\tfeatures\tbases\tlength\tmean_depth\n";
        char buf[128];
        for (uint64_t j = 0; j < B; ++j) {
            const uint64_t bases = pd[0].col[0][j], len = pd[0].col[1][j], features = pd[0].col[2][j];
            s.append(buf, std::snprintf(buf, sizeof buf, "%llu\t", (unsigned long long)j));
            append_column_label(s, layout, j);
            s.append(buf, std::snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%.6f\n", (unsigned long long)features, (unsigned long long)bases, (unsigned long long)len,
                                        len > 0 ? static_cast<double>(bases) / static_cast<double>(len) : 0.0));
        }
        out.write(s);
        out.close();
    }
    if (args.matrix) {
        Output mf(args.matrix);
        std::string s = "#chr\tstart\tend\tid\tstrand";
        char buf[32];
        for (uint64_t j = 0; j < B; ++j) s.append(buf, std::snprintf(buf, sizeof buf, "\tc%llu", (unsigned long long)j));
        s.push_back('\n');
        for (size_t i = 0; i < G; ++i) {
            s.append(index_data.num_to_seqid[f_seq[i]]);
            s.append(buf, std::snprintf(buf, sizeof buf, "\t%u\t%u\t", f_start[i], f_end[i]));
            s.append(f_id[i]);
            s.append(f_minus[i] ? "\t-" : "\t+");
            for (uint64_t j = 0; j < B; ++j) s.append(buf, std::snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)pd[0].matrix[i * B + j]));
            s.push_back('\n');
            if (s.size() > (1u << 20)) mf.write(s), s.clear();
        }
        mf.write(s);
        mf.close();
    }
    timer.lap("Writing");
    g_run_stats.count("gpus", static_cast<double>(D));
    g_run_stats.count("rows", static_cast<double>(rows));
    g_run_stats.count("features", static_cast<double>(G));
    g_run_stats.count("columns", static_cast<double>(B));
    g_run_stats.count("unstranded", static_cast<double>(unstranded));
    g_run_stats.count("pileup_folds", static_cast<double>(folds));
    g_run_stats.count("pileup_kernels_ms", fold_ms);
    g_run_stats.count("meta_kernel_ms", meta_ms);
    g_run_stats.write("meta", timer.total());
}

}  // namespace gffx::commands::meta
