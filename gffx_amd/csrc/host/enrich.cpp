// enrich.cpp -- `gffx enrich` above the C-ABI (an addition: the reference has no such command): a permutation test
// of the regions of a BED file against the feature classes of `gffx annotate`.  Every region is moved to a random place on its
// own seqid -n times (device/enrich_core.hpp has the random numbers and the placement rule); per class the observed bases and
// region counts are compared with the permutations'.  The class map is built as `annotate` builds it (layer_rows.hpp), the BED
// file streams chunk by chunk through a region store, and the device keeps only two (N + 1) x (T + 1) matrices of integer
// sums (gffx_hip_classmap_perm_*): the output depends neither on the chunk size nor on -t.
#include <cmath>
#include <cstdio>

#include "genome_file.hpp"
#include "layer_rows.hpp"
#include "region_feed.hpp"
#include "table_output.hpp"

namespace gffx::commands::enrich {

namespace {

void append_float(std::string &s, double v) {
    char buf[48];
    if (std::isnan(v))
        s.append("\tnan");  // (never "-nan")
    else
        s.append(buf, std::snprintf(buf, sizeof buf, "\t%.6g", v));
}

// one output line: X[0] observed, X[1 .. N] the permutations
void append_stats(std::string &s, const std::string &name, const char *quantity, const std::vector<uint64_t> &X) {
    const size_t N = X.size() - 1;
    const double nan = std::nan(""), obs = static_cast<double>(X[0]);
    double sum = 0, ss = 0;
    uint64_t n_ge = 0, n_le = 0;
    for (size_t p = 1; p <= N; ++p) sum += static_cast<double>(X[p]), n_ge += X[p] >= X[0], n_le += X[p] <= X[0];
    // (permutations that all give one value: mean is that value and sd is 0 exactly, whatever N x value rounds to in a double)
    bool all_equal = true;
    for (size_t p = 2; p <= N; ++p) all_equal &= X[p] == X[1];
    const double mean = all_equal ? static_cast<double>(X[1]) : sum / static_cast<double>(N);
    for (size_t p = 1; p <= N && !all_equal; ++p) ss += (static_cast<double>(X[p]) - mean) * (static_cast<double>(X[p]) - mean);
    const double sd = N > 1 ? std::sqrt(ss / static_cast<double>(N - 1)) : nan;
    const double z = (N > 1 && sd != 0) ? (obs - mean) / sd : nan, fold = mean != 0 ? obs / mean : nan;
    char buf[96];
    s.append(name).append("\t").append(quantity);
    s.append(buf, std::snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)X[0]));
    append_float(s, mean), append_float(s, sd), append_float(s, z), append_float(s, fold);
    s.append(buf, std::snprintf(buf, sizeof buf, "\t%llu\t%llu", (unsigned long long)n_ge, (unsigned long long)n_le));
    append_float(s, static_cast<double>(n_ge + 1) / static_cast<double>(N + 1));
    append_float(s, static_cast<double>(n_le + 1) / static_cast<double>(N + 1));
    s.push_back('\n');
}

}  // namespace

void run(const EnrichArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    const size_t threads = args.common.effective_threads();
    const std::vector<std::string> &layers = args.layers;
    const uint32_t T = static_cast<uint32_t>(layers.size()), N = args.n_perm;
    // (what needs no device comes first: a bad -g file ends the run before the device is touched)
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    const uint32_t n_seq = static_cast<uint32_t>(index_data.num_to_seqid.size());
    timer.lap("Loading tree index");
    std::vector<uint32_t> seq_len(n_seq, 0);
    if (args.genome) seq_len = read_genome(*args.genome, index_data.num_to_seqid, index_data.seqid_to_num);
    DeviceWarmup warm(args.device);
    std::vector<uint32_t> rows, seq_end(n_seq, 0);
    std::vector<uint64_t> per_layer(T, 0);
    uint64_t skipped = 0;
    layer_rows::collect(args.common.input, layers, index_data.seqid_to_num, threads, verbose, rows, per_layer, skipped, &seq_end);
    if (!args.genome) {
        seq_len = seq_end;
        if (verbose) std::fprintf(stderr, "[INFO] enrich: no -g: a seqid's length is the largest end of its lines, which understates the chromosome\n");
    }
    layer_rows::report(args.common.input, layers, per_layer, ": its class is empty", verbose ? "enrich" : nullptr, skipped);
    timer.lap("Layer rows from the line table");
    RegionFeed feed(std::nullopt, args.bed, index_data, args.common);
    warm.wait();
    feed.open(args.device, verbose, timer);
    const ClassMapHandle h = layer_rows::build_class_map(args.device, n_seq, T, rows);
    if (gffx_hip_classmap_perm_begin(h.get(), seq_len.data(), N, args.seed) != GFFX_OK) hip_fail("gffx_hip_classmap_perm_begin");
    feed.create_store(args.device);
    timer.lap("Class map + buffers");
    uint64_t regions = 0;
    double kernel_ms = 0;
    // n rows sit in staging buffer k: to the store and into the totals; `regions` is the global row of the first of them
    feed.run(threads, [&](gffx_hip_regions *store, int k, const uint32_t *, uint64_t n) {
        if (gffx_hip_regions_append(store, k, n) != GFFX_OK) hip_fail("gffx_hip_regions_append");
        if (gffx_hip_classmap_perm_run_store(h.get(), store, k, 0, n, regions) != GFFX_OK) hip_fail("gffx_hip_classmap_perm_run_store");
        if (gffx_hip_classmap_perm_wait(h.get()) != GFFX_OK) hip_fail("gffx_hip_classmap_perm_wait");
        double ms = 0;
        if (gffx_hip_classmap_perm_last_kernel_ms(h.get(), &ms) == GFFX_OK) kernel_ms += ms;
        regions += n;
    });
    const size_t cells = (static_cast<size_t>(N) + 1) * (T + 1);
    std::vector<uint64_t> B(cells, 0), R(cells, 0);
    uint64_t unplaced = 0;
    if (gffx_hip_classmap_perm_wait(h.get()) != GFFX_OK) hip_fail("gffx_hip_classmap_perm_wait");
    if (gffx_hip_classmap_perm_copy_totals(h.get(), B.data(), R.data(), &unplaced) != GFFX_OK) hip_fail("gffx_hip_classmap_perm_copy_totals");
    timer.lap("Regions through the device");
    Output out(args.common.output);
    {
        std::string s;
        s.append("#class\tquantity\tobserved\tmean\tsd\tz\tfold\tn_ge\tn_le\tp_ge\tp_le\n");
        std::vector<uint64_t> X(static_cast<size_t>(N) + 1);
        for (uint32_t k = 0; k <= T; ++k) {
            const std::string name = k < T ? layers[k] : std::string("none");
            for (size_t p = 0; p <= N; ++p) X[p] = B[p * (T + 1) + k];
            append_stats(s, name, "bases", X);
            for (size_t p = 0; p <= N; ++p) X[p] = R[p * (T + 1) + k];
            append_stats(s, name, "regions", X);
        }
        out.write(s);
    }
    out.close();
    if (args.perms) {
        Output pf(args.perms);
        std::string s;
        char buf[32];
        for (size_t p = 0; p <= N; ++p) {
            s.append(buf, std::snprintf(buf, sizeof buf, "%zu", p));
            for (const std::vector<uint64_t> *M : {&B, &R})
                for (uint32_t k = 0; k <= T; ++k) s.append(buf, std::snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)(*M)[p * (T + 1) + k]));
            s.push_back('\n');
            if (s.size() > (1u << 20)) pf.write(s), s.clear();
        }
        pf.write(s);
        pf.close();
    }
    timer.lap("Statistics + writing");
    if (unplaced)
        std::fprintf(stderr, "[WARN] %llu regions are wider than their seqid's length%s and stayed where they are in every permutation\n", (unsigned long long)unplaced,
                     args.genome ? "" : " (no -g: the length is the largest end of the seqid's lines)");
    if (verbose) std::fprintf(stderr, "[DEBUG] enrich: %llu regions in %zu chunks\n", (unsigned long long)regions, feed.chunks());
    const double total_ms = timer.total();
    double stage[6] = {0, 0, 0, 0, 0, 0};
    (void)gffx_hip_classmap_stage_ms(h.get(), stage);
    g_run_stats.count("regions", (double)regions);
    g_run_stats.count("layers", (double)T);
    g_run_stats.count("permutations", (double)N);
    g_run_stats.count("unplaced", (double)unplaced);
    g_run_stats.count("points", (double)gffx_hip_classmap_n_points(h.get()));
    g_run_stats.count("chunks", (double)feed.chunks());
    g_run_stats.count("kernel_ms", kernel_ms);
    g_run_stats.count("class_map_build_ms", stage[0] + stage[1] + stage[2] + stage[3] + stage[4] + stage[5]);
    g_run_stats.count("threads", (double)threads);
    g_run_stats.write("enrich", total_ms);
}

}  // namespace gffx::commands::enrich
