// annotate.cpp -- `gffx annotate` above the C-ABI (an addition: the reference has no such command): for every
// region how many of its bases are of each feature class.  -T names the layers in priority order; the class of a base is the
// first layer with a line that covers it (device/classmap_core.hpp).  The lines come from the all-line table `<gff>.lall`
// (or from the text when there is none), the class map is built on the device once (gffx_hip_classmap_*), and a BED file
// streams chunk by chunk through a region store like `gffx closest`: the output -- one line per region in input order --
// depends neither on the chunk size nor on -t.
#include <cstdio>

#include "layer_rows.hpp"
#include "region_feed.hpp"
#include "table_output.hpp"

namespace gffx::commands::annotate {

void run(const AnnotateArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    const size_t threads = args.common.effective_threads();
    const std::vector<std::string> &layers = args.layers;
    const uint32_t T = static_cast<uint32_t>(layers.size());
    DeviceWarmup warm(args.device);
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    const uint32_t n_seq = static_cast<uint32_t>(index_data.num_to_seqid.size());
    timer.lap("Loading tree index");
    // the layers' rows
    std::vector<uint32_t> rows;
    std::vector<uint64_t> per_layer(T, 0);
    uint64_t skipped = 0;
    layer_rows::collect(args.common.input, layers, index_data.seqid_to_num, threads, verbose, rows, per_layer, skipped, nullptr);
    layer_rows::report(args.common.input, layers, per_layer, ": its column is zero", verbose ? "annotate" : nullptr, skipped);
    timer.lap("Layer rows from the line table");
    RegionFeed feed(args.region, args.bed, index_data, args.common);
    warm.wait();
    feed.open(args.device, verbose, timer);
    const ClassMapHandle h = layer_rows::build_class_map(args.device, n_seq, T, rows);
    feed.create_store(args.device);
    timer.lap("Class map + buffers");
    Output out(args.common.output);
    {
        std::string head = "#chr\tstart\tend\tclass";
        for (const std::string &name : layers) head.append("\t").append(name);
        out.write(head + "\tnone\n");
    }
    std::vector<uint64_t> sum_regions(T + 1, 0), sum_bases(T + 1, 0);
    std::vector<uint32_t> counts;
    std::vector<uint8_t> cls;
    std::string text;
    uint64_t regions = 0;
    double kernel_ms = 0;
    // n rows sit in staging buffer k: to the store, through the device, to the output
    feed.run(threads, [&](gffx_hip_regions *store, int k, const uint32_t *stage, uint64_t n) {
        if (gffx_hip_regions_append(store, k, n) != GFFX_OK) hip_fail("gffx_hip_regions_append");
        if (gffx_hip_classmap_run_store(h.get(), store, k, 0, n) != GFFX_OK) hip_fail("gffx_hip_classmap_run_store");
        if (gffx_hip_classmap_wait(h.get()) != GFFX_OK) hip_fail("gffx_hip_classmap_wait");
        counts.resize(n * (T + 1)), cls.resize(n);
        if (gffx_hip_classmap_copy_counts(h.get(), counts.data()) != GFFX_OK || gffx_hip_classmap_copy_class(h.get(), cls.data()) != GFFX_OK)
            hip_fail("gffx_hip_classmap_copy");
        double ms = 0;
        if (gffx_hip_classmap_last_kernel_ms(h.get(), &ms) == GFFX_OK) kernel_ms += ms;
        text.clear();
        append_rows_parallel(text, n, threads, [&](size_t i, std::string &s) {  // (the staging buffer still holds the rows)
            char buf[64];
            s.append(index_data.num_to_seqid[stage[3 * i]]);
            s.append(buf, std::snprintf(buf, sizeof buf, "\t%u\t%u\t", stage[3 * i + 1], stage[3 * i + 2]));
            if (cls[i] < T)
                s.append(layers[cls[i]]);
            else
                s.push_back('.');
            for (uint32_t c = 0; c <= T; ++c) s.append(buf, std::snprintf(buf, sizeof buf, "\t%u", counts[i * (T + 1) + c]));
            s.push_back('\n');
        });
        out.write(text);
        for (uint64_t i = 0; i < n; ++i) {
            sum_regions[std::min<uint32_t>(cls[i], T)]++;
            for (uint32_t c = 0; c <= T; ++c) sum_bases[c] += counts[i * (T + 1) + c];
        }
        regions += n;
    });
    out.close();
    if (args.summary) {
        Output sum(args.summary);
        std::string s;
        for (uint32_t c = 0; c <= T; ++c) {
            char buf[64];
            s.append(c < T ? layers[c] : std::string("none"));
            s.append(buf, std::snprintf(buf, sizeof buf, "\t%llu\t%llu\n", (unsigned long long)sum_regions[c], (unsigned long long)sum_bases[c]));
        }
        sum.write(s);
        sum.close();
    }
    timer.lap("Regions through the device + writing");
    if (verbose) std::fprintf(stderr, "[DEBUG] annotate: %llu regions in %zu chunks\n", (unsigned long long)regions, feed.chunks());
    const double total_ms = timer.total();
    double stage[6] = {0, 0, 0, 0, 0, 0};
    (void)gffx_hip_classmap_stage_ms(h.get(), stage);
    g_run_stats.count("regions", (double)regions);
    g_run_stats.count("layers", (double)T);
    g_run_stats.count("points", (double)gffx_hip_classmap_n_points(h.get()));
    g_run_stats.count("chunks", (double)feed.chunks());
    g_run_stats.count("kernel_ms", kernel_ms);
    g_run_stats.count("class_map_build_ms", stage[0] + stage[1] + stage[2] + stage[3] + stage[4] + stage[5]);
    g_run_stats.count("threads", (double)threads);
    g_run_stats.write("annotate", total_ms);
}

}  // namespace gffx::commands::annotate
