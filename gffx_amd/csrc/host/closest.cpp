// closest.cpp -- `gffx closest` above the C-ABI (an addition: the reference has no such command): for every region
// the root features nearest to it and their signed distance.  The rule is device/closest_core.hpp; the search runs on the
// device (gffx_hip_closest_*).  A BED file streams chunk by chunk through a region store (two pinned staging buffers), each
// chunk is answered and written before the next one is parsed: memory is bounded by a chunk, and the output -- one line per
// answered root in kept-row order -- depends neither on the chunk size nor on -t.
#include <cstdio>

#include "../device/closest_core.hpp"
#include "region_feed.hpp"
#include "table_output.hpp"

namespace gffx::commands::closest {

namespace {

using ClosestHandle = Handle<gffx_hip_closest, gffx_hip_closest_destroy>;

// `.fts`: the ID of feature fid is line fid
std::vector<std::string_view> fts_lines(std::string_view data) {
    std::vector<std::string_view> ids;
    for (size_t pos = 0; pos < data.size();) {
        size_t nl = data.find('\n', pos);
        if (nl == std::string_view::npos) nl = data.size();
        std::string_view line = data.substr(pos, nl - pos);
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        ids.push_back(line);
        pos = nl + 1;
    }
    return ids;
}

struct Runner {
    const TreeIndexData &index;
    const std::vector<std::string_view> &ids;
    gffx_hip_closest *h;
    size_t threads;
    Output &out;
    uint64_t regions = 0, pairs = 0, unanswered = 0;
    double kernel_ms = 0;
    std::vector<uint32_t> counts{}, gaps{}, triples{};
    std::vector<uint64_t> offsets{};
    std::string text{};

    // the run on `rows` (n regions, already handed to the device) has been enqueued: its lines
    void finish(const uint32_t *rows, uint64_t n) {
        if (gffx_hip_closest_wait(h) != GFFX_OK) hip_fail("gffx_hip_closest_wait");
        uint64_t total = 0;
        if (gffx_hip_closest_total_pairs(h, &total) != GFFX_OK) hip_fail("gffx_hip_closest_total_pairs");
        counts.resize(n), gaps.resize(n), offsets.resize(n + 1), triples.resize(3 * total);
        if (gffx_hip_closest_copy_counts(h, counts.data()) != GFFX_OK || gffx_hip_closest_copy_gaps(h, gaps.data()) != GFFX_OK ||
            gffx_hip_closest_copy_offsets(h, offsets.data()) != GFFX_OK || gffx_hip_closest_copy_triples(h, triples.data()) != GFFX_OK)
            hip_fail("gffx_hip_closest_copy");
        double ms = 0;
        if (gffx_hip_closest_last_kernel_ms(h, &ms) == GFFX_OK) kernel_ms += ms;
        text.clear();
        append_rows_parallel(text, n, threads, [&](size_t i, std::string &s) {
            const uint32_t chr = rows[3 * i], qs = rows[3 * i + 1], qe = rows[3 * i + 2];
            char buf[64];
            const std::string &name = index.num_to_seqid[chr];
            const int head = std::snprintf(buf, sizeof buf, "\t%u\t%u\t", qs, qe);
            if (!counts[i]) {
                s.append(name).append(buf, head).append(".\t.\t.\t.\n");
                return;
            }
            for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) {
                const uint32_t fid = triples[3 * k], fs = triples[3 * k + 1], fe = triples[3 * k + 2];
                s.append(name).append(buf, head);
                if (fid < ids.size())
                    s.append(ids[fid]);
                else
                    s.push_back('.');
                char tail[80];
                const int m = std::snprintf(tail, sizeof tail, "\t%u\t%u\t%lld\n", fs, fe, gffx::closest::signed_distance(fs, fe, qs, qe, gaps[i]));
                s.append(tail, m);
            }
        });
        out.write(text);
        regions += n;
        pairs += total;
        for (uint64_t i = 0; i < n; ++i) unanswered += counts[i] == 0;
    }
};

}  // namespace

void run(const ClosestArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    const size_t threads = args.common.effective_threads();
    DeviceWarmup warm(args.device);
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    const std::string fts_path = append_suffix(args.common.input, ".fts");
    const MappedFile fts = map_file_or(fts_path, "Failed to mmap " + fts_path);
    const std::vector<std::string_view> ids = fts_lines(fts.view());
    timer.lap("Loading tree index + .fts");
    const uint32_t side_flag = args.side == Side::Left ? uint32_t(GFFX_CLOSEST_LEFT_ONLY) : args.side == Side::Right ? uint32_t(GFFX_CLOSEST_RIGHT_ONLY) : 0u;
    const uint32_t flags = (args.ignore_overlaps ? uint32_t(GFFX_CLOSEST_IGNORE_OVERLAPS) : 0u) | side_flag;
    RegionFeed feed(args.region, args.bed, index_data, args.common);
    warm.wait();
    index_data.ensure_device(args.device);
    timer.lap("Index upload");
    feed.open(args.device, verbose, timer);
    ClosestHandle h;
    if (gffx_hip_closest_create(index_data.device_index.get(), feed.chunk_rows(), OutPtr(h)) != GFFX_OK) hip_fail("gffx_hip_closest_create");
    feed.create_store(args.device);
    timer.lap("End table + buffers");
    Output out(args.common.output);
    out.write("chr\tstart\tend\tid\tfeature_start\tfeature_end\tdistance\n");
    Runner r{index_data, ids, h.get(), threads, out};
    // n rows sit in staging buffer k: to the store, through the device, to the output
    feed.run(threads, [&](gffx_hip_regions *store, int k, const uint32_t *stage, uint64_t n) {
        if (gffx_hip_regions_append(store, k, n) != GFFX_OK) hip_fail("gffx_hip_regions_append");
        if (gffx_hip_closest_run_store(h.get(), store, k, 0, n, flags) != GFFX_OK) hip_fail("gffx_hip_closest_run_store");
        r.finish(stage, n);
    });
    out.close();
    timer.lap("Regions through the device + writing");
    if (verbose)
        std::fprintf(stderr, "[DEBUG] closest: %llu regions, %llu answered roots, %llu regions without an answer\n", (unsigned long long)r.regions,
                     (unsigned long long)r.pairs, (unsigned long long)r.unanswered);
    const double total_ms = timer.total();
    double build_ms = 0;
    uint64_t grows = 0;
    (void)gffx_hip_closest_stats(h.get(), &build_ms, &grows);
    g_run_stats.count("regions", (double)r.regions);
    g_run_stats.count("answered_roots", (double)r.pairs);
    g_run_stats.count("regions_without_answer", (double)r.unanswered);
    g_run_stats.count("chunks", (double)feed.chunks());
    g_run_stats.count("kernel_ms", r.kernel_ms);
    g_run_stats.count("end_table_build_ms", build_ms);
    g_run_stats.count("pair_buffer_grows", (double)grows);
    g_run_stats.count("threads", (double)threads);
    g_run_stats.write("closest", total_ms);
}

}  // namespace gffx::commands::closest
