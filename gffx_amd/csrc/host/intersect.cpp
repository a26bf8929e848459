// intersect.cpp -- `gffx intersect` above the C-ABI (reference: commands/intersect.rs): the region argument and the command.
// Its parts: bed_parse.cpp (BED text), shard.cpp (--gpus N), join_a_stream.cpp (Join A), match_lines.cpp (per-line mode, Join B).
#include <cstdio>

#include "gffx.hpp"

namespace gffx::commands::intersect {

// intersect.rs:172-198
Region parse_region(const std::string &region, const std::unordered_map<std::string, uint32_t> &seqid_map,
                    const CommonArgs &common) {
    const size_t colon = region.find(':');
    if (colon == std::string::npos) throw Error("Invalid region format, expected 'chr:start-end'");
    const std::string seq = region.substr(0, colon), range = region.substr(colon + 1);
    const size_t dash = range.find('-');
    if (dash == std::string::npos) throw Error("Invalid range format, expected 'start-end'");
    const auto s = parse_u32_rust(std::string_view(range).substr(0, dash));
    const auto e = parse_u32_rust(std::string_view(range).substr(dash + 1));
    if (!s || !e) throw Error("invalid digit found in string");
    const auto it = seqid_map.find(seq);
    if (it == seqid_map.end()) throw Error("Sequence ID not found: " + seq);
    if (*s >= *e)
        throw Error("Region start must be less than end (" + std::to_string(*s) + " >= " + std::to_string(*e) + ")");
    if (common.verbose) std::fprintf(stderr, "[DEBUG] Parsed region: chr=%u, start=%u, end=%u\n", it->second, *s, *e);
    return {it->second, *s, *e};
}

// intersect.rs:541-655
void run(const IntersectArgs &args) {
    const bool verbose = args.common.verbose;
    StageTimer timer{verbose};
    if (verbose) {
        std::fprintf(stderr, "[DEBUG] Starting processing of \"%s\"\n", args.common.input.c_str());
        std::fprintf(stderr, "[DEBUG] Thread pool initialized with %zu threads\n", args.common.effective_threads());
        if (args.common.threads && args.common.effective_threads() != args.common.threads)
            std::fprintf(stderr, "[INFO] --threads %zu capped at %zu: twice the CPUs this process may use (cgroup quota / affinity)\n",
                         args.common.threads, args.common.effective_threads());
    }
    const OverlapMode mode = args.contained         ? OverlapMode::Contained
                             : args.contains_region ? OverlapMode::ContainsRegion
                                                    : OverlapMode::Overlap;
    DeviceWarmup warm(args.device);  // (the HIP runtime's 0.2 s start here, beside the index loader, not after it)
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.common.input);
    timer.lap("Loading tree index");
    const bool per_line = !args.common.entire_group || args.common.types;  // intersect.rs:619
    if (verbose) {
        static const char *kNames[] = {"Contained", "ContainsRegion", "Overlap"};
        std::fprintf(stderr, "[DEBUG] Mode: %s\n", kNames[static_cast<int>(mode)]);
    }
    std::vector<Region> regions;  // --region
    StreamResult sr;              // --bed: the regions never exist on the host as a whole
    std::vector<uint32_t> roots;
    if (args.bed) {
        // parse + Join A, streamed; the CLI only consumes the unique root ids (intersect.rs:598-615)
        sr = stream_unique_roots(index_data, *args.bed, mode, args.invert, verbose, args.common.effective_threads(), args.device,
                                 args.gpus, per_line);
        roots = std::move(sr.roots);
        if (verbose) std::fprintf(stderr, "[DEBUG] query_features over %llu regions\n", (unsigned long long)sr.n_regions);
        timer.lap("Parsing regions + Join A on the device (streamed: parse, H2D, kernel overlap)");
    } else if (args.region) {
        regions.push_back(parse_region(*args.region, index_data.seqid_to_num, args.common));
        timer.lap("Parsing regions");
        roots = query_unique_roots(index_data, regions, mode, args.invert, verbose, args.device);
        timer.lap("Join A on the device (index upload, regions H2D, kernel, root bitmap D2H)");
    } else {
        throw Error("No region specified");
    }
    const index_loader::GofMap gof = index_loader::load_gof(args.common.input);
    const std::vector<Block> blocks = gof.roots_to_offsets(roots, args.common.effective_threads());
    timer.lap("Root offsets");
    if (per_line && args.bed)
        write_matched_lines(args.common.input, blocks, sr.has_regions, nullptr, sr.n_regions, sr.store.get(), index_data.num_to_seqid,
                            args.common.types, args.common.output, mode, verbose, args.common.effective_threads(),
                            gffx_hip_index_device(index_data.device_index.get()), &gof);
    else if (per_line)
        write_gff_match_only_by_coords(args.common.input, blocks, regions, index_data.num_to_seqid, args.common.types,
                                       args.common.output, mode, verbose, args.common.effective_threads(), args.device, &gof);
    else
        write_gff_output(args.common.input, blocks, args.common.output, verbose);
    timer.lap(!args.common.entire_group || args.common.types ? "Join B + writing matched lines" : "Writing blocks");
    const double total_ms = timer.total();
    g_run_stats.count("regions", args.bed ? (double)sr.n_regions : (double)regions.size());
    g_run_stats.count("unique_roots", (double)roots.size());
    if (args.bed) g_run_stats.count("wide_form_passes", (double)sr.wide_form_passes);
    g_run_stats.count("blocks", (double)blocks.size());
    g_run_stats.count("threads", (double)args.common.effective_threads());
    g_run_stats.count("gpus", (double)args.gpus);
    if (args.bed) {
        std::string devs = "[";
        for (size_t d = 0; 2 * d + 1 < sr.per_device.size(); ++d)
            devs += std::string(d ? ", " : "") + "{\"regions\": " + std::to_string(sr.per_device[2 * d]) + ", \"kept_pairs\": " +
                    std::to_string(sr.per_device[2 * d + 1]) + "}";
        g_run_stats.extra("devices", devs + "]");
        g_run_stats.extra("devices_from_rccl_exchange", sr.exchanged ? "true" : "false");
        g_run_stats.extra("knobs", sr.knobs);
    }
    g_run_stats.write("intersect", total_ms);
}

}  // namespace gffx::commands::intersect
