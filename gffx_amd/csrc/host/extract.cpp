// extract.cpp -- `gffx extract` above the C-ABI (reference: commands/extract.rs:37-162): the `.fts` / `.prt` loaders
// (index_loader/fts.rs:97-138, prt.rs:108-125), the name list, the block set and the two writers.  The name -> fid lookup
// (fts.rs:16-93), the fid -> root chase (prt.rs:54-102) and the ID test of every line of the hit blocks
// (utils/common.rs:389-431) run on the device through gffx_hip_ids_*; there is no CPU lookup here.
//
// The keep set as integers.  The reference hands write_gff_output_filtered, per root r, the ID STRINGS of the requested fids
// whose root is r (extract.rs:122-135), and keeps a line of block r iff the value after its first `ID=` is one of them.  A
// requested fid is always the LAST `.fts` line of its string (fts.rs:16-22), so a value X is in that set iff X is in the
// table, its fid f was requested and root(f) == r: an integer test, exact also where two blocks carry the same ID (only the
// block of the last line's root keeps it).
//
// Deliberate differences:
//   - the names that are not found are listed in the order of their first appearance (the reference prints them in the order
//     of an FxHashSet walk);
//   - a parent cycle that no root closes never ends in the reference (prt.rs:58-71); here the chase ends after n steps and the
//     fid is reported with the invalid ones (device/ids_core.hpp chase_root);
//   - the reference loads `.fts` first and fails with "Failed to mmap <path>" when it is missing; here the index files are
//     checked first (check_index_files_exist, common.rs:151-170) and the run fails with its "Missing index file(s)" list.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_set>

#include "filtered_output.hpp"
#include "gffx.hpp"

namespace gffx::commands::extract {

namespace {

using filtered::Names;
using filtered::load_prt;

// fts.rs:97-138: one ID per line; empty lines are dropped, a trailing '\r' is stripped (a line that is only "\r" stays, empty)
Names load_fts(const std::string &gff) {
    const std::string path = append_suffix(gff, ".fts");
    const MappedFile f = map_file_or(path, "Failed to mmap " + path);
    const std::string_view data = f.view();
    Names ids;
    ids.bytes.reserve(data.size());
    size_t start = 0;
    auto take = [&](size_t end) {
        std::string_view slice = data.substr(start, end - start);
        if (slice.empty()) return;
        if (slice.back() == '\r') slice.remove_suffix(1);
        if (!utf8_valid(slice)) throw Error("FTS contains invalid UTF-8 at byte " + std::to_string(start));
        ids.push(slice);
    };
    while (start < data.size()) {
        const size_t nl = data.find('\n', start);
        if (nl == std::string_view::npos) break;
        take(nl);
        start = nl + 1;
    }
    if (start < data.size()) take(data.size());
    return ids;
}

// extract.rs:61-80: -F FILE one name per line (BufRead::lines: cut at '\n', one '\r' before it dropped, invalid UTF-8 fails
// the run), each trim()ed, empty ones dropped; -f ID as given.  Duplicates collapse (an FxHashSet there); the order here is
// that of the first appearance.
Names read_names(const ExtractArgs &args) {
    Names names;
    if (args.feature_file) {
        const MappedFile f = map_file_or(*args.feature_file, "Cannot open feature list: \"" + *args.feature_file + "\"");
        const std::string_view data = f.view();
        std::unordered_set<std::string_view> seen;
        std::vector<std::string_view> order;
        for (size_t pos = 0; pos < data.size();) {
            size_t nl = data.find('\n', pos);
            const size_t next = nl == std::string_view::npos ? data.size() : nl + 1;
            if (nl == std::string_view::npos) nl = data.size();
            std::string_view line = data.substr(pos, nl - pos);
            pos = next;
            if (!line.empty() && line.back() == '\r' && nl < data.size()) line.remove_suffix(1);
            if (!utf8_valid(line)) throw Error("stream did not contain valid UTF-8");
            line = trim_unicode_ws(line);
            if (line.empty()) continue;
            if (seen.insert(line).second) order.push_back(line);
        }
        for (std::string_view s : order) names.push(s);
    } else if (args.feature_id) {
        names.push(*args.feature_id);
    } else {
        throw Error("Either --feature-id (-f) or --feature-file (-F) must be specified");
    }
    return names;
}

// Rust's `{:?}` of a str, for the printable cases: quotes, backslashes and control characters escaped
std::string rust_debug(std::string_view s) {
    std::string o = "\"";
    for (unsigned char c : s) {
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            case 0: o += "\\0"; break;
            default:
                if (c < 0x20 || c == 0x7f) {
                    char b[16];
                    std::snprintf(b, sizeof b, "\\u{%x}", c);
                    o += b;
                } else {
                    o += static_cast<char>(c);
                }
        }
    }
    return o + "\"";
}

// common.rs:289-465 with the key "ID" (the host half is filtered_output.hpp's, shared with `gffx search`)
void write_gff_output_filtered(const std::string &gff_path, const std::vector<Block> &blocks, gffx_hip_ids *ids,
                               const index_loader::GofMap &gof, const std::optional<std::string> &types_filter,
                               const std::optional<std::string> &output_path, bool verbose, size_t threads) {
    const filtered::TypeList types(types_filter);  // common.rs:306-311
    filtered::write_gff_output_filtered(
        gff_path, blocks, gof, output_path, verbose, threads, "  ID filter on the device (chunks H2D, k_ids_filter, flags back)",
        [&](const uint8_t *text, uint64_t bytes, uint64_t n_lines, const uint64_t *off, const uint32_t *root, uint8_t *keep) {
            if (gffx_hip_ids_filter_lines(ids, text, bytes, n_lines, off, root, types_filter ? 1 : 0, types.n,
                                          reinterpret_cast<const uint8_t *>(types.bytes.data()), types.off.data(), keep) != GFFX_OK)
                hip_fail("gffx_hip_ids_filter_lines");
        });
}

}  // namespace

// extract.rs:37-162
void run_extract(const ExtractArgs &args) {
    const bool verbose = args.common.verbose;
    const std::string &gff_path = args.common.input;
    StageTimer timer{verbose};
    if (verbose) {
        std::fprintf(stderr, "[DEBUG] Starting processing of \"%s\"\n", gff_path.c_str());
        std::fprintf(stderr, "[DEBUG] Thread pool initialized with %zu threads\n", args.common.effective_threads());
    }
    if (!check_index_files_exist(gff_path)) throw Error("index files of \"" + gff_path + "\" are missing: run `gffx index` first");
    DeviceWarmup warm(args.device);  // (the HIP runtime's start beside the loaders)
    const Names fts = load_fts(gff_path);                                   // extract.rs:52
    const std::vector<uint32_t> prt = load_prt(gff_path);                   // :55
    const index_loader::GofMap gof = index_loader::load_gof(gff_path);      // :58
    const Names names = read_names(args);                                   // :61-80
    timer.lap("Loading .fts / .prt / .gof + reading the names");
    warm.wait();
    IdsHandle ids;
    if (gffx_hip_ids_create(args.device, fts.size(), reinterpret_cast<const uint8_t *>(fts.bytes.data()), fts.off.data(), prt.size(),
                            prt.data(), -1, OutPtr(ids)) != GFFX_OK)
        hip_fail("gffx_hip_ids_create");
    timer.lap("ID table on the device (names H2D, k_table_insert)");
    // Phase A (extract.rs:84-111): names -> fids -> roots
    std::vector<uint32_t> fid(std::max<size_t>(names.size(), 1)), root(std::max<size_t>(names.size(), 1));
    if (gffx_hip_ids_resolve(ids.get(), names.size(), reinterpret_cast<const uint8_t *>(names.bytes.data()), names.off.data(), fid.data(),
                             root.data()) != GFFX_OK)
        hip_fail("gffx_hip_ids_resolve");
    std::string missing;
    size_t n_missing = 0;
    std::vector<uint32_t> invalid;
    for (size_t i = 0; i < names.size(); ++i) {
        if (fid[i] == UINT32_MAX) {
            missing += (n_missing++ ? ", " : "") + rust_debug(names.at(i));
        } else if (root[i] == UINT32_MAX) {
            invalid.push_back(fid[i]);
        }
    }
    if (n_missing) std::fprintf(stderr, "[WARN] %zu feature IDs not found: [%s]\n", n_missing, missing.c_str());  // :88-90
    std::sort(invalid.begin(), invalid.end());
    invalid.erase(std::unique(invalid.begin(), invalid.end()), invalid.end());
    if (!invalid.empty()) {  // :100-111
        std::string list;
        for (size_t i = 0; i < invalid.size(); ++i) list += (i ? ", " : "") + std::to_string(invalid[i]);
        std::fprintf(stderr, "[WARN] %zu numeric feature IDs are invalid (out-of-range child or parent), skipped: [%s]\n", invalid.size(),
                     list.c_str());
    }
    // :114-116: the valid roots, sorted and deduplicated -- the set bits of the root bitmap, ascending
    std::vector<uint64_t> words((std::max(fts.size(), prt.size()) + 63) / 64);
    if (gffx_hip_ids_copy_root_bitmap(ids.get(), words.data(), words.size()) != GFFX_OK) hip_fail("gffx_hip_ids_copy_root_bitmap");
    std::vector<uint32_t> roots;
    for (size_t w = 0; w < words.size(); ++w)
        for (uint64_t m = words[w]; m; m &= m - 1) roots.push_back(static_cast<uint32_t>(64 * w + __builtin_ctzll(m)));
    timer.lap("Names -> fids -> roots on the device (names H2D, k_ids_resolve, results + root bitmap D2H)");
    const std::vector<Block> blocks = gof.roots_to_offsets(roots, args.common.effective_threads());  // :119
    timer.lap("Root offsets");
    const bool per_feature = !args.common.entire_group || args.common.types;  // :121
    if (per_feature)
        write_gff_output_filtered(gff_path, blocks, ids.get(), gof, args.common.types, args.common.output, verbose,
                                  args.common.effective_threads());
    else
        write_gff_output(gff_path, blocks, args.common.output, verbose);
    timer.lap(per_feature ? "ID filter + writing matched lines" : "Writing blocks");
    double ms[3] = {0, 0, 0};
    (void)gffx_hip_ids_stage_ms(ids.get(), &ms[0], &ms[1], &ms[2]);
    if (verbose)
        std::fprintf(stderr, "[TIMER] [device] table build %.3f ms, resolve %.3f ms, line filter %.3f ms (HIP events)\n", ms[0], ms[1], ms[2]);
    const double total_ms = timer.total();
    g_run_stats.count("names", static_cast<double>(names.size()));
    g_run_stats.count("names_missing", static_cast<double>(n_missing));
    g_run_stats.count("fids_invalid", static_cast<double>(invalid.size()));
    g_run_stats.count("table_names", static_cast<double>(fts.size()));
    g_run_stats.count("unique_roots", static_cast<double>(roots.size()));
    g_run_stats.count("blocks", static_cast<double>(blocks.size()));
    g_run_stats.count("device_table_build_ms", ms[0]);
    g_run_stats.count("device_resolve_ms", ms[1]);
    g_run_stats.count("device_filter_ms", ms[2]);
    g_run_stats.write("extract", total_ms);
}

}  // namespace gffx::commands::extract
