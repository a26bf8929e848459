// search.cpp -- `gffx search` above the C-ABI (reference: commands/search.rs:55-252): the `.atn` / `.a2f` / `.prt` loaders
// (index_loader/core.rs:37-89, a2f.rs:77-113, prt.rs:108-125), the value or pattern list, the three bails, the two warnings
// and the two writers.  The match of every `.atn` value against the list (search.rs:89-111) -- exact, or with -r against
// the DFAs that regex_dfa.cpp compiles from the patterns --, aids -> fids -> roots (search.rs:125-187) and the value test of
// every line of the hit blocks (utils/common.rs:389-431) run on the device through gffx_hip_attrs_*; there is no CPU
// matcher in this path.
//
// The keep set as integers: device/search_core.hpp's header.  The aid of a value is its position in the loaded vector, as
// in the reference (core.rs:42-68) -- also where a dropped line (a '#' value, a line that is blank after trim()) makes it
// disagree with the aids `.a2f` was written with.  That is the reference's behaviour and it is not repaired here.
//
// Deliberate differences:
//   - "[WARN] AID n not found (no FIDs)." lines come in ascending aid order (the reference walks an FxHashMap of the matched
//     strings, a2f.rs:54-64), and the per-string [DEBUG] listings of -v (search.rs:118-149) are not printed;
//   - -r takes a documented subset of the `regex` crate's syntax (regex_dfa.hpp); anything else is an error, never another
//     meaning;
//   - a parent cycle that no root closes never ends in the reference (prt.rs:58-71); here the chase ends after n steps and
//     the fid is reported with the invalid ones;
//   - the index files are checked first (check_index_files_exist, common.rs:151-170), as in extract.cpp;
//   - an -A file that cannot be opened is named in the message (the reference prints the bare OS error).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "filtered_output.hpp"
#include "gffx.hpp"
#include "regex_dfa.hpp"

namespace gffx::commands::search {

namespace {

using filtered::Names;

// core.rs:37-89: (attribute name, values); the aid of a value is its index
std::pair<std::string, Names> load_atn(const std::string &gff) {
    const std::string path = append_suffix(gff, ".atn");
    const MappedFile f = map_file_or(path, "Failed to mmap file: \"" + path + "\"");
    const std::string_view data = f.view();
    Names values;
    std::optional<std::string> attr_name;
    auto push_line = [&](std::string_view bytes) {  // :46-70
        if (bytes.empty()) return;
        if (!utf8_valid(bytes)) throw Error("ATN contains invalid UTF-8");
        std::string_view line = trim_unicode_ws(bytes);
        if (!attr_name && line.substr(0, 3) == "\xEF\xBB\xBF") line.remove_prefix(3);  // :55-57: only before the header has been seen
        static constexpr std::string_view kHeader = "#attribute=";
        if (line.substr(0, kHeader.size()) == kHeader) {
            if (attr_name) throw Error("Multiple #attribute= headers found in .atn file");
            attr_name = std::string(line.substr(kHeader.size()));
        } else if (!line.empty() && line[0] != '#') {
            values.push(line);
        }
    };
    size_t start = 0;
    for (size_t nl; (nl = data.find('\n', start)) != std::string_view::npos; start = nl + 1) push_line(data.substr(start, nl - start));
    if (start < data.size()) push_line(data.substr(start));
    if (!attr_name) throw Error("Missing #attribute=... header in .atn file");
    return {*attr_name, std::move(values)};
}

// a2f.rs:77-113: word f = the aid of fid f, u32::MAX = none
std::vector<uint32_t> load_a2f(const std::string &gff) {
    const std::string path = append_suffix(gff, ".a2f");
    const MappedFile f = map_file_or(path, "Failed to mmap " + path);
    if (f.size() % 4 != 0) throw Error("Corrupted A2F (" + path + "): length " + std::to_string(f.size()) + " not aligned to u32");
    std::vector<uint32_t> a2f(f.size() / 4);
    for (size_t i = 0; i < a2f.size(); ++i) a2f[i] = get_le32(f.data() + 4 * i);
    return a2f;
}

// search.rs:76-87: -A FILE one pattern per line (BufRead::lines: cut at '\n', one '\r' before it dropped, invalid UTF-8
// fails the run), each trim()ed, empty ones dropped -- a Vec, duplicates stay; -a VALUE as given.
Names read_patterns(const SearchArgs &args) {
    Names out;
    if (args.attr_list) {
        const MappedFile f = map_file_or(*args.attr_list, "Cannot open attribute list: \"" + *args.attr_list + "\"");
        const std::string_view data = f.view();
        for (size_t pos = 0; pos < data.size();) {
            size_t nl = data.find('\n', pos);
            const size_t next = nl == std::string_view::npos ? data.size() : nl + 1;
            if (nl == std::string_view::npos) nl = data.size();
            std::string_view line = data.substr(pos, nl - pos);
            pos = next;
            if (!line.empty() && line.back() == '\r' && nl < data.size()) line.remove_suffix(1);
            if (!utf8_valid(line)) throw Error("stream did not contain valid UTF-8");
            line = trim_unicode_ws(line);
            if (!line.empty()) out.push(line);
        }
    } else if (args.attr) {
        out.push(*args.attr);
    } else {
        throw Error("Either --attr-list (-A) or --attr (-a) must be provided.");
    }
    return out;
}

std::vector<uint32_t> set_bits(const std::vector<uint64_t> &words) {
    std::vector<uint32_t> v;
    for (size_t w = 0; w < words.size(); ++w)
        for (uint64_t m = words[w]; m; m &= m - 1) v.push_back(static_cast<uint32_t>(64 * w + __builtin_ctzll(m)));
    return v;
}

std::string debug_list(const std::vector<uint32_t> &v) {  // `{:?}` of a Vec<u32>
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

}  // namespace

// search.rs:55-252
void run_search(const SearchArgs &args) {
    const bool verbose = args.common.verbose;
    const std::string &gff_path = args.common.input;
    StageTimer timer{verbose};
    if (verbose) {
        std::fprintf(stderr, "[DEBUG] Starting processing of \"%s\"\n", gff_path.c_str());
        std::fprintf(stderr, "[DEBUG] Thread pool initialized with %zu threads\n", args.common.effective_threads());
    }
    if (!check_index_files_exist(gff_path)) throw Error("index files of \"" + gff_path + "\" are missing: run `gffx index` first");
    DeviceWarmup warm(args.device);  // (the HIP runtime's start beside the loaders)
    const std::vector<uint32_t> prt = filtered::load_prt(gff_path);      // search.rs:70
    const index_loader::GofMap gof = index_loader::load_gof(gff_path);  // :71
    const std::vector<uint32_t> a2f = load_a2f(gff_path);               // :72
    const auto [attr_name, atn] = load_atn(gff_path);                   // :73
    const Names patterns = read_patterns(args);                         // :76-87
    timer.lap("Loading .prt / .gof / .a2f / .atn + reading the patterns");
    regex::Compiled dfas;
    if (args.regex) {  // :93-97: every pattern must compile -- before the run waits on the device
        std::vector<std::string> list;
        for (size_t i = 0; i < patterns.size(); ++i) list.emplace_back(patterns.at(i));
        dfas = regex::compile(list);
        timer.lap("Compiling the patterns to DFAs");
    }
    warm.wait();
    AttrsHandle attrs;
    if (gffx_hip_attrs_create(args.device, atn.size(), reinterpret_cast<const uint8_t *>(atn.bytes.data()), atn.off.data(), a2f.size(), a2f.data(),
                              prt.size(), prt.data(), reinterpret_cast<const uint8_t *>(attr_name.data()), static_cast<uint32_t>(attr_name.size()),
                              -1, 0, OutPtr(attrs)) != GFFX_OK)
        hip_fail("gffx_hip_attrs_create");
    timer.lap("Value table on the device (values H2D, k_table_insert, k_attr_classes)");
    // Step 1 (search.rs:89-116): the aids whose value matches
    if (args.regex) {
        for (const regex::Dfa &d : dfas.groups)
            if (gffx_hip_attrs_match_dfa(attrs.get(), d.n_states, d.n_classes, d.init, d.cls, d.trans.data()) != GFFX_OK)
                hip_fail("gffx_hip_attrs_match_dfa");
    } else if (gffx_hip_attrs_match_exact(attrs.get(), patterns.size(), reinterpret_cast<const uint8_t *>(patterns.bytes.data()),
                                          patterns.off.data()) != GFFX_OK) {
        hip_fail("gffx_hip_attrs_match_exact");
    }
    std::vector<uint64_t> mwords((atn.size() + 63) / 64);
    if (gffx_hip_attrs_copy_matched_bitmap(attrs.get(), mwords.data(), mwords.size()) != GFFX_OK) hip_fail("gffx_hip_attrs_copy_matched_bitmap");
    const std::vector<uint32_t> aids = set_bits(mwords);
    timer.lap(args.regex ? "Matching the values on the device (k_attr_match_dfa, matched bitmap D2H)"
                         : "Matching the values on the device (k_attr_match_exact, matched bitmap D2H)");
    if (verbose && args.regex)
        std::fprintf(stderr, "[INFO] %zu pattern(s) in %zu DFA group(s), %s\n", patterns.size(), dfas.groups.size(),
                     gffx_hip_attrs_dfa_kernel(attrs.get()));
    if (aids.empty()) throw Error("None of the attributes matched.");  // :114-116
    // Steps 2 and 3 (:125-187): aids -> fids -> roots
    if (gffx_hip_attrs_resolve(attrs.get()) != GFFX_OK) hip_fail("gffx_hip_attrs_resolve");
    const size_t n_words = (std::max(a2f.size(), prt.size()) + 63) / 64;
    std::vector<uint64_t> fwords(n_words), rwords(n_words), iwords(n_words);
    if (gffx_hip_attrs_copy_fid_bitmap(attrs.get(), fwords.data(), n_words) != GFFX_OK) hip_fail("gffx_hip_attrs_copy_fid_bitmap");
    if (gffx_hip_attrs_copy_root_bitmap(attrs.get(), rwords.data(), n_words) != GFFX_OK) hip_fail("gffx_hip_attrs_copy_root_bitmap");
    if (gffx_hip_attrs_copy_invalid_bitmap(attrs.get(), iwords.data(), n_words) != GFFX_OK) hip_fail("gffx_hip_attrs_copy_invalid_bitmap");
    const std::vector<uint32_t> fids = set_bits(fwords), roots = set_bits(rwords), invalid = set_bits(iwords);
    {  // a2f.rs:54-64: a matched aid that no fid carries
        std::vector<char> has_fid(atn.size(), 0);
        for (uint32_t f : fids)
            if (f < a2f.size() && a2f[f] < atn.size()) has_fid[a2f[f]] = 1;
        for (uint32_t a : aids)
            if (!has_fid[a]) std::fprintf(stderr, "[WARN] AID %u not found (no FIDs).\n", a);
    }
    timer.lap("Aids -> fids -> roots on the device (k_attr_resolve, three bitmaps D2H)");
    if (fids.empty()) throw Error("No feature IDs (FIDs) resolved from matched attributes.");  // :140-142
    if (verbose) std::fprintf(stderr, "[DEBUG] Total unique FIDs: %zu\n", fids.size());
    if (!invalid.empty())  // :177-185
        std::fprintf(stderr, "[WARN] %zu FIDs have invalid parent chains (or out-of-range): %s\n", invalid.size(), debug_list(invalid).c_str());
    if (roots.empty()) throw Error("No valid root features resolved from matched attributes.");  // :189-191
    if (verbose) std::fprintf(stderr, "[DEBUG] Total unique roots: %zu\n", roots.size());
    const std::vector<Block> blocks = gof.roots_to_offsets(roots, args.common.effective_threads());  // :196
    timer.lap("Root offsets");
    const bool per_feature = !args.common.entire_group || args.common.types;  // :198
    if (per_feature) {
        const filtered::TypeList types(args.common.types);
        filtered::write_gff_output_filtered(
            gff_path, blocks, gof, args.common.output, verbose, args.common.effective_threads(),
            "  value filter on the device (chunks H2D, k_attr_filter, flags back)",
            [&](const uint8_t *text, uint64_t bytes, uint64_t n_lines, const uint64_t *off, const uint32_t *root, uint8_t *keep) {
                if (gffx_hip_attrs_filter_lines(attrs.get(), text, bytes, n_lines, off, root, args.common.types ? 1 : 0, types.n,
                                                reinterpret_cast<const uint8_t *>(types.bytes.data()), types.off.data(), keep) != GFFX_OK)
                    hip_fail("gffx_hip_attrs_filter_lines");
            });
    } else {
        write_gff_output(gff_path, blocks, args.common.output, verbose);
    }
    timer.lap(per_feature ? "Value filter + writing matched lines" : "Writing blocks");
    double ms[4] = {0, 0, 0, 0};
    (void)gffx_hip_attrs_stage_ms(attrs.get(), &ms[0], &ms[1], &ms[2], &ms[3]);
    if (verbose)
        std::fprintf(stderr, "[TIMER] [device] table build %.3f ms, match %.3f ms, resolve %.3f ms, line filter %.3f ms (HIP events)\n", ms[0], ms[1],
                     ms[2], ms[3]);
    const double total_ms = timer.total();
    g_run_stats.count("patterns", static_cast<double>(patterns.size()));
    g_run_stats.count("dfa_groups", static_cast<double>(dfas.groups.size()));
    g_run_stats.count("table_values", static_cast<double>(atn.size()));
    g_run_stats.count("aids_matched", static_cast<double>(aids.size()));
    g_run_stats.count("fids_matched", static_cast<double>(fids.size()));
    g_run_stats.count("fids_invalid", static_cast<double>(invalid.size()));
    g_run_stats.count("unique_roots", static_cast<double>(roots.size()));
    g_run_stats.count("blocks", static_cast<double>(blocks.size()));
    g_run_stats.count("device_table_build_ms", ms[0]);
    g_run_stats.count("device_match_ms", ms[1]);
    g_run_stats.count("device_resolve_ms", ms[2]);
    g_run_stats.count("device_filter_ms", ms[3]);
    g_run_stats.write("search", total_ms);
}

}  // namespace gffx::commands::search
