// match_lines.cpp -- the per-line mode of `gffx intersect` (commands/intersect.rs:232-538): hit blocks' lines, -T, Join B, copy-out
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "intersect_internal.hpp"

namespace gffx::commands::intersect {

// intersect.rs:80-102
bool gff_type_allowed(std::string_view line, const std::vector<std::string> &allow) {
    size_t off = 0;
    for (int tabs = 0; tabs < 2; ++tabs) {
        const size_t t = line.find('\t', off);
        if (t == std::string_view::npos) return false;
        off = t + 1;
    }
    const size_t t = line.find('\t', off);
    if (t == std::string_view::npos) return false;
    const std::string_view ty = line.substr(off, t - off);
    if (!utf8_valid(ty)) return false;
    for (const auto &a : allow)
        if (ty == a) return true;
    return false;
}

// intersect.rs:446-494
bool split_line_for_join_b(std::string_view line, std::string_view &seq, uint32_t &start, uint32_t &end) {
    size_t tab[5];
    size_t off = 0;
    for (int c = 0; c < 5; ++c) {
        tab[c] = line.find('\t', off);
        if (tab[c] == std::string_view::npos) return false;
        off = tab[c] + 1;
    }
    const auto s = parse_u32_ascii(line.substr(tab[2] + 1, tab[3] - tab[2] - 1));
    if (!s) return false;
    const auto e = parse_u32_ascii(line.substr(tab[3] + 1, tab[4] - tab[3] - 1));
    if (!e) return false;
    seq = line.substr(0, tab[0]);
    if (!utf8_valid(seq)) return false;
    start = *s;
    end = *e;
    return true;
}

namespace {

// blocks in output order (intersect.rs:335), sentinels and empty ranges dropped (:269-277)
std::vector<std::pair<uint64_t, uint64_t>> hit_ranges(const std::vector<Block> &blocks, size_t file_len) {
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (const auto &[root, s, e] : blocks) {
        if (s == MISSING) {
            std::fprintf(stderr, "[WARN] skipped fid=%u due to sentinel start offset\n", root);
            continue;
        }
        const uint64_t ee = std::min<uint64_t>(e, file_len);
        if (s >= ee) continue;
        ranges.emplace_back(s, ee);
    }
    std::sort(ranges.begin(), ranges.end());
    return ranges;
}

// line table of the hit blocks: (abs start, abs end incl. '\n', seqid number, raw start, raw end)
struct Part {
    std::vector<uint64_t> ls, le;
    std::vector<uint32_t> seq, s, e;
    void push(uint64_t l0, uint64_t l1, uint32_t sq, uint32_t start, uint32_t end) {
        ls.push_back(l0), le.push_back(l1), seq.push_back(sq), s.push_back(start), e.push_back(end);
    }
};

// what decides whether a line of a hit block enters the table
struct LineFilter {
    std::string_view data;                                             // the GFF
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // the hit blocks
    bool by_type = false;                                              // -T given
    std::vector<std::string> allow;                                    // its names
    std::unordered_map<std::string_view, uint32_t> seq_with_regions;  // query_ivmap's keys (intersect.rs:621-633): seqid NAME -> number
    AllLinesView all;                                                  // `<gff>.lall`, when it is used:
    std::vector<char> type_ok;                                         //   per type number: passes -T
    std::vector<uint32_t> seq_target;  //   per column-1 name number: the seqid number that owns regions, or UINT32_MAX
};

// The all-line table `<gff>.lall` written by `gffx index` (line_index.cpp): with it no text is parsed here.  An index made
// by the reference's own `gffx index` has none, a stale or damaged one is not used, GFFX_LINE_TABLE=parse ignores it.
bool open_all_lines(LineFilter &F, const std::string &gff_path, const index_loader::GofMap *gof, bool verbose) {
    const char *lt = std::getenv("GFFX_LINE_TABLE");
    std::string why = "disabled";
    bool use_all = false;
    if (!(lt && std::string(lt) == "parse")) {
        std::optional<index_loader::GofMap> own;
        if (!gof) {
            own = index_loader::load_gof(gff_path);
            gof = &*own;
        }
        use_all = F.all.open(append_suffix(gff_path, ".lall"), F.data.size(), index_loader::line_table_key(gff_path, *gof), why);
    }
    if (use_all) {
        F.type_ok.assign(F.all.type_names.size(), 1);
        if (F.by_type)
            for (size_t i = 0; i < F.all.type_names.size(); ++i)
                F.type_ok[i] = std::find(F.allow.begin(), F.allow.end(), F.all.type_names[i]) != F.allow.end();
        F.seq_target.assign(F.all.seq_names.size(), UINT32_MAX);
        for (size_t i = 0; i < F.all.seq_names.size(); ++i) {
            const auto it = F.seq_with_regions.find(F.all.seq_names[i]);
            if (it != F.seq_with_regions.end()) F.seq_target[i] = it->second;
        }
    }
    if (verbose)
        std::fprintf(stderr, use_all ? "[INFO] all-line table from %s.lall (%llu lines)\n" : "[INFO] all-line table not used (%s): parsing the hit blocks\n",
                     use_all ? gff_path.c_str() : why.c_str(), (unsigned long long)F.all.n_lines);
    return use_all;
}

// blocks [b0, b1) from the table: no text is read.  false: the image does not describe these blocks.
bool lines_from_table(const LineFilter &F, size_t b0, size_t b1, Part &P, const std::atomic<bool> &failed) {
    const AllLinesView &all = F.all;
    size_t cap = 0;  // (one allocation per column: the blocks' line counts are known before a line is looked at)
    for (size_t b = b0; b < b1; ++b) {
        uint64_t lo, hi;
        if (all.block_lines(F.ranges[b].first, F.ranges[b].second, lo, hi)) cap += hi - lo;
    }
    P.ls.reserve(cap), P.le.reserve(cap), P.seq.reserve(cap), P.s.reserve(cap), P.e.reserve(cap);
    for (size_t b = b0; b < b1; ++b) {
        uint64_t lo, hi;
        if (failed.load(std::memory_order_relaxed)) return false;
        if (!all.block_lines(F.ranges[b].first, F.ranges[b].second, lo, hi)) return false;
        uint64_t at = F.ranges[b].first;
        for (uint64_t i = lo; i < hi; ++i) {
            const uint64_t l0 = all.ls[i], l1 = l0 + all.len[i];
            if (l0 < at || l1 > F.ranges[b].second || all.len[i] == 0) return false;  // (damaged image: starts must ascend inside the block)
            at = l1;
            if (!(all.flags[i] & 1u)) continue;
            const uint32_t ty = all.type[i], sq = all.seq[i];
            if (F.by_type && (ty >= F.type_ok.size() || !F.type_ok[ty])) continue;
            if (sq >= F.seq_target.size()) return false;
            if (F.seq_target[sq] == UINT32_MAX) continue;
            P.push(l0, l1, F.seq_target[sq], all.start[i], all.end[i]);
        }
    }
    return true;
}

// blocks [b0, b1) from the GFF text (intersect.rs:284-321)
void lines_from_text(const LineFilter &F, size_t b0, size_t b1, Part &P) {
    for (size_t b = b0; b < b1; ++b) {
        size_t pos = F.ranges[b].first;
        const size_t stop = F.ranges[b].second;
        while (pos < stop) {
            size_t nl = F.data.find('\n', pos);
            nl = (nl == std::string_view::npos || nl >= stop) ? stop : nl + 1;
            std::string_view line = F.data.substr(pos, nl - pos);
            if (!line.empty() && line.back() == '\n') line.remove_suffix(1);
            if (!line.empty() && line[0] != '#' && (!F.by_type || gff_type_allowed(line, F.allow))) {
                std::string_view seq;
                uint32_t s, e;
                if (split_line_for_join_b(line, seq, s, e)) {
                    const auto it = F.seq_with_regions.find(seq);
                    if (it != F.seq_with_regions.end()) P.push(pos, nl, it->second, s, e);
                }
            }
            pos = nl;
        }
    }
}

// The line table of the hit blocks in parts (contiguous runs of blocks, eight per thread, taken in turn).  false: the
// all-line table failed on one of them (the parts are then worthless).
bool build_parts(const LineFilter &F, bool use_all, size_t n_threads, std::vector<Part> &parts) {
    const size_t n_parts = std::min(F.ranges.size(), n_threads * 8);
    parts.assign(std::max<size_t>(n_parts, 1), Part{});
    std::atomic<bool> table_failed{false};
    parallel_for(n_parts, n_threads, [&](size_t pi) {
        const size_t b0 = F.ranges.size() * pi / n_parts, b1 = F.ranges.size() * (pi + 1) / n_parts;
        if (!use_all) return lines_from_text(F, b0, b1, parts[pi]);
        if (table_failed.load(std::memory_order_relaxed)) return;
        if (!lines_from_table(F, b0, b1, parts[pi], table_failed)) table_failed = true;
    });
    return !table_failed;
}

struct LineTable {  // the parts back to back
    size_t n = 0;
    std::unique_ptr<uint64_t[]> ls, le;
    std::unique_ptr<uint32_t[]> seq, s, e;
};

// (copied by the same threads: 68 MB at GENCODE scale; the parts are emptied on the way)
LineTable concat_parts(std::vector<Part> &parts, size_t n_threads) {
    std::vector<size_t> part_off(parts.size() + 1, 0);
    for (size_t i = 0; i < parts.size(); ++i) part_off[i + 1] = part_off[i] + parts[i].ls.size();
    LineTable t;
    t.n = part_off.back();
    const size_t room = std::max<size_t>(t.n, 1);
    t.ls.reset(new uint64_t[room]), t.le.reset(new uint64_t[room]);
    t.seq.reset(new uint32_t[room]), t.s.reset(new uint32_t[room]), t.e.reset(new uint32_t[room]);
    parallel_for(parts.size(), n_threads, [&](size_t pi) {
        Part &P = parts[pi];
        const size_t at = part_off[pi], n = P.ls.size();
        if (!n) return;
        std::memcpy(t.ls.get() + at, P.ls.data(), n * 8);
        std::memcpy(t.le.get() + at, P.le.data(), n * 8);
        std::memcpy(t.seq.get() + at, P.seq.data(), n * 4);
        std::memcpy(t.s.get() + at, P.s.data(), n * 4);
        std::memcpy(t.e.get() + at, P.e.data(), n * 4);
        P = Part{};
    });
    return t;
}

// Join B on the device (commands/intersect.rs:500-521): keep[i] for line i, against the regions on the host (flat) or in `store`
std::vector<uint8_t> join_b(const LineTable &t, int device, const uint32_t *flat, uint64_t n_regions, gffx_hip_regions *store,
                            uint32_t n_seq, OverlapMode mode) {
    std::vector<uint8_t> keep(std::max<size_t>(t.n, 1), 0);
    if (!t.n) return keep;
    LinesHandle lines;
    if (gffx_hip_lines_create(device, t.n, t.seq.get(), t.s.get(), t.e.get(), OutPtr(lines)) != GFFX_OK) hip_fail("gffx_hip_lines_create");
    const int rc = store ? gffx_hip_lines_test_store(lines.get(), store, n_seq, static_cast<int>(mode), keep.data())
                         : gffx_hip_lines_test(lines.get(), flat, n_regions, n_seq, static_cast<int>(mode), keep.data());
    lines.reset();
    if (rc != GFFX_OK) hip_fail("gffx_hip_lines_test");
    return keep;
}

// kept lines that touch in the file leave as one write: (offset, length)
std::vector<std::pair<uint64_t, uint64_t>> kept_runs(const LineTable &t, const std::vector<uint8_t> &keep) {
    std::vector<std::pair<uint64_t, uint64_t>> seg;
    for (size_t i = 0; i < t.n;) {
        if (!keep[i]) {
            ++i;
            continue;
        }
        size_t j = i + 1;
        while (j < t.n && keep[j] && t.ls[j] == t.le[j - 1]) ++j;
        seg.emplace_back(t.ls[i], t.le[j - 1] - t.ls[i]);
        i = j;
    }
    return seg;
}

}  // namespace

// The body of write_gff_match_only_by_coords with the regions either on the host (flat triples) or already in a device
// region store (the streaming CLI); has_regions[seqid] = the seqid owns at least one region (query_ivmap's keys).
void write_matched_lines(const std::string &gff_path, const std::vector<Block> &blocks, const std::vector<char> &has,
                         const uint32_t *flat, uint64_t n_regions, gffx_hip_regions *store,
                         const std::vector<std::string> &num_to_seqid, const std::optional<std::string> &types_filter,
                         const std::optional<std::string> &output_path, OverlapMode mode, bool verbose, size_t threads, int device,
                         const index_loader::GofMap *gof) {
    const MappedFile gff = map_file_or(gff_path, "Cannot open GFF: \"" + gff_path + "\"");
    LineFilter F;
    F.data = gff.view();
    F.by_type = types_filter.has_value();
    F.allow = split_types(types_filter);
    {
        // the reference goes name -> num -> name; with duplicate names the later number owns the name
        std::unordered_map<std::string_view, uint32_t> name_to_num;
        for (uint32_t i = 0; i < num_to_seqid.size(); ++i) name_to_num[num_to_seqid[i]] = i;
        for (const auto &[name, num] : name_to_num)
            if (num < has.size() && has[num]) F.seq_with_regions.emplace(name, num);
    }
    F.ranges = hit_ranges(blocks, gff.size());
    StageTimer sub{verbose};
    const bool use_all = open_all_lines(F, gff_path, gof, verbose);
    const size_t n_threads = std::max<size_t>(1, std::min<size_t>(threads ? threads : 1, 64));
    std::vector<Part> parts;
    if (!build_parts(F, use_all, n_threads, parts)) {  // the image does not describe these blocks (offsets that are not line starts, damage)
        std::fprintf(stderr, "[WARN] %s.lall does not match the index's blocks; parsing the GFF text instead\n", gff_path.c_str());
        build_parts(F, false, n_threads, parts);
    }
    const LineTable table = concat_parts(parts, n_threads);
    sub.lap("  line table of the hit blocks (host threads)");
    const std::vector<uint8_t> keep = join_b(table, device, flat, n_regions, store, static_cast<uint32_t>(num_to_seqid.size()), mode);
    sub.lap("  Join B on the device (region sort + tables + k_lines_exists + flags back)");
    const std::vector<std::pair<uint64_t, uint64_t>> seg = kept_runs(table, keep);
    sub.lap("  runs of kept lines");
    write_segments(gff.data(), seg, output_path, threads);
    sub.lap("  writing the kept lines");
    if (verbose) std::fprintf(stderr, "[INFO] match-only by coords completed; minput blocks %zu\n", blocks.size());
}

void write_gff_match_only_by_coords(const std::string &gff_path, const std::vector<Block> &blocks,
                                    const std::vector<Region> &regions, const std::vector<std::string> &num_to_seqid,
                                    const std::optional<std::string> &types_filter,
                                    const std::optional<std::string> &output_path, OverlapMode mode, bool verbose,
                                    size_t threads, int device, const index_loader::GofMap *gof) {
    std::vector<char> has(num_to_seqid.size(), 0);
    for (const auto &r : regions)
        if (std::get<0>(r) < has.size()) has[std::get<0>(r)] = 1;
    const std::vector<uint32_t> flat = flatten(regions);
    write_matched_lines(gff_path, blocks, has, flat.data(), regions.size(), nullptr, num_to_seqid, types_filter, output_path, mode,
                        verbose, threads, device, gof);
}

}  // namespace gffx::commands::intersect
