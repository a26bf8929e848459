// filtered_output.hpp -- the host half of write_gff_output_filtered (utils/common.rs:289-465) that `gffx extract` and
// `gffx search` share: the hit blocks in output order, their line boundaries (from `<gff>.lall` or from the text), the
// packing of the lines into chunks for the device's per-line test, and the copy-out of the kept lines.  The test itself
// is the caller's: extract asks gffx_hip_ids_filter_lines (key "ID"), search asks gffx_hip_attrs_filter_lines
// (key `<attribute name>`).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gffx.hpp"

namespace gffx::filtered {

using commands::intersect::AllLinesView;

struct Names {  // strings back to back
    std::string bytes;
    std::vector<uint64_t> off{0};
    size_t size() const { return off.size() - 1; }
    void push(std::string_view s) {
        bytes.append(s);
        off.push_back(bytes.size());
    }
    std::string_view at(size_t i) const { return std::string_view(bytes).substr(off[i], off[i + 1] - off[i]); }
};

// prt.rs:108-125: word i = the parent of fid i
inline std::vector<uint32_t> load_prt(const std::string &gff) {
    const std::string path = append_suffix(gff, ".prt");
    const MappedFile f = map_file_or(path, "Failed to mmap " + path);
    if (f.size() % 4 != 0) throw Error("Corrupted PRT: not aligned to u32");
    std::vector<uint32_t> prt(f.size() / 4);
    for (size_t i = 0; i < prt.size(); ++i) prt[i] = get_le32(f.data() + 4 * i);
    return prt;
}

inline size_t chunk_budget() {  // GFFX_EXTRACT_CHUNK_BYTES: text bytes per device pass of the line filter (results never depend on it)
    const char *e = std::getenv("GFFX_EXTRACT_CHUNK_BYTES");
    if (e && *e) {
        const long long v = std::atoll(e);
        if (v > 0) return static_cast<size_t>(v);
    }
    return size_t(64) << 20;
}

struct HitLines {  // the lines of the hit blocks in output order: [ls, le) with the line ending, the root of the block
    std::vector<uint64_t> ls, le;
    std::vector<uint32_t> root;
};

// common.rs:323-335: blocks in order of their start, cut at the file's end, empty ones dropped (a sentinel start is >= any end)
inline std::vector<Block> hit_ranges(const std::vector<Block> &blocks, uint64_t file_len) {
    std::vector<Block> r;
    for (const auto &[root, s, e] : blocks) {
        const uint64_t ee = std::min<uint64_t>(e, file_len);
        if (s >= ee) continue;
        r.emplace_back(root, s, ee);
    }
    std::sort(r.begin(), r.end(), [](const Block &a, const Block &b) {
        return std::make_tuple(std::get<1>(a), std::get<2>(a), std::get<0>(a)) < std::make_tuple(std::get<1>(b), std::get<2>(b), std::get<0>(b));
    });
    return r;
}

// the line boundaries from the all-line image `<gff>.lall`: it lists exactly the non-empty lines that do not begin with '#'
// (the others are never kept: no TAB, or the '#').  false: the image does not describe these blocks.
inline bool lines_from_table(const AllLinesView &all, const std::vector<Block> &ranges, HitLines &L) {
    for (const auto &[root, s, e] : ranges) {
        uint64_t lo, hi;
        if (!all.block_lines(s, e, lo, hi)) return false;
        uint64_t at = s;
        for (uint64_t i = lo; i < hi; ++i) {
            const uint64_t l0 = all.ls[i], l1 = l0 + all.len[i];
            if (l0 < at || l1 > e || all.len[i] == 0) return false;
            at = l1;
            L.ls.push_back(l0), L.le.push_back(l1), L.root.push_back(root);
        }
    }
    return true;
}

// ... or from the text (common.rs:342-359): every line of [s, e), the '#' ones too (the device skips them)
inline void lines_from_text(std::string_view data, const std::vector<Block> &ranges, HitLines &L) {
    for (const auto &[root, s, e] : ranges) {
        for (uint64_t pos = s; pos < e;) {
            const void *nl = std::memchr(data.data() + pos, '\n', e - pos);
            const uint64_t next = nl ? static_cast<uint64_t>(static_cast<const char *>(nl) - data.data()) + 1 : e;
            L.ls.push_back(pos), L.le.push_back(next), L.root.push_back(root);
            pos = next;
        }
    }
}

// the -T strings (common.rs:306-311) back to back, as the device takes them
struct TypeList {
    std::string bytes;
    std::vector<uint32_t> off{0};
    uint32_t n = 0;
    explicit TypeList(const std::optional<std::string> &types_filter) {
        for (const std::string &t : split_types(types_filter)) {
            bytes += t;
            off.push_back(static_cast<uint32_t>(bytes.size()));
            ++n;
        }
    }
};

// common.rs:289-465: the lines of the hit blocks go to the device in chunks cut at line boundaries (a line longer than the
// budget is a chunk of its own), the kept ones are written in block order.  test(text, n_bytes, n_lines, line_off, line_root,
// keep) fills keep[0, n_lines) on the device; filter_lap names its stage timer.
template <typename Test>
void write_gff_output_filtered(const std::string &gff_path, const std::vector<Block> &blocks, const index_loader::GofMap &gof,
                               const std::optional<std::string> &output_path, bool verbose, size_t threads, const char *filter_lap,
                               Test &&test) {
    const MappedFile gff = map_file_or(gff_path, "Cannot open GFF file: \"" + gff_path + "\"");
    const std::vector<Block> ranges = hit_ranges(blocks, gff.size());
    StageTimer sub{verbose};
    HitLines L;
    {
        AllLinesView all;
        const char *lt = std::getenv("GFFX_LINE_TABLE");
        std::string why = "disabled";
        bool use_all = false;
        if (!(lt && std::string(lt) == "parse"))
            use_all = all.open(append_suffix(gff_path, ".lall"), gff.size(), index_loader::line_table_key(gff_path, gof), why);
        if (use_all && !lines_from_table(all, ranges, L)) {
            std::fprintf(stderr, "[WARN] %s.lall does not match the index's blocks; reading the GFF text instead\n", gff_path.c_str());
            use_all = false;
            why = "does not match the blocks";
        }
        if (!use_all) {
            L = HitLines{};
            lines_from_text(gff.view(), ranges, L);
        }
        if (verbose)
            std::fprintf(stderr, use_all ? "[INFO] line boundaries from %s.lall\n" : "[INFO] all-line table not used (%s): line boundaries from the text\n",
                         use_all ? gff_path.c_str() : why.c_str());
    }
    sub.lap("  line boundaries of the hit blocks");
    const size_t budget = chunk_budget(), n = L.ls.size();
    std::vector<uint8_t> text, keep;
    std::vector<uint64_t> off;
    std::vector<std::pair<uint64_t, uint64_t>> seg;  // kept lines that touch in the file leave as one write
    uint64_t last_end = UINT64_MAX;
    size_t chunks = 0, kept = 0;
    for (size_t i = 0; i < n;) {
        size_t j = i;
        uint64_t bytes = 0;
        while (j < n && (j == i || bytes + (L.le[j] - L.ls[j]) <= budget)) bytes += L.le[j] - L.ls[j], ++j;
        text.resize(bytes);
        off.assign(1, 0);
        for (size_t k = i; k < j; ++k) {
            std::memcpy(text.data() + off.back(), gff.data() + L.ls[k], L.le[k] - L.ls[k]);
            off.push_back(off.back() + (L.le[k] - L.ls[k]));
        }
        keep.assign(j - i, 0);
        test(text.data(), bytes, j - i, off.data(), L.root.data() + i, keep.data());
        for (size_t k = i; k < j; ++k) {
            if (!keep[k - i]) continue;
            ++kept;
            if (!seg.empty() && L.ls[k] == last_end)
                seg.back().second += L.le[k] - L.ls[k];
            else
                seg.emplace_back(L.ls[k], L.le[k] - L.ls[k]);
            last_end = L.le[k];
        }
        ++chunks;
        i = j;
    }
    sub.lap(filter_lap);
    write_segments(gff.data(), seg, output_path, threads);
    sub.lap("  writing the kept lines");
    g_run_stats.count("lines_tested", static_cast<double>(n));
    g_run_stats.count("lines_kept", static_cast<double>(kept));
    g_run_stats.count("filter_chunks", static_cast<double>(chunks));
}

}  // namespace gffx::filtered
