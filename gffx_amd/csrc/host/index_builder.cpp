// index_builder.cpp -- `gffx index`: one pass over the GFF text -> the eight side-car files
// (reference: index_builder/core.rs:41-242; formats: SURVEY.md Appendix A).
//
// What parity depends on (and is therefore reproduced literally):
//   * a feature's numeric id is the index of the LAST non-skipped line carrying its ID= value
//     (feature_map.insert overwrites: core.rs:141-144, fid lookup :160);
//   * a feature is a ROOT iff its Parent= is absent, unseen or a comma list (:163-170); roots
//     alone enter the interval index, as 0-based half-open [start-1, end) with start/end swapped
//     when reversed (:107-109), and open a byte block that ends at the next root's line (:182-185);
//   * seqid numbers are handed out in order of first appearance as a ROOT's seqid (:171-175).
//
// Two producers of the arrays, one writer: build_index walks the text on the host; build_index_device (`gffx index --gpu`)
// feeds it to the engine (gffx_hip_gff_*, device/gff.hip) and takes the arrays back.  write_index builds the trees,
// serialises them and writes the eight files for both.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <unordered_set>

#include "../../../include/gffx_hip.h"
#include "../device/gff_core.hpp"
#include "gffx.hpp"

namespace gffx {

namespace {

// leftmost match of  <key>=([^;\s]+)  (stop_at_ws) or  <key>=([^;]+)
std::optional<std::string_view> capture_after_key(std::string_view line, std::string_view key, bool stop_at_ws) {
    size_t from = 0;
    while (true) {
        const size_t at = line.find(key, from);
        if (at == std::string_view::npos) return std::nullopt;
        const size_t eq = at + key.size();
        if (eq < line.size() && line[eq] == '=') {
            size_t q = eq + 1;
            const size_t q0 = q;
            while (q < line.size() && line[q] != ';' &&
                   !(stop_at_ws && unicode_ws_len(line.data() + q, line.size() - q)))
                ++q;
            if (q > q0) return line.substr(q0, q - q0);
        }
        from = at + 1;
    }
}

struct RawFeature {  // core.rs:59-67
    std::string seqid;
    uint32_t start, end;
    uint64_t line_offset;
    std::string id;
    std::optional<std::string> parent, attr;
};

struct TreeNode {  // utils/tree.rs:17-23, only to lay out .rit
    uint32_t center;
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> ivs;
    int left = -1, right = -1;
};

// utils/tree.rs:35-64, iterative bookkeeping over an arena
int build_tree(std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> ivs, std::vector<TreeNode> &arena) {
    if (ivs.empty()) return -1;
    std::stable_sort(ivs.begin(), ivs.end(), [](const auto &a, const auto &b) { return std::get<0>(a) < std::get<0>(b); });
    const uint32_t center = std::get<0>(ivs[ivs.size() / 2]);
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> l, r, c;
    for (const auto &iv : ivs) {
        if (std::get<1>(iv) < center)
            l.push_back(iv);
        else if (std::get<0>(iv) > center)
            r.push_back(iv);
        else
            c.push_back(iv);
    }
    const int me = static_cast<int>(arena.size());
    arena.push_back(TreeNode{center, std::move(c), -1, -1});
    const int li = build_tree(std::move(l), arena);
    const int ri = build_tree(std::move(r), arena);
    arena[me].left = li;
    arena[me].right = ri;
    return me;
}

// bincode 1.x default layout of IntervalTree<u32> (hypothesis):
// Option tag u8 | center u32 | len u64 | (start,end,root_fid) u32 x3 ... | left | right
void serialize_tree(const std::vector<TreeNode> &arena, int node, std::string &out) {
    if (node < 0) {
        out.push_back('\0');
        return;
    }
    out.push_back('\1');
    const TreeNode &n = arena[node];
    put_le32(out, n.center);
    put_le64(out, n.ivs.size());
    for (const auto &[s, e, f] : n.ivs) {
        put_le32(out, s);
        put_le32(out, e);
        put_le32(out, f);
    }
    serialize_tree(arena, n.left, out);
    serialize_tree(arena, n.right, out);
}

// what both producers hand to the writer
struct IndexArrays {
    std::string fts, gof, prt, a2f;  // the files' bytes
    std::string sqs, atn;            // the names in number order, a '\n' after each (.atn without its "#attribute=" line)
    std::vector<std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>> trees_input;  // per seqid, in file order
};

// .rit / .rix (core.rs:206-224, utils/tree_io.rs:37-63) and the eight files
void write_index(const std::string &gff, const std::string &attr_key, const IndexArrays &ia) {
    std::string rit, rix = "[";
    for (size_t c = 0; c < ia.trees_input.size(); ++c) {
        if (c) rix.push_back(',');
        rix += std::to_string(rit.size());
        std::vector<TreeNode> arena;
        const int root = build_tree(ia.trees_input[c], arena);
        serialize_tree(arena, root, rit);
    }
    rix.push_back(']');

    const std::string atn_text = "#attribute=" + attr_key + "\n" + ia.atn;

    write_whole_file(append_suffix(gff, ".fts"), ia.fts);
    write_whole_file(append_suffix(gff, ".gof"), ia.gof);
    write_whole_file(append_suffix(gff, ".rit"), rit);
    write_whole_file(append_suffix(gff, ".rix"), rix);
    write_whole_file(append_suffix(gff, ".sqs"), ia.sqs);
    write_whole_file(append_suffix(gff, ".atn"), atn_text);
    write_whole_file(append_suffix(gff, ".a2f"), ia.a2f);
    write_whole_file(append_suffix(gff, ".prt"), ia.prt);
}

const char *kWarnFormat = "[WARN] Attribute value contains invalid chars (.,;) (should be URL-encoded): in '%s'\n";

}  // namespace

void build_index(const std::string &gff, const std::string &attr_key, const std::string &skip_types,
                 bool verbose) {
    std::unordered_set<std::string> skip;  // core.rs:47 split(',') (no trimming)
    {
        size_t a = 0;
        while (true) {
            const size_t c = skip_types.find(',', a);
            skip.insert(skip_types.substr(a, c == std::string::npos ? std::string::npos : c - a));
            if (c == std::string::npos) break;
            a = c + 1;
        }
    }
    if (verbose) std::fprintf(stderr, "Building index for %s ...\n", gff.c_str());
    MappedFile file(gff);
    const std::string_view data = file.view();

    std::vector<RawFeature> raw;
    size_t offset = 0;
    while (offset < data.size()) {  // core.rs:71-138
        size_t nl = data.find('\n', offset);
        if (nl == std::string_view::npos) nl = data.size();
        std::string_view line_bytes = data.substr(offset, nl - offset);
        const uint64_t line_offset = offset;
        offset = nl + 1;
        if (line_bytes.empty() || line_bytes[0] == '#') continue;
        if (!utf8_valid(line_bytes)) throw Error("invalid utf-8 sequence in GFF line at byte " + std::to_string(line_offset));
        const std::string_view line = trim_unicode_ws(line_bytes);
        if (line.empty()) continue;
        std::string_view f[9];
        size_t nf = 0, a = 0;
        while (true) {
            const size_t t = line.find('\t', a);
            if (nf < 9) f[nf] = line.substr(a, t == std::string_view::npos ? std::string_view::npos : t - a);
            ++nf;
            if (t == std::string_view::npos) break;
            a = t + 1;
        }
        if (nf != 9) throw Error("Invalid GFF line (expected 9 columns): " + std::string(line));
        if (skip.count(std::string(f[2]))) {
            if (verbose) std::printf("skip comment feature: %.*s\n", (int)f[2].size(), f[2].data());
            continue;
        }
        const auto s1o = parse_u32_rust(f[3]);
        const auto e1o = parse_u32_rust(f[4]);
        if (!s1o || !e1o) throw Error("invalid digit found in string");
        uint32_t s1 = *s1o, e1 = *e1o;
        if (e1 == 0) continue;
        if (s1 > e1) std::swap(s1, e1);
        const auto id = capture_after_key(line, "ID", true);
        if (!id) throw Error("Missing ID in feature: " + std::string(line));
        RawFeature rf;
        rf.seqid = std::string(f[0]);
        rf.start = s1 ? s1 - 1 : 0;
        rf.end = e1;
        rf.line_offset = line_offset;
        rf.id = std::string(*id);
        if (const auto p = capture_after_key(line, "Parent", true)) rf.parent = std::string(*p);
        if (const auto v = capture_after_key(line, attr_key, false)) {
            rf.attr = std::string(*v);
            if (rf.attr->find_first_of(" ;,") != std::string::npos)
                std::fprintf(stderr, kWarnFormat, rf.attr->c_str());
        }
        raw.push_back(std::move(rf));
    }

    std::unordered_map<std::string_view, uint32_t> feature_map;  // core.rs:141-144
    feature_map.reserve(raw.size() * 2);
    for (size_t i = 0; i < raw.size(); ++i) feature_map[raw[i].id] = static_cast<uint32_t>(i);

    IndexArrays ia;
    std::string &fts = ia.fts, &gof = ia.gof, &prt = ia.prt, &a2f = ia.a2f;
    std::vector<std::string> atn, seqids;
    std::unordered_map<std::string, uint32_t> attr_ids, seq_ids;
    auto &trees_input = ia.trees_input;
    bool have_root = false;
    uint32_t cur_fid = 0, cur_seq = 0;
    uint64_t cur_off = 0;
    auto emit_gof = [&](uint64_t end_off) {  // core.rs:32-38
        put_le32(gof, cur_fid);
        put_le32(gof, cur_seq);
        put_le64(gof, cur_off);
        put_le64(gof, end_off);
    };
    for (const RawFeature &rf : raw) {  // core.rs:159-199
        const uint32_t fid = feature_map[rf.id];
        fts += rf.id;
        fts.push_back('\n');
        uint32_t parent_id = fid;
        if (rf.parent) {
            const auto it = feature_map.find(*rf.parent);
            if (it != feature_map.end()) parent_id = it->second;
        }
        put_le32(prt, parent_id);
        if (parent_id == fid) {
            auto [it, fresh] = seq_ids.try_emplace(rf.seqid, static_cast<uint32_t>(seqids.size()));
            if (fresh) {
                seqids.push_back(rf.seqid);
                trees_input.emplace_back();
            }
            const uint32_t seqnum = it->second;
            trees_input[seqnum].emplace_back(rf.start, rf.end, fid);
            if (have_root) emit_gof(rf.line_offset);
            have_root = true;
            cur_fid = fid;
            cur_off = rf.line_offset;
            cur_seq = seqnum;
        }
        if (rf.attr) {
            auto [it, fresh] = attr_ids.try_emplace(*rf.attr, static_cast<uint32_t>(atn.size()));
            if (fresh) atn.push_back(*rf.attr);
            put_le32(a2f, it->second);
        } else {
            put_le32(a2f, 0xFFFFFFFFu);
        }
    }
    if (have_root) emit_gof(data.size());  // core.rs:201-203

    for (const auto &s : seqids) ia.sqs += s + "\n";
    for (const auto &v : atn) ia.atn += v + "\n";
    write_index(gff, attr_key, ia);
    if (verbose) std::fprintf(stderr, "Index built successfully for %s\n", gff.c_str());
}

void build_index_device(const std::string &gff, const std::string &attr_key, const std::string &skip_types, int device,
                        bool verbose) {
    std::string skip_bytes;  // core.rs:47 split(',') (no trimming)
    std::vector<uint32_t> skip_off{0};
    {
        size_t a = 0;
        while (true) {
            const size_t c = skip_types.find(',', a);
            skip_bytes += skip_types.substr(a, c == std::string::npos ? std::string::npos : c - a);
            skip_off.push_back(static_cast<uint32_t>(skip_bytes.size()));
            if (c == std::string::npos) break;
            a = c + 1;
        }
    }
    if (attr_key.find('\0') != std::string::npos) throw Error("the attribute key holds a NUL byte");
    if (verbose) std::fprintf(stderr, "Building index for %s ...\n", gff.c_str());
    MappedFile file(gff);
    const std::string_view data = file.view();

    uint64_t chunk = 0;  // GFFX_INDEX_CHUNK_BYTES: the text bytes per device pass (0 / unset: the engine's 64 MiB)
    if (const char *e = std::getenv("GFFX_INDEX_CHUNK_BYTES")) chunk = std::strtoull(e, nullptr, 10);
    gffx_hip_gff *h = nullptr;
    auto engine_error = [&]() { return Error(std::string("gffx index --gpu: ") + gffx_hip_last_error()); };
    if (gffx_hip_gff_create(device, attr_key.c_str(), static_cast<uint32_t>(skip_off.size() - 1), skip_bytes.data(), skip_off.data(), chunk, -1, &h) !=
        GFFX_OK)
        throw engine_error();
    struct Closer {
        gffx_hip_gff *h;
        ~Closer() { gffx_hip_gff_destroy(h); }
    } closer{h};

    const uint8_t *text = reinterpret_cast<const uint8_t *>(data.data());
    int rc = gffx_hip_gff_feed(h, text, data.size());
    if (rc == GFFX_OK) rc = gffx_hip_gff_finish(h);
    if (rc != GFFX_OK) {
        uint64_t off = 0;
        int kind = 0;
        gffx_hip_gff_error(h, &off, &kind);
        if (kind == 0 || off > data.size()) throw engine_error();
        // the host path's message for the line the device names
        size_t nl = data.find('\n', off);
        if (nl == std::string_view::npos) nl = data.size();
        const std::string line(trim_unicode_ws(data.substr(off, nl - off)));
        switch (kind) {
            case gff::kBadUtf8: throw Error("invalid utf-8 sequence in GFF line at byte " + std::to_string(off));
            case gff::kColumns: throw Error("Invalid GFF line (expected 9 columns): " + line);
            case gff::kDigits: throw Error("invalid digit found in string");
            default: throw Error("Missing ID in feature: " + line);
        }
    }

    IndexArrays ia;
    auto take = [&](int r) {
        if (r != GFFX_OK) throw engine_error();
    };
    const uint64_t n_rows = gffx_hip_gff_n_rows(h), n_roots = gffx_hip_gff_n_roots(h);
    ia.fts.resize(gffx_hip_gff_fts_bytes(h));
    ia.prt.resize(4 * n_rows);
    ia.a2f.resize(4 * n_rows);
    ia.gof.resize(24 * n_roots);
    ia.sqs.resize(gffx_hip_gff_seqids_bytes(h));
    ia.atn.resize(gffx_hip_gff_atn_bytes(h));
    auto u8 = [](std::string &s) { return reinterpret_cast<uint8_t *>(s.data()); };
    auto u32 = [](std::string &s) { return reinterpret_cast<uint32_t *>(s.data()); };  // (the files are little-endian, as the host is)
    take(gffx_hip_gff_copy_fts(h, u8(ia.fts)));
    take(gffx_hip_gff_copy_prt(h, u32(ia.prt)));
    take(gffx_hip_gff_copy_a2f(h, u32(ia.a2f)));
    take(gffx_hip_gff_copy_gof(h, u8(ia.gof)));
    take(gffx_hip_gff_copy_seqids(h, u8(ia.sqs)));
    take(gffx_hip_gff_copy_atn(h, u8(ia.atn)));
    std::vector<uint32_t> roots(4 * n_roots);
    take(gffx_hip_gff_copy_roots(h, roots.data()));
    uint64_t n_seq = 0;
    take(gffx_hip_gff_counts(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_seq, nullptr));
    ia.trees_input.resize(n_seq);  // the roots per seqid, in file order: what the stable sort of build_tree sees today
    for (uint64_t k = 0; k < n_roots; ++k) {
        const uint32_t seq = roots[4 * k + 3];
        if (seq >= n_seq) throw Error("gffx index --gpu: a root with seqid number " + std::to_string(seq) + " of " + std::to_string(n_seq));
        ia.trees_input[seq].emplace_back(roots[4 * k], roots[4 * k + 1], roots[4 * k + 2]);
    }

    if (verbose) {  // the `skip comment feature` lines, in file order
        std::vector<uint64_t> skipped(gffx_hip_gff_n_skipped_lines(h));
        take(gffx_hip_gff_copy_skipped_lines(h, skipped.data()));
        for (const uint64_t off : skipped) {
            if (off > data.size()) continue;
            size_t nl = data.find('\n', off);
            if (nl == std::string_view::npos) nl = data.size();
            const std::string_view line = trim_unicode_ws(data.substr(off, nl - off));
            size_t a = 0;
            for (int k = 0; k < 2 && a != std::string_view::npos; ++k) {
                a = line.find('\t', a);
                if (a != std::string_view::npos) ++a;
            }
            if (a == std::string_view::npos) continue;
            const size_t z = line.find('\t', a);
            const std::string_view ty = line.substr(a, z == std::string_view::npos ? std::string_view::npos : z - a);
            std::printf("skip comment feature: %.*s\n", (int)ty.size(), ty.data());
        }
    }
    {  // the [WARN] lines, one per flagged row in file order: the row's value is name a2f[row] of .atn
        std::vector<uint32_t> warn(gffx_hip_gff_n_warn_rows(h));
        take(gffx_hip_gff_copy_warn_rows(h, warn.data()));
        if (!warn.empty()) {
            std::vector<size_t> name_at{0};
            for (size_t i = 0; i < ia.atn.size(); ++i)
                if (ia.atn[i] == '\n') name_at.push_back(i + 1);
            const uint32_t *a2f = u32(ia.a2f);
            for (const uint32_t row : warn) {
                if (row >= n_rows || a2f[row] + 1 >= name_at.size()) continue;
                const std::string v = ia.atn.substr(name_at[a2f[row]], name_at[a2f[row] + 1] - 1 - name_at[a2f[row]]);
                std::fprintf(stderr, kWarnFormat, v.c_str());
            }
        }
    }
    write_index(gff, attr_key, ia);
    if (verbose) std::fprintf(stderr, "Index built successfully for %s\n", gff.c_str());
}

}  // namespace gffx
