// layer_rows.hpp -- the rows of the class map's layers from a GFF file and the map built from them, shared by `gffx annotate`
// and `gffx enrich` (`gffx meta` takes its features the same way): -T names the layers in priority order, the lines come from
// the all-line table `<gff>.lall` (or from the text when there is none: GFFX_LINE_TABLE=parse, a stale or missing image).
#pragma once
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

#include "intersect_internal.hpp"

namespace gffx::commands::layer_rows {

// The layers' rows (layer, seqid number, start - 1, end) from the all-line table's columns.  A line counts when its type is
// one of the names, its split succeeded and 1 <= start <= end; a line on a seqid the index does not know is skipped.
// seq_end (unless NULL, sized by the caller to the index's seqids): the largest end of ANY such valid line per seqid, whatever
// its type.  line_start (unless NULL; ls: where every line begins in the text): per row where its line begins (`gffx meta`
// reads the strand and the ID there: feature_rows.hpp).
template <typename Names>
void collect_rows(uint64_t n_lines, const uint32_t *start, const uint32_t *end, const uint32_t *seq, const uint32_t *type, const uint8_t *flags,
                  const Names &seq_names, const Names &type_names, const std::vector<std::string> &layers,
                  const std::unordered_map<std::string, uint32_t> &seqid_to_num, std::vector<uint32_t> &rows, std::vector<uint64_t> &per_layer, uint64_t &skipped,
                  std::vector<uint32_t> *seq_end, const uint64_t *ls = nullptr, std::vector<uint64_t> *line_start = nullptr) {
    std::vector<uint32_t> layer_of(type_names.size(), UINT32_MAX), seq_of(seq_names.size(), UINT32_MAX);
    for (size_t i = 0; i < type_names.size(); ++i)
        for (size_t k = 0; k < layers.size(); ++k)
            if (std::string_view(type_names[i]) == layers[k]) layer_of[i] = static_cast<uint32_t>(k);
    for (size_t i = 0; i < seq_names.size(); ++i) {
        const auto it = seqid_to_num.find(std::string(seq_names[i]));
        if (it != seqid_to_num.end()) seq_of[i] = it->second;
    }
    for (uint64_t i = 0; i < n_lines; ++i) {
        if (seq_end && (flags[i] & 1u) && start[i] >= 1 && start[i] <= end[i] && seq[i] < seq_of.size() && seq_of[seq[i]] < seq_end->size())
            (*seq_end)[seq_of[seq[i]]] = std::max((*seq_end)[seq_of[seq[i]]], end[i]);
        // (0xFFFFFFFF marks a type that gff_type_allowed rejects whatever the filter: it is no index into the names)
        if (type[i] >= layer_of.size() || layer_of[type[i]] == UINT32_MAX || !(flags[i] & 1u)) continue;
        if (start[i] < 1 || start[i] > end[i]) continue;
        if (seq[i] >= seq_of.size() || seq_of[seq[i]] == UINT32_MAX) {
            ++skipped;
            continue;
        }
        const uint32_t k = layer_of[type[i]];
        rows.insert(rows.end(), {k, seq_of[seq[i]], start[i] - 1, end[i]});
        per_layer[k]++;
        if (line_start) line_start->push_back(ls[i]);
    }
}

// ... from the file: its line table when it is usable, else its text
inline void collect(const std::string &gff_path, const std::vector<std::string> &layers, const std::unordered_map<std::string, uint32_t> &seqid_to_num, size_t threads,
                    bool verbose, std::vector<uint32_t> &rows, std::vector<uint64_t> &per_layer, uint64_t &skipped, std::vector<uint32_t> *seq_end,
                    std::vector<uint64_t> *line_start = nullptr) {
    const MappedFile gff = map_file_or(gff_path, "Cannot open GFF file: \"" + gff_path + "\"");
    const char *lt = std::getenv("GFFX_LINE_TABLE");
    std::string why = "disabled";
    intersect::AllLinesView all;
    bool use_all = false;
    if (!(lt && std::string(lt) == "parse")) {
        const index_loader::GofMap gof = index_loader::load_gof(gff_path);
        use_all = all.open(append_suffix(gff_path, ".lall"), gff.size(), index_loader::line_table_key(gff_path, gof), why);
    }
    if (use_all) {
        collect_rows(all.n_lines, all.start, all.end, all.seq, all.type, all.flags, all.seq_names, all.type_names, layers, seqid_to_num, rows, per_layer, skipped,
                     seq_end, all.ls, line_start);
    } else {
        const intersect::AllLines A = intersect::build_all_lines(gff.view(), threads);
        collect_rows(A.ls.size(), A.start.data(), A.end.data(), A.seq.data(), A.type.data(), A.flags.data(), A.seq_names, A.type_names, layers, seqid_to_num, rows,
                     per_layer, skipped, seq_end, A.ls.data(), line_start);
    }
    if (verbose && use_all) std::fprintf(stderr, "[INFO] all-line table from %s.lall (%llu lines)\n", gff_path.c_str(), (unsigned long long)all.n_lines);
    if (verbose && !use_all) std::fprintf(stderr, "[INFO] all-line table not used (%s): parsing the text\n", why.c_str());
}

// What the user hears about the layers: a [WARN] line for every name without a line (tail: what that means for the command);
// with debug_cmd (NULL: none of it) a [DEBUG] line per layer and one for the lines that collect() skipped.
inline void report(const std::string &gff_path, const std::vector<std::string> &layers, const std::vector<uint64_t> &per_layer, const char *tail,
                   const char *debug_cmd, uint64_t skipped) {
    for (size_t k = 0; k < layers.size(); ++k) {
        if (!per_layer[k]) std::fprintf(stderr, "[WARN] no line of %s has type '%s'%s\n", gff_path.c_str(), layers[k].c_str(), tail);
        if (debug_cmd) std::fprintf(stderr, "[DEBUG] %s: layer %zu '%s': %llu lines\n", debug_cmd, k, layers[k].c_str(), (unsigned long long)per_layer[k]);
    }
    if (debug_cmd) std::fprintf(stderr, "[DEBUG] %s: %llu lines skipped (a seqid the index does not know)\n", debug_cmd, (unsigned long long)skipped);
}

// The finished class map of collect()'s rows on `device`; the rows are given up.
inline ClassMapHandle build_class_map(int device, uint32_t n_seq, uint32_t n_layers, std::vector<uint32_t> &rows) {
    ClassMapHandle h;
    if (gffx_hip_classmap_create(device, n_seq, n_layers, OutPtr(h)) != GFFX_OK) hip_fail("gffx_hip_classmap_create");
    if (gffx_hip_classmap_add_rows_host(h.get(), rows.data(), rows.size() / 4) != GFFX_OK) hip_fail("gffx_hip_classmap_add_rows_host");
    if (gffx_hip_classmap_finish(h.get()) != GFFX_OK) hip_fail("gffx_hip_classmap_finish");
    std::vector<uint32_t>().swap(rows);
    return h;
}

}  // namespace gffx::commands::layer_rows
