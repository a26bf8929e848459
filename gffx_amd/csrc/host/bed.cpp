// bed.cpp -- the host side of a BED source read on the device, for `gffx intersect -b`, `gffx depth -s` and `gffx coverage -s`.
// The content decides the route, as in sam.cpp: a file that begins with the gzip magic is BGZF (the BC extra field: its members
// go to the engine, whose inflated bytes never leave the device) or refused (plain gzip has no block structure to inflate in
// parallel; the message names bgzip); anything else is text, which goes to the host parsers unless GFFX_BED_DEVICE=1 sends it
// through the same device reader (gffx_hip_bed_*, device/bed.hip).  The engine finds the lines, cuts the fields, reads the
// coordinates and looks the names up by the rules of the command's host parser (the dialect; device/bed_core.hpp) and hands
// back the kept (seqid number, start, end) rows in file order: what both host parsers give, unchanged.
// The BGZF front end (directory, EOF marker, chunked feed) is bgzf_file.hpp's and the read-back of times, rows and tallies
// source_read.hpp's, both shared with bam.cpp and sam.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "source_read.hpp"

namespace gffx::bed {

namespace {
const source::Reader<gffx_hip_bed> kReader = {gffx_hip_bed_stage_ms, gffx_hip_bed_rows, gffx_hip_bed_copy_rows, gffx_hip_bed_counts,
                                              {"BED inflate (device)", "BED line scan (device)", "BED rows (device)",
                                               "BED chunks in all (staging, device, rows back)", "BED rows copy"}};

bool knob_on() {  // GFFX_BED_DEVICE: unset, empty or 0 is the host parser
    const char *e = std::getenv("GFFX_BED_DEVICE");
    return e && *e && std::strcmp(e, "0") != 0;
}
}  // namespace

Route route(const std::string &path) {
    uint8_t magic[2] = {0, 0};
    size_t got = 0;
    if (FILE *f = std::fopen(path.c_str(), "rb")) {
        got = std::fread(magic, 1, 2, f);
        std::fclose(f);
    } else {
        return Route::Host;  // (the host path reports a file that does not open, in its command's words)
    }
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) return Route::Device;
    return knob_on() ? Route::Device : Route::Host;
}

std::vector<uint32_t> read_rows(const std::string &path, const std::unordered_map<std::string, uint32_t> &seqid_to_num, int dialect,
                                int device, bool verbose) {
    using source::clock;
    using source::ms_since;
    const source::Timer timer{verbose};
    const std::string who = "BED file \"" + path + "\"";
    const MappedFile f = map_file_or(path, "cannot open " + who);
    const std::string_view v = f.view();
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    const uint64_t n = v.size();
    std::vector<uint64_t> member_off;  // BGZF: member i = [member_off[i], member_off[i + 1])
    bool bgzf_text = false;
    if (n >= 2 && p[0] == 0x1f && p[1] == 0x8b) {
        uint64_t bad_off = 0;
        if (const int st = bgzf_file::member_directory(p, n, &member_off, &bad_off)) {
            if (st == bgzf::kHeader && bad_off == 0)
                throw Error(who + " is gzip-compressed but not BGZF (no BC extra field): recompress it with bgzip, or decompress it");
            throw Error(who + ": BGZF block at file offset " + std::to_string(bad_off) + ": " + bgzf::status_name(st));
        }
        bgzf_text = true;
        if (!bgzf_file::has_eof_marker(p, n))
            std::fprintf(stderr, "[WARN] BED file \"%s\" has no BGZF EOF marker: it may be truncated\n", path.c_str());
    }
    // the engine numbers the names by their rank here; num[i] = the index's seqid number of name i
    std::vector<std::pair<uint32_t, const std::string *>> order;
    order.reserve(seqid_to_num.size());
    for (const auto &kv : seqid_to_num) order.emplace_back(kv.second, &kv.first);
    std::sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first < b.first : *a.second < *b.second; });
    std::string names;
    std::vector<uint64_t> name_off{0};
    bool identity = true;
    for (size_t i = 0; i < order.size(); ++i) {
        names += *order[i].second;
        name_off.push_back(names.size());
        identity = identity && order[i].first == i;
    }

    const auto t = clock::now();
    const uint64_t chunk = source::chunk_bytes_from_env("GFFX_BED_CHUNK_BYTES", 0);  // (0: the engine's default)
    Handle<gffx_hip_bed, gffx_hip_bed_destroy> owner;
    // a malformed line: the host parser's message, as it is.  A member that does not inflate: the engine's, with the file's name
    auto engine_error = [&]() {
        const std::string msg = gffx_hip_last_error();
        return Error(msg.rfind("BGZF", 0) == 0 ? who + ": " + msg : msg);
    };
    if (gffx_hip_bed_create(device, (uint32_t)order.size(), names.data(), name_off.data(), dialect, chunk, bgzf_text ? 1 : 0, OutPtr(owner)) !=
        GFFX_OK)
        hip_fail("gffx_hip_bed_create");
    gffx_hip_bed *h = owner.get();
    auto feed = [&](const uint8_t *q, uint64_t nb) { return gffx_hip_bed_feed(h, q, nb) == GFFX_OK; };
    if (!(bgzf_text ? bgzf_file::feed_chunks(p, member_off, chunk ? chunk : (64ull << 20), feed) : feed(p, n))) throw engine_error();
    if (gffx_hip_bed_finish(h) != GFFX_OK) throw engine_error();
    uint64_t c[4] = {0, 0, 0, 0};  // lines, skipped, no_seq, kept
    std::vector<uint32_t> rows = source::take_rows(h, kReader, timer, ms_since(t), c, engine_error);
    if (!identity)
        for (size_t i = 0; i < rows.size(); i += 3) rows[i] = order[rows[i]].first;
    if (verbose)
        std::fprintf(stderr, "[INFO] BED on the device: %s, %llu lines, %llu skipped, %llu without a seqid of the index, %llu rows kept\n",
                     bgzf_text ? "BGZF text" : "plain text", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                     (unsigned long long)c[3]);
    g_run_stats.count("bed_lines", (double)c[0]);
    g_run_stats.count("bed_rows_kept", (double)c[3]);
    return rows;
}

}  // namespace gffx::bed
