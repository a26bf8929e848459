// bam.cpp -- the host side of a BAM source for `gffx depth` / `gffx coverage` (reference: commands/depth.rs:297-372
// process_bam, commands/coverage.rs:125-168 collect_by_root_from_bam, which read through rust-htslib).  No htslib here:
// the file is mapped, its BGZF block directory is built and checked, the header is inflated on the host with the decoder
// the device uses (bgzf_file.hpp, shared with sam.cpp; this file words the messages and reads the header), and the members
// go to the engine in chunks (gffx_hip_bam_*, device/bgzf.hip; the read-back of times, rows and tallies is source_read.hpp's),
// which inflates, frames and filters the records and hands back the kept (seqid number, start, end) rows in file order --
// what the BED path of both commands takes, unchanged.
#include <cstring>

#include "source_read.hpp"

namespace gffx::bam {

namespace {
std::string offset_error(const std::string &path, uint64_t off, int st) {
    return "BAM file \"" + path + "\": BGZF block at file offset " + std::to_string(off) + ": " + bgzf::status_name(st);
}

const source::Reader<gffx_hip_bam> kReader = {gffx_hip_bam_stage_ms, gffx_hip_bam_rows, gffx_hip_bam_copy_rows, gffx_hip_bam_counts,
                                              {"BAM inflate (device)", "BAM framing (device)", "BAM rows (device)",
                                               "BAM chunks in all (staging, device, rows back)", "BAM rows copy"}};
}  // namespace

std::vector<uint32_t> read_rows(const std::string &path, const std::unordered_map<std::string, uint32_t> &seqid_to_num, int device,
                                bool verbose) {
    using source::clock;
    using source::ms_since;
    const source::Timer timer{verbose};
    const MappedFile f = map_file_or(path, "cannot open BAM file \"" + path + "\" (read without htslib)");
    const std::string_view v = f.view();
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    const uint64_t n = v.size();
    if (n == 0) throw Error("BAM file \"" + path + "\" is empty");

    // block directory: every member's header checked, lengths by hopping BSIZE
    auto t = clock::now();
    std::vector<uint64_t> member_off;  // member i = [member_off[i], member_off[i + 1])
    uint64_t bad_off = 0;
    if (const int st = bgzf_file::member_directory(p, n, &member_off, &bad_off)) throw Error(offset_error(path, bad_off, st));
    const size_t n_members = member_off.size() - 1;
    if (!bgzf_file::has_eof_marker(p, n))
        std::fprintf(stderr, "[WARN] BAM file \"%s\" has no BGZF EOF marker: it may be truncated\n", path.c_str());
    timer("BAM block directory", ms_since(t));

    // the header, inflated on the host (it may span several members; records may begin in its last one)
    t = clock::now();
    std::vector<uint8_t> head;
    uint64_t header_bytes = 0;
    uint32_t n_ref = 0;
    int hst = bgzf::kTruncated;
    auto complete = [&](const std::vector<uint8_t> &h) { return bgzf::bam_header_size(h.data(), h.size(), &header_bytes, &n_ref); };
    if (const int st = bgzf_file::inflate_header(p, member_off, &head, complete, &hst, &bad_off)) throw Error(offset_error(path, bad_off, st));
    if (hst == bgzf::kTruncated) throw Error("BAM file \"" + path + "\" ends inside its header");
    if (hst != bgzf::kOk) throw Error("\"" + path + "\" is not a BAM file (bad magic or header)");
    // tid -> seqid number (depth.rs:320-326); names the index does not know map to UINT32_MAX
    std::vector<uint32_t> ref_seq(n_ref, 0xFFFFFFFFu);
    {
        uint64_t at = 8 + (uint64_t)bgzf::le32(head.data() + 4) + 4;
        for (uint32_t r = 0; r < n_ref; ++r) {
            const uint32_t l_name = bgzf::le32(head.data() + at);
            std::string name(reinterpret_cast<const char *>(head.data() + at + 4), l_name);
            const size_t nul = name.find('\0');
            if (nul != std::string::npos) name.resize(nul);
            const auto it = seqid_to_num.find(name);
            if (it != seqid_to_num.end()) ref_seq[r] = it->second;
            at += 8 + l_name;
        }
    }
    timer("BAM header", ms_since(t));

    // the members in chunks of about chunk_bytes, through the engine
    t = clock::now();
    const uint64_t chunk = source::chunk_bytes_from_env("GFFX_BAM_CHUNK_BYTES", 256ull << 20);
    Handle<gffx_hip_bam, gffx_hip_bam_destroy> owner;
    if (gffx_hip_bam_create(device, n_ref, ref_seq.data(), header_bytes, chunk, OutPtr(owner)) != GFFX_OK) hip_fail("gffx_hip_bam_create");
    gffx_hip_bam *h = owner.get();
    auto engine_error = [&]() { return Error("BAM file \"" + path + "\": " + gffx_hip_last_error()); };
    if (!bgzf_file::feed_chunks(p, member_off, chunk, [&](const uint8_t *q, uint64_t nb) { return gffx_hip_bam_feed(h, q, nb) == GFFX_OK; }))
        throw engine_error();
    if (gffx_hip_bam_finish(h) != GFFX_OK) throw engine_error();
    uint64_t c[4] = {0, 0, 0, 0};  // records, unmapped, no_seq, kept
    std::vector<uint32_t> rows = source::take_rows(h, kReader, timer, ms_since(t), c, engine_error);
    if (verbose)
        std::fprintf(stderr, "[INFO] BAM: %zu members, %llu records, %llu unmapped, %llu without a seqid of the index, %llu rows kept\n",
                     n_members, (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3]);
    g_run_stats.count("bam_records", (double)c[0]);
    g_run_stats.count("bam_rows_kept", (double)c[3]);
    return rows;
}

}  // namespace gffx::bam
