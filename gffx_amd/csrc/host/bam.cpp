// bam.cpp -- the host side of a BAM source for `gffx depth` / `gffx coverage` (reference: commands/depth.rs:297-372
// process_bam, commands/coverage.rs:125-168 collect_by_root_from_bam, which read through rust-htslib).  No htslib here:
// the file is mapped, its BGZF block directory is built and checked, the header is inflated on the host with the decoder
// the device uses (device/bgzf_core.hpp), and the members go to the engine in chunks (gffx_hip_bam_*, device/bgzf.hip),
// which inflates, frames and filters the records and hands back the kept (seqid number, start, end) rows in file order --
// what the BED path of both commands takes, unchanged.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../device/bgzf_core.hpp"
#include "gffx.hpp"

namespace gffx::bam {

namespace {
// the 28-byte empty member that ends a BGZF file (SAM spec §4.1.2)
const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

std::string offset_error(const std::string &path, uint64_t off, int st) {
    return "BAM file \"" + path + "\": BGZF block at file offset " + std::to_string(off) + ": " + bgzf::status_name(st);
}

uint64_t chunk_bytes_from_env() {
    const char *e = std::getenv("GFFX_BAM_CHUNK_BYTES");
    if (e && *e) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end && !*end && v > 0) return v;
    }
    return 256ull << 20;
}
}  // namespace

std::vector<uint32_t> read_rows(const std::string &path, const std::unordered_map<std::string, uint32_t> &seqid_to_num, int device,
                                bool verbose) {
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
    auto timer = [&](const char *what, double ms) {
        if (verbose) std::fprintf(stderr, "[TIMER] [run] %s took %.3f ms\n", what, ms);
        g_run_stats.stage(what, ms);
    };
    const MappedFile f = map_file_or(path, "cannot open BAM file \"" + path + "\" (read without htslib)");
    const std::string_view v = f.view();
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    const uint64_t n = v.size();
    if (n == 0) throw Error("BAM file \"" + path + "\" is empty");

    // block directory: every member's header checked, lengths by hopping BSIZE
    auto t = clock::now();
    std::vector<uint64_t> member_off;  // member i = [member_off[i], member_off[i + 1])
    for (uint64_t at = 0; at < n;) {
        uint32_t total = 0, hdr = 0;
        const int st = bgzf::member_header(p + at, n - at, &total, &hdr);
        if (st != bgzf::kOk) throw Error(offset_error(path, at, st));
        member_off.push_back(at);
        at += total;
    }
    member_off.push_back(n);
    const size_t n_members = member_off.size() - 1;
    if (n < 28 || std::memcmp(p + n - 28, kEof, 28) != 0)
        std::fprintf(stderr, "[WARN] BAM file \"%s\" has no BGZF EOF marker: it may be truncated\n", path.c_str());
    timer("BAM block directory", ms_since(t));

    // the header, inflated on the host (it may span several members; records may begin in its last one)
    t = clock::now();
    std::vector<uint8_t> head;
    std::unique_ptr<bgzf::Scratch> scratch(new bgzf::Scratch);
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; ++i) crc_table[i] = bgzf::crc_table_entry(i);
    uint64_t header_bytes = 0;
    uint32_t n_ref = 0;
    int hst = bgzf::kTruncated;
    for (size_t m = 0; m < n_members && hst == bgzf::kTruncated; ++m) {
        const size_t at = head.size();
        head.resize(at + bgzf::kMaxIsize);
        uint32_t total = 0, isize = 0;
        const int st = bgzf::member_inflate(p + member_off[m], member_off[m + 1] - member_off[m], head.data() + at, bgzf::kMaxIsize,
                                            &total, &isize, scratch.get(), crc_table);
        if (st != bgzf::kOk) throw Error(offset_error(path, member_off[m], st));
        head.resize(at + isize);
        hst = bgzf::bam_header_size(head.data(), head.size(), &header_bytes, &n_ref);
    }
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
    const uint64_t chunk = chunk_bytes_from_env();
    Handle<gffx_hip_bam, gffx_hip_bam_destroy> owner;
    if (gffx_hip_bam_create(device, n_ref, ref_seq.data(), header_bytes, chunk, OutPtr(owner)) != GFFX_OK) hip_fail("gffx_hip_bam_create");
    gffx_hip_bam *h = owner.get();
    auto engine_error = [&]() { return Error("BAM file \"" + path + "\": " + gffx_hip_last_error()); };
    for (size_t m = 0; m < n_members;) {
        size_t e = m + 1;
        while (e < n_members && member_off[e + 1] - member_off[m] <= chunk) ++e;
        if (gffx_hip_bam_feed(h, p + member_off[m], member_off[e] - member_off[m]) != GFFX_OK) throw engine_error();
        m = e;
    }
    if (gffx_hip_bam_finish(h) != GFFX_OK) throw engine_error();
    const double feed_ms = ms_since(t);
    double ms_inflate = 0, ms_frame = 0, ms_rows = 0;
    gffx_hip_bam_stage_ms(h, &ms_inflate, &ms_frame, &ms_rows);
    timer("BAM inflate (device)", ms_inflate);
    timer("BAM framing (device)", ms_frame);
    timer("BAM rows (device)", ms_rows);
    timer("BAM chunks in all (staging, device, rows back)", feed_ms);
    t = clock::now();
    std::vector<uint32_t> rows(3 * gffx_hip_bam_rows(h));
    if (gffx_hip_bam_copy_rows(h, rows.data()) != GFFX_OK) throw engine_error();
    timer("BAM rows copy", ms_since(t));
    uint64_t records = 0, unmapped = 0, no_seq = 0, kept = 0;
    gffx_hip_bam_counts(h, &records, &unmapped, &no_seq, &kept);
    if (verbose)
        std::fprintf(stderr, "[INFO] BAM: %zu members, %llu records, %llu unmapped, %llu without a seqid of the index, %llu rows kept\n",
                     n_members, (unsigned long long)records, (unsigned long long)unmapped, (unsigned long long)no_seq,
                     (unsigned long long)kept);
    g_run_stats.count("bam_records", (double)records);
    g_run_stats.count("bam_rows_kept", (double)kept);
    return rows;
}

}  // namespace gffx::bam
