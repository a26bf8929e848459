// sam.cpp -- the host side of a SAM source for `gffx depth` / `gffx coverage` (reference: commands/depth.rs:588-591,
// commands/coverage.rs:520-541, which send .sam through the htslib reader they use for .bam).  No htslib here: the file is
// mapped and sniffed by content as htslib does (plain text; BGZF-compressed text; a BAM file under a .sam name goes to
// bam::read_rows), the header's end and its @SQ names are found on the host (device/sam_core.hpp, shared with the device),
// and the text -- or the BGZF members, whose inflated bytes never leave the device -- goes to the engine in chunks
// (gffx_hip_sam_*, device/sam.hip), which finds the lines, reads FLAG, RNAME, POS and CIGAR and hands back the kept
// (seqid number, start, end) rows in file order: what the BED path of both commands takes, unchanged.
// Every failure message ends in "(read without htslib)".
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../device/sam_core.hpp"
#include "gffx.hpp"

namespace gffx::sam {

namespace {
const char *const kNoHtslib = " (read without htslib)";
// the 28-byte empty member that ends a BGZF file (SAM spec §4.1.2)
const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

uint64_t chunk_bytes_from_env() {
    const char *e = std::getenv("GFFX_SAM_CHUNK_BYTES");
    if (e && *e) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end && !*end && v > 0) return v;
    }
    return 0;  // the engine's default
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
    const std::string who = "SAM file \"" + path + "\"";
    std::vector<uint64_t> member_off;  // BGZF: member i = [member_off[i], member_off[i + 1])
    std::vector<uint8_t> head;         // BGZF: the inflated text up to the header's end
    u64 header_bytes = 0;  // (sam_core.hpp's type)
    bool bgzf_text = false;
    {
        const MappedFile f = map_file_or(path, "cannot open " + who + kNoHtslib);
        const std::string_view v = f.view();
        const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
        const uint64_t n = v.size();
        if (n == 0) throw Error(who + " is empty" + kNoHtslib);
        auto t = clock::now();
        if (n >= 2 && p[0] == 0x1f && p[1] == 0x8b) {
            // gzip: BGZF members (the BC extra field) or refused
            for (uint64_t at = 0; at < n;) {
                uint32_t total = 0, hdr = 0;
                const int st = bgzf::member_header(p + at, n - at, &total, &hdr);
                if (st == bgzf::kHeader && at == 0)
                    throw Error(who + " is gzip-compressed but not BGZF (no BC extra field): recompress it with bgzip, or decompress it" + kNoHtslib);
                if (st != bgzf::kOk)
                    throw Error(who + ": BGZF block at file offset " + std::to_string(at) + ": " + bgzf::status_name(st) + kNoHtslib);
                member_off.push_back(at);
                at += total;
            }
            member_off.push_back(n);
            bgzf_text = true;
            // the header, inflated on the host (it may span several members; lines may begin in its last one)
            std::unique_ptr<bgzf::Scratch> scratch(new bgzf::Scratch);
            uint32_t crc_table[256];
            for (uint32_t i = 0; i < 256; ++i) crc_table[i] = bgzf::crc_table_entry(i);
            int hst = bgzf::kTruncated;
            for (size_t m = 0; m + 1 < member_off.size() && hst == bgzf::kTruncated; ++m) {
                const size_t at = head.size();
                head.resize(at + bgzf::kMaxIsize);
                uint32_t total = 0, isize = 0;
                const int st = bgzf::member_inflate(p + member_off[m], member_off[m + 1] - member_off[m], head.data() + at, bgzf::kMaxIsize,
                                                    &total, &isize, scratch.get(), crc_table);
                if (st != bgzf::kOk)
                    throw Error(who + ": BGZF block at file offset " + std::to_string(member_off[m]) + ": " + bgzf::status_name(st) + kNoHtslib);
                head.resize(at + isize);
                if (m == 0 && head.size() >= 4 && std::memcmp(head.data(), "BAM\1", 4) == 0) {
                    if (verbose) std::fprintf(stderr, "[INFO] \"%s\" holds BAM: read as BAM\n", path.c_str());
                    return bam::read_rows(path, seqid_to_num, device, verbose);
                }
                hst = sam_header_scan(head.data(), head.size(), &header_bytes);
            }
            if (hst == bgzf::kTruncated) header_bytes = head.size();  // all header
            head.resize(header_bytes);
            if (n < 28 || std::memcmp(p + n - 28, kEof, 28) != 0)
                std::fprintf(stderr, "[WARN] SAM file \"%s\" has no BGZF EOF marker: it may be truncated\n", path.c_str());
        } else {
            if (sam_header_scan(p, n, &header_bytes) == bgzf::kTruncated) header_bytes = n;  // all header
        }
        const uint8_t *hp = bgzf_text ? head.data() : p;
        // tid -> seqid number in @SQ order (depth.rs:320-326); names the index does not know map to UINT32_MAX
        const std::vector<std::string> sq = sq_names(hp, header_bytes);
        if (sq.empty())
            std::fprintf(stderr, "[WARN] SAM file \"%s\" has no @SQ header line: no read has a reference, no row is kept\n", path.c_str());
        std::string names;
        std::vector<uint64_t> name_off{0};
        std::vector<uint32_t> ref_seq;
        for (const std::string &s : sq) {  // (a duplicate name is the engine's to refuse: gffx_hip_sam_create)
            names += s;
            name_off.push_back(names.size());
            const auto it = seqid_to_num.find(s);
            ref_seq.push_back(it == seqid_to_num.end() ? 0xFFFFFFFFu : it->second);
        }
        timer("SAM header", ms_since(t));

        t = clock::now();
        const uint64_t chunk = chunk_bytes_from_env();
        Handle<gffx_hip_sam, gffx_hip_sam_destroy> owner;
        auto engine_error = [&]() { return Error(who + ": " + gffx_hip_last_error() + kNoHtslib); };
        const int rc = gffx_hip_sam_create(device, (uint32_t)sq.size(), names.data(), name_off.data(), ref_seq.data(), header_bytes, chunk,
                                           bgzf_text ? 1 : 0, OutPtr(owner));
        if (rc == GFFX_E_INVALID) throw engine_error();  // the header's names: a duplicate @SQ SN, checked before any device call
        if (rc != GFFX_OK) hip_fail("gffx_hip_sam_create");
        gffx_hip_sam *h = owner.get();
        if (bgzf_text) {
            const uint64_t per = chunk ? chunk : (64ull << 20);
            const size_t n_members = member_off.size() - 1;
            for (size_t m = 0; m < n_members;) {
                size_t e = m + 1;
                while (e < n_members && member_off[e + 1] - member_off[m] <= per) ++e;
                if (gffx_hip_sam_feed(h, p + member_off[m], member_off[e] - member_off[m]) != GFFX_OK) throw engine_error();
                m = e;
            }
        } else if (gffx_hip_sam_feed(h, p, n) != GFFX_OK) {
            throw engine_error();
        }
        if (gffx_hip_sam_finish(h) != GFFX_OK) throw engine_error();
        const double feed_ms = ms_since(t);
        double ms_inflate = 0, ms_lines = 0, ms_rows = 0;
        gffx_hip_sam_stage_ms(h, &ms_inflate, &ms_lines, &ms_rows);
        timer("SAM inflate (device)", ms_inflate);
        timer("SAM line scan (device)", ms_lines);
        timer("SAM rows (device)", ms_rows);
        timer("SAM chunks in all (staging, device, rows back)", feed_ms);
        t = clock::now();
        std::vector<uint32_t> rows(3 * gffx_hip_sam_rows(h));
        if (gffx_hip_sam_copy_rows(h, rows.data()) != GFFX_OK) throw engine_error();
        timer("SAM rows copy", ms_since(t));
        uint64_t lines = 0, unmapped = 0, no_seq = 0, kept = 0;
        gffx_hip_sam_counts(h, &lines, &unmapped, &no_seq, &kept);
        if (verbose)
            std::fprintf(stderr, "[INFO] SAM: %s, %llu lines, %llu unmapped, %llu without a seqid of the index, %llu rows kept\n",
                         bgzf_text ? "BGZF text" : "plain text", (unsigned long long)lines, (unsigned long long)unmapped,
                         (unsigned long long)no_seq, (unsigned long long)kept);
        g_run_stats.count("sam_lines", (double)lines);
        g_run_stats.count("sam_rows_kept", (double)kept);
        return rows;
    }
}

}  // namespace gffx::sam
