// sam.cpp -- the host side of a SAM source for `gffx depth` / `gffx coverage` (reference: commands/depth.rs:588-591,
// commands/coverage.rs:520-541, which send .sam through the htslib reader they use for .bam).  No htslib here: the file is
// mapped and sniffed by content as htslib does (plain text; BGZF-compressed text; a BAM file under a .sam name goes to
// bam::read_rows), the header's end and its @SQ names are found on the host (device/sam_core.hpp, shared with the device),
// and the text -- or the BGZF members, whose inflated bytes never leave the device -- goes to the engine in chunks
// (gffx_hip_sam_*, device/sam.hip), which finds the lines, reads FLAG, RNAME, POS and CIGAR and hands back the kept
// (seqid number, start, end) rows in file order: what the BED path of both commands takes, unchanged.
// The BGZF front end (directory, EOF marker, header inflate, chunked feed) is bgzf_file.hpp's and the read-back of times, rows
// and tallies source_read.hpp's, both shared with bam.cpp; the sniffing, the header's names and the messages are this file's.
// Every failure message ends in "(read without htslib)".
#include <cstring>

#include "../device/sam_core.hpp"
#include "source_read.hpp"

namespace gffx::sam {

namespace {
const char *const kNoHtslib = " (read without htslib)";

const source::Reader<gffx_hip_sam> kReader = {gffx_hip_sam_stage_ms, gffx_hip_sam_rows, gffx_hip_sam_copy_rows, gffx_hip_sam_counts,
                                              {"SAM inflate (device)", "SAM line scan (device)", "SAM rows (device)",
                                               "SAM chunks in all (staging, device, rows back)", "SAM rows copy"}};
}  // namespace

std::vector<uint32_t> read_rows(const std::string &path, const std::unordered_map<std::string, uint32_t> &seqid_to_num, int device,
                                bool verbose) {
    using source::clock;
    using source::ms_since;
    const source::Timer timer{verbose};
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
            auto offset_error = [&](uint64_t off, int st) {
                return Error(who + ": BGZF block at file offset " + std::to_string(off) + ": " + bgzf::status_name(st) + kNoHtslib);
            };
            uint64_t bad_off = 0;
            if (const int st = bgzf_file::member_directory(p, n, &member_off, &bad_off)) {
                if (st == bgzf::kHeader && bad_off == 0)
                    throw Error(who + " is gzip-compressed but not BGZF (no BC extra field): recompress it with bgzip, or decompress it" + kNoHtslib);
                throw offset_error(bad_off, st);
            }
            bgzf_text = true;
            // the header, inflated on the host (it may span several members; lines may begin in its last one)
            bool first = true, holds_bam = false;
            auto complete = [&](const std::vector<uint8_t> &h) {
                if (first && h.size() >= 4 && std::memcmp(h.data(), "BAM\1", 4) == 0) holds_bam = true;
                first = false;
                return holds_bam ? (int)bgzf::kOk : sam_header_scan(h.data(), h.size(), &header_bytes);
            };
            int hst = bgzf::kTruncated;
            if (const int st = bgzf_file::inflate_header(p, member_off, &head, complete, &hst, &bad_off)) throw offset_error(bad_off, st);
            if (holds_bam) {
                if (verbose) std::fprintf(stderr, "[INFO] \"%s\" holds BAM: read as BAM\n", path.c_str());
                return bam::read_rows(path, seqid_to_num, device, verbose);
            }
            if (hst == bgzf::kTruncated) header_bytes = head.size();  // all header
            head.resize(header_bytes);
            if (!bgzf_file::has_eof_marker(p, n))
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
        const uint64_t chunk = source::chunk_bytes_from_env("GFFX_SAM_CHUNK_BYTES", 0);  // (0: the engine's default)
        Handle<gffx_hip_sam, gffx_hip_sam_destroy> owner;
        auto engine_error = [&]() { return Error(who + ": " + gffx_hip_last_error() + kNoHtslib); };
        const int rc = gffx_hip_sam_create(device, (uint32_t)sq.size(), names.data(), name_off.data(), ref_seq.data(), header_bytes, chunk,
                                           bgzf_text ? 1 : 0, OutPtr(owner));
        if (rc == GFFX_E_INVALID) throw engine_error();  // the header's names: a duplicate @SQ SN, checked before any device call
        if (rc != GFFX_OK) hip_fail("gffx_hip_sam_create");
        gffx_hip_sam *h = owner.get();
        auto feed = [&](const uint8_t *q, uint64_t nb) { return gffx_hip_sam_feed(h, q, nb) == GFFX_OK; };
        if (!(bgzf_text ? bgzf_file::feed_chunks(p, member_off, chunk ? chunk : (64ull << 20), feed) : feed(p, n))) throw engine_error();
        if (gffx_hip_sam_finish(h) != GFFX_OK) throw engine_error();
        uint64_t c[4] = {0, 0, 0, 0};  // lines, unmapped, no_seq, kept
        std::vector<uint32_t> rows = source::take_rows(h, kReader, timer, ms_since(t), c, engine_error);
        if (verbose)
            std::fprintf(stderr, "[INFO] SAM: %s, %llu lines, %llu unmapped, %llu without a seqid of the index, %llu rows kept\n",
                         bgzf_text ? "BGZF text" : "plain text", (unsigned long long)c[0], (unsigned long long)c[1],
                         (unsigned long long)c[2], (unsigned long long)c[3]);
        g_run_stats.count("sam_lines", (double)c[0]);
        g_run_stats.count("sam_rows_kept", (double)c[3]);
        return rows;
    }
}

}  // namespace gffx::sam
