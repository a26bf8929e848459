// bgzf_file.hpp -- the front end of a mapped BGZF file that the BAM and the SAM source share (bam.cpp, sam.cpp): its member
// directory, the EOF-marker test, the header inflated on the host with the decoder the device uses, and the walk over the
// members in chunks.  Nothing here throws or prints: a bad member comes back as its bgzf::Status and file offset, and the
// callers word their own messages.  Depends on device/bgzf_core.hpp alone, so tools/bgzf_check.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../device/bgzf_core.hpp"

namespace gffx::bgzf_file {

// the 28-byte empty member that ends a BGZF file (SAM spec §4.1.2)
inline constexpr uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

inline bool has_eof_marker(const uint8_t *p, uint64_t n) { return n >= 28 && std::memcmp(p + n - 28, kEof, 28) == 0; }

// The block directory of p[0, n): every member's header checked, lengths by hopping BSIZE; member i = [off[i], off[i + 1]).
// Returns bgzf::kOk, or the status of the first bad member and *bad_off = its file offset (off then holds the members before it).
inline int member_directory(const uint8_t *p, uint64_t n, std::vector<uint64_t> *off, uint64_t *bad_off) {
    for (uint64_t at = 0; at < n;) {
        uint32_t total = 0, hdr = 0;
        const int st = bgzf::member_header(p + at, n - at, &total, &hdr);
        if (st != bgzf::kOk) {
            *bad_off = at;
            return st;
        }
        off->push_back(at);
        at += total;
    }
    off->push_back(n);
    return bgzf::kOk;
}

// Inflates members from the front, appending to head, until done(head) -- asked after every member -- no longer answers
// bgzf::kTruncated (the header is complete, or is none) or the members run out.  Returns bgzf::kOk and *header_status =
// done's last answer (kTruncated: the file ends inside its header), or the status of the member that failed to inflate
// and *bad_off = its file offset.
template <class Done>
int inflate_header(const uint8_t *p, const std::vector<uint64_t> &off, std::vector<uint8_t> *head, Done &&done, int *header_status,
                   uint64_t *bad_off) {
    std::unique_ptr<bgzf::Scratch> scratch(new bgzf::Scratch);
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; ++i) crc_table[i] = bgzf::crc_table_entry(i);
    *header_status = bgzf::kTruncated;
    for (size_t m = 0; m + 1 < off.size() && *header_status == bgzf::kTruncated; ++m) {
        const size_t at = head->size();
        head->resize(at + bgzf::kMaxIsize);
        uint32_t total = 0, isize = 0;
        const int st = bgzf::member_inflate(p + off[m], off[m + 1] - off[m], head->data() + at, bgzf::kMaxIsize, &total, &isize,
                                            scratch.get(), crc_table);
        if (st != bgzf::kOk) {
            head->resize(at);
            *bad_off = off[m];
            return st;
        }
        head->resize(at + isize);
        *header_status = done(*head);
    }
    return bgzf::kOk;
}

// The members in runs of about `per` bytes (whole members, at least one): feed(first byte, length) for each run in order,
// until one answers false.  Returns whether all did.
template <class Feed>
bool feed_chunks(const uint8_t *p, const std::vector<uint64_t> &off, uint64_t per, Feed &&feed) {
    const size_t n_members = off.size() - 1;
    for (size_t m = 0; m < n_members;) {
        size_t e = m + 1;
        while (e < n_members && off[e + 1] - off[m] <= per) ++e;
        if (!feed(p + off[m], off[e] - off[m])) return false;
        m = e;
    }
    return true;
}

}  // namespace gffx::bgzf_file
