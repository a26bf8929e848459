// bgzf_check.cpp -- the host build of device/bgzf_core.hpp (the DEFLATE / BGZF / BAM-record decoder k_bgzf_inflate and
// k_bam_rows run) under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc bgzf_check`), driven by
// tests/test_bgzf_cpu.py.  Every buffer is a heap allocation of exactly its size, so a read or write past it is reported.
//   bgzf_check inflate IN OUT      all members of IN -> OUT; exit 3 + "status <n> <name> offset <file offset>" on a bad member
//   bgzf_check bam IN [K]          the records of a BAM file framed as the device frames them (frame_guess / frame_fix on
//                                  chunks of K members, default all, the unfinished record carried): "header <bytes> <n_ref>",
//                                  then one line per record "<kind> <tid> <start> <end> <flag>" (kind: keep / skip); exit 3
//                                  on a malformed or unfinished record
//   bgzf_check truncate IN         IN's first member cut at every length 0 .. len-1: each must fail with a status
//   bgzf_check fuzz IN N SEED      N random corruptions of IN (byte flips, truncations, spliced bytes), each inflated
//   bgzf_check front IN [LEN [PER]] the file front end of the BAM and SAM sources (host/bgzf_file.hpp) on the first LEN bytes of IN
//                                  (default all): "members <n> eof <0|1>", "header <ok|truncated|bad> <bytes> <n_ref> inflated
//                                  <bytes>" (the BAM header rule), "chunks <calls> bytes <fed>" for runs of PER bytes (default
//                                  1); exit 3 + "status <n> <name> offset <file offset>" on a bad member
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/bgzf_core.hpp"
#include "../gffx_amd/csrc/host/bgzf_file.hpp"

using namespace gffx::bgzf;

namespace {
uint32_t g_crc[256];

std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

// inflates every member of in[0, n) (exactly n bytes on the heap) into out; status of the first bad one, *bad = its offset
int inflate_all(const uint8_t *in, uint64_t n, std::vector<uint8_t> *out, uint64_t *bad) {
    std::unique_ptr<Scratch> s(new Scratch);
    std::unique_ptr<uint8_t[]> blk(new uint8_t[kMaxIsize]);
    for (uint64_t at = 0; at < n;) {
        uint32_t total = 0, isize = 0;
        const int st = member_inflate(in + at, n - at, blk.get(), kMaxIsize, &total, &isize, s.get(), g_crc);
        if (st != kOk) {
            *bad = at;
            return st;
        }
        if (out) out->insert(out->end(), blk.get(), blk.get() + isize);
        at += total;
    }
    return kOk;
}

int heap_inflate(const std::vector<uint8_t> &data, size_t len, uint64_t *bad) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(copy.get(), data.data(), len);
    return inflate_all(copy.get(), len, nullptr, bad);
}
}  // namespace

int main(int argc, char **argv) {
    for (uint32_t i = 0; i < 256; ++i) g_crc[i] = crc_table_entry(i);
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "inflate" && argc == 4) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        std::vector<uint8_t> out;
        uint64_t bad = 0;
        int st = heap_inflate(in, in.size(), &bad);
        if (st == kOk) st = inflate_all(in.data(), in.size(), &out, &bad);
        if (st != kOk) {
            std::printf("status %d %s offset %llu\n", st, status_name(st), (unsigned long long)bad);
            return 3;
        }
        FILE *f = std::fopen(argv[3], "wb");
        if (!f || (out.size() && std::fwrite(out.data(), 1, out.size(), f) != out.size())) return 2;
        std::fclose(f);
        std::printf("ok %zu\n", out.size());
        return 0;
    }
    if (mode == "bam" && (argc == 3 || argc == 4)) {
        // the device's framing (frame_guess on every segment, then frame_fix) on chunks of `per` members, the unfinished
        // record carried from chunk to chunk as segment 0, every buffer a heap allocation of exactly its size
        const std::vector<uint8_t> in = read_file(argv[2]);
        const size_t per = argc == 4 ? (size_t)std::max(1l, std::atol(argv[3])) : (size_t)-1;
        std::vector<uint64_t> moff;
        for (uint64_t at = 0; at < in.size();) {
            uint32_t total = 0, h = 0;
            const int st = member_header(in.data() + at, in.size() - at, &total, &h);
            if (st != kOk) {
                std::printf("status %d %s offset %llu\n", st, status_name(st), (unsigned long long)at);
                return 3;
            }
            moff.push_back(at);
            at += total;
        }
        moff.push_back(in.size());
        const size_t n_members = moff.size() - 1;
        std::unique_ptr<Scratch> scr(new Scratch);
        std::vector<uint8_t> carry, head;
        uint64_t skip = 0;
        uint32_t n_ref = 0;
        bool have_header = false;
        for (size_t m0 = 0; m0 < n_members; m0 += std::min(per, n_members - m0)) {
            const size_t m1 = std::min(n_members, m0 + std::min(per, n_members - m0));
            std::vector<uint8_t> out;
            std::vector<u64> seg{0, carry.size()};  // the carry, then each member's start; the last end is N
            out.insert(out.end(), carry.begin(), carry.end());
            std::unique_ptr<uint8_t[]> blk(new uint8_t[kMaxIsize]);
            for (size_t m = m0; m < m1; ++m) {
                uint32_t total = 0, isize = 0;
                const int st = member_inflate(in.data() + moff[m], moff[m + 1] - moff[m], blk.get(), kMaxIsize, &total, &isize, scr.get(), g_crc);
                if (st != kOk) {
                    std::printf("status %d %s offset %llu\n", st, status_name(st), (unsigned long long)moff[m]);
                    return 3;
                }
                out.insert(out.end(), blk.get(), blk.get() + isize);
                seg.push_back(out.size());
            }
            if (!have_header) {
                head.insert(head.end(), out.begin(), out.end());
                uint64_t hb = 0;
                const int st = bam_header_size(head.data(), head.size(), &hb, &n_ref);
                if (st == kTruncated) {
                    skip += out.size();
                    continue;
                }
                if (st != kOk) {
                    std::printf("header status %d\n", st);
                    return 3;
                }
                std::printf("header %llu %u\n", (unsigned long long)hb, n_ref);
                have_header = true;
                skip = hb - skip;  // header bytes in this chunk
            }
            const u64 N = out.size();
            const uint32_t n_seg = (uint32_t)(seg.size() - 1);
            std::unique_ptr<uint8_t[]> D(new uint8_t[N ? N : 1]);
            if (N) std::memcpy(D.get(), out.data(), N);
            std::unique_ptr<u64[]> ge(new u64[n_seg]), entry(new u64[n_seg]), sg(new u64[n_seg + 1]);
            std::unique_ptr<uint32_t[]> gn(new uint32_t[n_seg]), cnt(new uint32_t[n_seg]);
            std::memcpy(sg.get(), seg.data(), (n_seg + 1) * sizeof(u64));
            for (uint32_t s = 0; s < n_seg; ++s) frame_guess(D.get(), N, sg[s], sg[s + 1], &ge[s], &gn[s]);
            const u64 start = std::min<u64>(skip, N);
            skip -= start;
            u64 tail = N, err = 0;
            if (frame_fix(D.get(), N, sg.get(), n_seg, start, ge.get(), gn.get(), entry.get(), cnt.get(), &tail, &err) != kOk) {
                std::printf("malformed record at chunk offset %llu\n", (unsigned long long)err);
                return 3;
            }
            for (uint32_t s = 0; s < n_seg; ++s) {
                u64 p = entry[s];
                for (uint32_t c = 0; c < cnt[s]; ++c) {  // (as k_frame_list, then k_bam_rows on a copy of exactly the record)
                    const uint32_t bs = le32(D.get() + p);
                    std::unique_ptr<uint8_t[]> rec(new uint8_t[4 + (size_t)bs]);
                    std::memcpy(rec.get(), D.get() + p, 4 + (size_t)bs);
                    Row row{0, 0, 0, 0};
                    const int st = bam_record(rec.get(), n_ref, &row);
                    if (st == kMalformed) {
                        std::printf("malformed record at chunk offset %llu\n", (unsigned long long)p);
                        return 3;
                    }
                    std::printf("%s %d %u %u %u\n", st == kKeep ? "keep" : "skip", row.tid, row.start, row.end, row.flag);
                    p += 4 + (u64)bs;
                }
            }
            carry.assign(out.begin() + (long)tail, out.end());
        }
        if (!have_header) {
            std::printf("ends inside the header\n");
            return 3;
        }
        if (!carry.empty()) {
            std::printf("unfinished record (%zu bytes)\n", carry.size());
            return 3;
        }
        return 0;
    }
    if (mode == "truncate" && argc == 3) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        uint32_t total = 0, h = 0;
        if (member_header(in.data(), in.size(), &total, &h) != kOk) return 2;
        size_t rejected = 0;
        for (size_t len = 0; len < total; ++len) {
            uint64_t bad = 0;
            if (heap_inflate(in, len, &bad) == kOk && len > 0) {
                std::printf("accepted a member cut at %zu of %u bytes\n", len, total);
                return 4;
            }
            ++rejected;
        }
        std::printf("ok %zu\n", rejected);
        return 0;
    }
    if (mode == "fuzz" && argc == 5) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        const long iters = std::atol(argv[3]);
        std::mt19937_64 rng(std::strtoull(argv[4], nullptr, 10));
        long hist[16] = {0};
        for (long it = 0; it < iters; ++it) {
            std::vector<uint8_t> v = in;
            const int kind = (int)(rng() % 4);
            if (kind == 0 || v.empty()) {
                for (int k = 1 + (int)(rng() % 4); k && !v.empty(); --k) v[rng() % v.size()] ^= (uint8_t)(1u << (rng() % 8));
            } else if (kind == 1) {
                v.resize(rng() % v.size());
            } else if (kind == 2) {
                const size_t at = rng() % v.size();
                for (int k = 0; k < 16; ++k) v.insert(v.begin() + (long)at, (uint8_t)rng());
            } else {
                const size_t at = 18 + rng() % (v.size() > 26 ? v.size() - 26 : 1);  // inside the DEFLATE data
                for (size_t k = 0; k < 8 && at + k < v.size(); ++k) v[at + k] = (uint8_t)rng();
            }
            uint64_t bad = 0;
            hist[heap_inflate(v, v.size(), &bad) & 15]++;
        }
        std::printf("ok");
        for (int k = 0; k < 16; ++k)
            if (hist[k]) std::printf(" %d:%ld", k, hist[k]);
        std::printf("\n");
        return 0;
    }
    if (mode == "front" && argc >= 3 && argc <= 5) {
        namespace bf = gffx::bgzf_file;
        const std::vector<uint8_t> in = read_file(argv[2]);
        const size_t len = argc > 3 ? std::min<size_t>(in.size(), std::strtoull(argv[3], nullptr, 10)) : in.size();
        const uint64_t per = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 1;
        std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);  // exactly the bytes: a read past them is reported
        if (len) std::memcpy(copy.get(), in.data(), len);
        const uint8_t *p = copy.get();
        std::vector<uint64_t> off;
        uint64_t bad = 0;
        int st = bf::member_directory(p, len, &off, &bad);
        if (st != kOk) {
            std::printf("status %d %s offset %llu\n", st, status_name(st), (unsigned long long)bad);
            return 3;
        }
        std::printf("members %zu eof %d\n", off.size() - 1, bf::has_eof_marker(p, len) ? 1 : 0);
        std::vector<uint8_t> head;
        uint64_t hb = 0;
        uint32_t n_ref = 0;
        int hst = kTruncated;
        st = bf::inflate_header(p, off, &head, [&](const std::vector<uint8_t> &h) { return bam_header_size(h.data(), h.size(), &hb, &n_ref); },
                                &hst, &bad);
        if (st != kOk) {
            std::printf("status %d %s offset %llu\n", st, status_name(st), (unsigned long long)bad);
            return 3;
        }
        std::printf("header %s %llu %u inflated %zu\n", hst == kOk ? "ok" : hst == kTruncated ? "truncated" : "bad",
                    (unsigned long long)(hst == kOk ? hb : 0), hst == kOk ? n_ref : 0, head.size());
        uint64_t calls = 0, fed = 0, next = 0;
        const bool all = bf::feed_chunks(p, off, per, [&](const uint8_t *q, uint64_t nb) {
            if (q != p + next || nb == 0) return false;  // runs are adjacent, in order, never empty
            next += nb;
            ++calls;
            fed += nb;
            return true;
        });
        if (!all || fed != len) {
            std::printf("chunks do not tile the file (%llu of %zu bytes)\n", (unsigned long long)fed, len);
            return 4;
        }
        std::printf("chunks %llu bytes %llu\n", (unsigned long long)calls, (unsigned long long)fed);
        return 0;
    }
    std::fprintf(stderr, "usage: bgzf_check inflate IN OUT | bam IN [K] | truncate IN | fuzz IN N SEED | front IN [LEN [PER]]\n");
    return 2;
}
