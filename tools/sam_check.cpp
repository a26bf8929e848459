// sam_check.cpp -- the host build of device/sam_core.hpp (the header scan, the rules of one alignment line and the names table
// that k_sam_rows runs) under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc sam_check`), driven by
// tests/test_sam_cpu.py.  Every buffer the core reads is a heap allocation of exactly its size (each line a copy of exactly
// the line), so a read past it is reported.
//   sam_check rows IN [MISSING...]  the lines of a plain SAM file as the device reads them: "header <bytes> <n_sq>", then one line
//                                   per alignment line: "keep <seq> <start> <end> <flag>" or "skip <why> <flag>" (why: unmapped,
//                                   noseq, nointerval); the first malformed line prints "malformed <line number> <reason>" and
//                                   ends the run with exit 3.  seq = the @SQ line's rank, UINT32_MAX for the names MISSING.  The
//                                   text is cut at '\n'; a non-empty rest after the last '\n' is the last line.
//   sam_check header IN             sam_header_scan on every prefix of IN: one line "<length> <status> <header_bytes>" each
//   sam_check lookup NAMES QUERIES  a table of the names in NAMES (one per line, value = rank); per line of QUERIES its value
//                                   or -1; "duplicate <rank>" and exit 3 when NAMES repeats a name
//   sam_check bound N...            "<kMinKeptLine>", then per N "<N> <max_kept_lines(N)>": what sizes k_sam_rows' output
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/sam_core.hpp"

using namespace gffx;
using namespace gffx::sam;

namespace {
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

std::unique_ptr<uint8_t[]> exact(const uint8_t *p, size_t n) {
    std::unique_ptr<uint8_t[]> c(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(c.get(), p, n);
    return c;
}

// a names table on the heap, every part exactly its size
struct Table {
    std::unique_ptr<uint8_t[]> bytes;
    std::unique_ptr<NameEntry[]> slots;
    Names view{nullptr, nullptr, 0};
    long dup = -1;
    Table(const std::vector<std::string> &names, const std::vector<uint32_t> &ref_seq) {
        std::string cat;
        std::vector<uint64_t> off{0};
        for (const std::string &s : names) {
            cat += s;
            off.push_back(cat.size());
        }
        std::vector<NameEntry> t;
        dup = names_build((uint32_t)names.size(), reinterpret_cast<const uint8_t *>(cat.data()), off.data(), ref_seq.data(), &t);
        bytes = exact(reinterpret_cast<const uint8_t *>(cat.data()), cat.size());
        slots.reset(new NameEntry[t.size()]);
        std::memcpy(slots.get(), t.data(), t.size() * sizeof(NameEntry));
        view = Names{slots.get(), bytes.get(), (uint32_t)t.size() - 1};
    }
};

std::vector<std::string> lines_of(const std::vector<uint8_t> &v) {
    std::vector<std::string> out;
    size_t a = 0;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == '\n') {
            out.emplace_back(reinterpret_cast<const char *>(v.data() + a), i - a);
            a = i + 1;
        }
    if (a < v.size()) out.emplace_back(reinterpret_cast<const char *>(v.data() + a), v.size() - a);
    return out;
}
}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rows" && argc >= 3) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        const std::unique_ptr<uint8_t[]> text = exact(in.data(), in.size());
        u64 hb = 0;
        if (sam_header_scan(text.get(), in.size(), &hb) == bgzf::kTruncated) hb = in.size();
        const std::vector<std::string> sq = sq_names(text.get(), hb);
        std::vector<uint32_t> ref_seq(sq.size());
        for (size_t i = 0; i < sq.size(); ++i) {
            ref_seq[i] = (uint32_t)i;
            for (int a = 3; a < argc; ++a)
                if (sq[i] == argv[a]) ref_seq[i] = 0xFFFFFFFFu;
        }
        const Table table(sq, ref_seq);
        if (table.dup >= 0) {
            std::printf("duplicate %ld\n", table.dup);
            return 3;
        }
        std::printf("header %llu %zu\n", hb, sq.size());
        u64 line_no = 0;
        for (u64 i = 0; i < hb; ++i) line_no += in[i] == '\n';
        if (hb == in.size() && hb && in[hb - 1] != '\n') ++line_no;
        // the alignment lines: cut at '\n', the rest after the last one included when it is not empty
        for (u64 a = hb; a < in.size();) {
            u64 e = a;
            while (e < in.size() && in[e] != '\n') ++e;
            ++line_no;
            const std::unique_ptr<uint8_t[]> line = exact(in.data() + a, e - a);
            Row row{};
            const int st = sam_record(line.get(), e - a, table.view, &row);
            if (st == bgzf::kMalformed) {
                std::printf("malformed %llu %s\n", line_no, status_name(row.reason));
                return 3;
            }
            if (st == bgzf::kKeep)
                std::printf("keep %u %u %u %u\n", row.seq, row.start, row.end, row.flag);
            else
                std::printf("skip %s %u\n", row.skip == kUnmapped ? "unmapped" : row.skip == kNoSeq ? "noseq" : "nointerval", row.flag);
            a = e + 1;
        }
        return 0;
    }
    if (mode == "header" && argc == 3) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        for (size_t len = 0; len <= in.size(); ++len) {
            const std::unique_ptr<uint8_t[]> text = exact(in.data(), len);
            u64 hb = 0;
            const int st = sam_header_scan(text.get(), len, &hb);
            std::printf("%zu %d %llu\n", len, st, st == bgzf::kOk ? hb : 0ull);
        }
        return 0;
    }
    if (mode == "lookup" && argc == 4) {
        const std::vector<std::string> names = lines_of(read_file(argv[2])), queries = lines_of(read_file(argv[3]));
        std::vector<uint32_t> ref_seq(names.size());
        for (size_t i = 0; i < names.size(); ++i) ref_seq[i] = (uint32_t)i;
        const Table table(names, ref_seq);
        if (table.dup >= 0) {
            std::printf("duplicate %ld\n", table.dup);
            return 3;
        }
        std::printf("slots %u\n", table.view.mask + 1);
        for (const std::string &q : queries) {
            const std::unique_ptr<uint8_t[]> name = exact(reinterpret_cast<const uint8_t *>(q.data()), q.size());
            uint32_t v = 0;
            if (names_find(table.view, name.get(), (uint32_t)q.size(), &v))
                std::printf("%u\n", v);
            else
                std::printf("-1\n");
        }
        return 0;
    }
    if (mode == "bound") {
        std::printf("%llu\n", kMinKeptLine);
        for (int a = 2; a < argc; ++a) {
            const u64 n = std::strtoull(argv[a], nullptr, 10);
            std::printf("%llu %llu\n", n, max_kept_lines(n));
        }
        return 0;
    }
    std::fprintf(stderr, "usage: sam_check rows IN [MISSING...] | header IN | lookup NAMES QUERIES | bound N...\n");
    return 2;
}
