// bed_check.cpp -- the host build of device/bed_core.hpp (the rules of one BED line in the two dialects, with the UTF-8 rule of
// gff_core.hpp and the names table of sam_core.hpp that k_bed_rows runs) under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C gffx_amd/csrc bed_check`), driven by tests/test_bed_cpu.py.  Every buffer the core reads is a heap allocation of
// exactly its size (each line a copy of exactly the line), so a read past it is reported.
//   bed_check rows IN DIALECT [NAME...]  DIALECT: intersect | depth.  The names are seqid 0, 1, ...; an argument @FILE stands
//                                        for the lines of FILE (a name longer than an argument may be).  One line out per line
//                                        of IN, as the device cuts them (at '\n'; a non-empty rest after the last one is the
//                                        last line; depth reads a line with its '\n'): "keep <seq> <start> <end>",
//                                        "skip <why>" or "malformed <reason>"; then "tally <lines> <skipped> <no_seq> <kept>
//                                        <malformed>"
//   bed_check lookup NAMES QUERIES       a table of the names in NAMES (one per line, value = rank); "slots <n>", then per line
//                                        of QUERIES its value or -1; "duplicate <rank>" and exit 3 when NAMES repeats a name
//   bed_check utf8 IN                    per line of IN (cut at '\n'): 1 when it is valid UTF-8, else 0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/bed_core.hpp"

using namespace gffx;

namespace {
std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    static uint8_t buf[1 << 16];
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

// a names table on the heap, every part exactly its size; name i has value i
struct Table {
    std::unique_ptr<uint8_t[]> bytes;
    std::unique_ptr<sam::NameEntry[]> slots;
    sam::Names view{nullptr, nullptr, 0};
    long dup = -1;
    explicit Table(const std::vector<std::string> &names) {
        std::string cat;
        std::vector<uint64_t> off{0};
        std::vector<uint32_t> number;
        for (const std::string &s : names) {
            cat += s;
            off.push_back(cat.size());
            number.push_back((uint32_t)number.size());
        }
        std::vector<sam::NameEntry> t;
        dup = sam::names_build((uint32_t)names.size(), reinterpret_cast<const uint8_t *>(cat.data()), off.data(), number.data(), &t);
        bytes = exact(reinterpret_cast<const uint8_t *>(cat.data()), cat.size());
        slots.reset(new sam::NameEntry[t.size()]);
        std::memcpy(slots.get(), t.data(), t.size() * sizeof(sam::NameEntry));
        view = sam::Names{slots.get(), bytes.get(), (uint32_t)t.size() - 1};
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
    if (mode == "rows" && argc >= 4) {
        const std::string d = argv[3];
        if (d != "intersect" && d != "depth") {
            std::fprintf(stderr, "bed_check rows: dialect %s (intersect or depth)\n", argv[3]);
            return 2;
        }
        const int dialect = d == "depth" ? bed::kDepth : bed::kIntersect;
        std::vector<std::string> names;
        for (int a = 4; a < argc; ++a) {
            if (argv[a][0] == '@') {
                for (std::string &s : lines_of(read_file(argv[a] + 1))) names.push_back(std::move(s));
            } else {
                names.emplace_back(argv[a]);
            }
        }
        const Table table(names);
        if (table.dup >= 0) {
            std::printf("duplicate %ld\n", table.dup);
            return 3;
        }
        const std::vector<uint8_t> in = read_file(argv[2]);
        unsigned long long lines = 0, skipped = 0, no_seq = 0, kept = 0, malformed = 0;
        for (size_t a = 0; a < in.size();) {
            size_t e = a;
            while (e < in.size() && in[e] != '\n') ++e;
            const size_t len = e - a + ((dialect == bed::kDepth && e < in.size()) ? 1 : 0);
            const std::unique_ptr<uint8_t[]> line = exact(in.data() + a, len);
            bed::Row row{};
            const int st = bed::bed_record(line.get(), len, dialect, table.view, &row);
            ++lines;
            if (st == bgzf::kMalformed) {
                ++malformed;
                std::printf("malformed %s\n", bed::reason_name(row.reason));
            } else if (st == bgzf::kKeep) {
                ++kept;
                std::printf("keep %u %u %u\n", row.seq, row.start, row.end);
            } else {
                ++(row.skip == bed::kNoSeq ? no_seq : skipped);
                std::printf("skip %s\n", bed::skip_name(row.skip));
            }
            a = e + 1;
        }
        std::printf("tally %llu %llu %llu %llu %llu\n", lines, skipped, no_seq, kept, malformed);
        return 0;
    }
    if (mode == "lookup" && argc == 4) {
        const std::vector<std::string> names = lines_of(read_file(argv[2])), queries = lines_of(read_file(argv[3]));
        const Table table(names);
        if (table.dup >= 0) {
            std::printf("duplicate %ld\n", table.dup);
            return 3;
        }
        std::printf("slots %u\n", table.view.mask + 1);
        for (const std::string &q : queries) {
            const std::unique_ptr<uint8_t[]> name = exact(reinterpret_cast<const uint8_t *>(q.data()), q.size());
            uint32_t v = 0;
            if (sam::names_find(table.view, name.get(), (uint32_t)q.size(), &v))
                std::printf("%u\n", v);
            else
                std::printf("-1\n");
        }
        return 0;
    }
    if (mode == "utf8" && argc == 3) {
        for (const std::string &s : lines_of(read_file(argv[2]))) {
            const std::unique_ptr<uint8_t[]> line = exact(reinterpret_cast<const uint8_t *>(s.data()), s.size());
            std::printf("%d\n", gff::utf8_valid(line.get(), s.size()) ? 1 : 0);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: bed_check rows IN intersect|depth [NAME|@FILE...] | lookup NAMES QUERIES | utf8 IN\n");
    return 2;
}
