// gff_check.cpp -- the host build of device/gff_core.hpp (the rules of one GFF3 line that k_gff_rows of device/gff.hip runs) under
// AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc gff_check`), driven by tests/test_index_device_cpu.py.
// Every line is a heap copy of exactly its bytes (the key and the skip strings too), so a read past it is reported.
//   gff_check lines TEXT KEY SKIP             the lines of TEXT (cut at every '\n'; a non-empty rest is the last line), KEY the
//                                             attribute key, SKIP the raw --skip-types string.  Per line its status name, and
//                                               row <start> <end> <warn> <seq> <id> <parent|-> <value|->     (strings in hex)
//                                               skipped_type <type in hex>
//   gff_check build TEXT KEY SKIP [HASH_BITS] the finish steps of gff.hip restated on the host in order -- the ID table via
//                                             ids::table_build_host and ids::table_find, the parents, the numbers by first
//                                             appearance via gff::first_rows_host -- over the rows of TEXT:
//                                               error <file offset of the line> <KIND>            (the first bad line; nothing else)
//                                             or
//                                               counts <lines> <blank> <skipped_type> <zero_end> <rows> <roots> <seqids> <values>
//                                               row <id in hex> <fid> <prt> <a2f|-1>               per row
//                                               seqid <hex> / value <hex>                          in number order
//                                               gof <fid> <seq> <start offset> <end offset>        per root
//                                               root <start> <end> <fid> <seq>                     per root
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/gff_core.hpp"

using namespace gffx;
using gffx::gff::u64;

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

template <typename T>
std::unique_ptr<T[]> exact(const T *p, size_t n) {
    std::unique_ptr<T[]> c(new T[n ? n : 1]);
    if (n) std::memcpy(c.get(), p, n * sizeof(T));
    return c;
}

std::string hex(const uint8_t *p, u64 n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (u64 i = 0; i < n; ++i) {
        s.push_back(d[p[i] >> 4]);
        s.push_back(d[p[i] & 15]);
    }
    return s.empty() ? "." : s;  // "." = the empty string
}

struct Params {  // the key and the skip list, every part exactly its size
    std::unique_ptr<uint8_t[]> key, skip_bytes;
    std::unique_ptr<uint32_t[]> skip_off;
    uint32_t key_len;
    gff::SkipList skip;
    Params(const char *key_s, const char *skip_s) {
        key_len = (uint32_t)std::strlen(key_s);
        key = exact(reinterpret_cast<const uint8_t *>(key_s), key_len);
        std::string cat;
        std::vector<uint32_t> off{0};
        const std::string raw = skip_s;
        size_t a = 0;
        while (true) {  // split(',') without trimming; an empty string is a member
            const size_t c = raw.find(',', a);
            cat += raw.substr(a, c == std::string::npos ? std::string::npos : c - a);
            off.push_back((uint32_t)cat.size());
            if (c == std::string::npos) break;
            a = c + 1;
        }
        skip_bytes = exact(reinterpret_cast<const uint8_t *>(cat.data()), cat.size());
        skip_off = exact(off.data(), off.size());
        skip = gff::SkipList{skip_bytes.get(), skip_off.get(), (uint32_t)off.size() - 1};
    }
};

struct Line {
    u64 off, len;
};
std::vector<Line> lines_of(const std::vector<uint8_t> &v) {
    std::vector<Line> out;
    u64 a = 0;
    for (u64 i = 0; i < v.size(); ++i)
        if (v[i] == '\n') {
            out.push_back({a, i - a});
            a = i + 1;
        }
    if (a < v.size()) out.push_back({a, v.size() - a});
    return out;
}
}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "lines" && argc == 5) {
        const std::vector<uint8_t> text = read_file(argv[2]);
        const Params P(argv[3], argv[4]);
        for (const Line &l : lines_of(text)) {
            const std::unique_ptr<uint8_t[]> line = exact(text.data() + l.off, l.len);
            gff::Rec r{};
            const int st = gff::gff_record(line.get(), l.len, P.key.get(), P.key_len, P.skip, &r);
            const uint8_t *p = line.get();
            if (st == gff::kRow)
                std::printf("row %u %u %u %s %s %s %s\n", r.start, r.end, r.warn, hex(p + r.seq_a, r.seq_z - r.seq_a).c_str(),
                            hex(p + r.id_a, r.id_z - r.id_a).c_str(), r.par_z > r.par_a ? hex(p + r.par_a, r.par_z - r.par_a).c_str() : "-",
                            r.attr_z > r.attr_a ? hex(p + r.attr_a, r.attr_z - r.attr_a).c_str() : "-");
            else if (st == gff::kSkipType)
                std::printf("skipped_type %s\n", hex(p + r.type_a, r.type_z - r.type_a).c_str());
            else
                std::printf("%s\n", gff::status_name(st));
        }
        return 0;
    }
    if (mode == "build" && (argc == 5 || argc == 6)) {
        const std::vector<uint8_t> text = read_file(argv[2]);
        const Params P(argv[3], argv[4]);
        const int hash_bits = argc == 6 ? std::atoi(argv[5]) : -1;
        // the rows, as the passes of gff.hip append them
        std::vector<u64> line_off;
        std::vector<uint32_t> start, end;
        std::string cat[4];
        std::vector<u64> off[4];
        for (auto &o : off) o.push_back(0);
        u64 n_lines = 0, blank = 0, skipped = 0, zero_end = 0;
        for (const Line &l : lines_of(text)) {
            ++n_lines;
            const std::unique_ptr<uint8_t[]> line = exact(text.data() + l.off, l.len);
            gff::Rec r{};
            const int st = gff::gff_record(line.get(), l.len, P.key.get(), P.key_len, P.skip, &r);
            if (st >= gff::kFirstError) {
                std::printf("error %llu %s\n", l.off, gff::status_name(st));
                return 0;
            }
            if (st == gff::kBlank) ++blank;
            if (st == gff::kSkipType) ++skipped;
            if (st == gff::kZeroEnd) ++zero_end;
            if (st != gff::kRow) continue;
            line_off.push_back(l.off);
            start.push_back(r.start);
            end.push_back(r.end);
            const u64 a[4] = {r.seq_a, r.id_a, r.par_a, r.attr_a}, z[4] = {r.seq_z, r.id_z, r.par_z, r.attr_z};
            for (int k = 0; k < 4; ++k) {
                cat[k].append(reinterpret_cast<const char *>(line.get()) + a[k], z[k] - a[k]);
                off[k].push_back(cat[k].size());
            }
        }
        const u64 n = line_off.size();
        std::unique_ptr<uint8_t[]> bytes[4];
        std::unique_ptr<u64[]> offs[4];
        for (int k = 0; k < 4; ++k) {
            bytes[k] = exact(reinterpret_cast<const uint8_t *>(cat[k].data()), cat[k].size());
            offs[k] = exact(off[k].data(), off[k].size());
        }
        // 1. the ID table, 2. the parents
        std::vector<u64> slot_v;
        std::vector<uint32_t> val_v;
        ids::table_build_host(n, bytes[1].get(), offs[1].get(), hash_bits, &slot_v, &val_v);
        const std::unique_ptr<u64[]> slot = exact(slot_v.data(), slot_v.size());
        const std::unique_ptr<uint32_t[]> val = exact(val_v.data(), val_v.size());
        const ids::Table t{slot.get(), val.get(), bytes[1].get(), offs[1].get(), (uint32_t)slot_v.size() - 1, ids::hash_mask_of(hash_bits)};
        std::vector<uint32_t> fid(n), prt(n);
        std::vector<uint8_t> root(n), has_attr(n);
        for (u64 r = 0; r < n; ++r) {
            fid[r] = ids::table_find(t, bytes[1].get() + offs[1][r], offs[1][r + 1] - offs[1][r]);
            prt[r] = fid[r];
            const u64 pn = offs[2][r + 1] - offs[2][r];
            if (pn) {
                const std::unique_ptr<uint8_t[]> q = exact(bytes[2].get() + offs[2][r], pn);
                const uint32_t f = ids::table_find(t, q.get(), pn);
                if (f != ids::kNone) prt[r] = f;
            }
            root[r] = prt[r] == fid[r];
            has_attr[r] = offs[3][r + 1] > offs[3][r];
        }
        // 3. the numbers by first appearance: the count of first rows before a string's first row
        auto number = [&](int k, const std::vector<uint8_t> &eligible, std::vector<uint32_t> *num, std::vector<std::string> *names) {
            std::vector<uint32_t> first;
            gff::first_rows_host(n, bytes[k].get(), offs[k].get(), eligible.data(), hash_bits, &first);
            std::vector<uint32_t> rank(n + 1, 0);
            for (u64 r = 0; r < n; ++r) {
                rank[r + 1] = rank[r] + (first[r] == r ? 1u : 0u);
                if (first[r] == r) names->push_back(hex(bytes[k].get() + offs[k][r], offs[k][r + 1] - offs[k][r]));
            }
            num->assign(n, ids::kNone);
            for (u64 r = 0; r < n; ++r)
                if (first[r] != ids::kNone) (*num)[r] = rank[first[r]];
        };
        std::vector<uint32_t> seq, a2f;
        std::vector<std::string> seq_names, attr_names;
        number(0, root, &seq, &seq_names);
        number(3, has_attr, &a2f, &attr_names);
        // 4. the root list
        std::vector<uint32_t> roots;
        for (u64 r = 0; r < n; ++r)
            if (root[r]) roots.push_back((uint32_t)r);
        std::printf("counts %llu %llu %llu %llu %llu %zu %zu %zu\n", n_lines, blank, skipped, zero_end, n, roots.size(), seq_names.size(),
                    attr_names.size());
        for (u64 r = 0; r < n; ++r)
            std::printf("row %s %u %u %lld\n", hex(bytes[1].get() + offs[1][r], offs[1][r + 1] - offs[1][r]).c_str(), fid[r], prt[r],
                        a2f[r] == ids::kNone ? -1ll : (long long)a2f[r]);
        for (const std::string &s : seq_names) std::printf("seqid %s\n", s.c_str());
        for (const std::string &s : attr_names) std::printf("value %s\n", s.c_str());
        for (size_t k = 0; k < roots.size(); ++k) {
            const uint32_t r = roots[k];
            std::printf("gof %u %u %llu %llu\n", fid[r], seq[r], line_off[r], k + 1 < roots.size() ? line_off[roots[k + 1]] : (u64)text.size());
        }
        for (const uint32_t r : roots) std::printf("root %u %u %u %u\n", start[r], end[r], fid[r], seq[r]);
        return 0;
    }
    std::fprintf(stderr, "usage: gff_check lines TEXT KEY SKIP | build TEXT KEY SKIP [HASH_BITS]\n");
    return 2;
}
