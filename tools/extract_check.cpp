// extract_check.cpp -- the host build of device/ids_core.hpp (the ID table's hash, compare and lookup, the bounded parent chase,
// the slices of a GFF line and the keep test that the kernels of device/ids.hip run) under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc extract_check`), driven by tests/test_extract_cpu.py.  Every buffer the
// core reads is a heap allocation of exactly its size (each query and each line a copy of exactly its bytes), so a read past
// it is reported.  The table is built on the host, in order, with the device's hash and probing (ids::table_build_host).
//   extract_check lookup NAMES QUERIES [HASH_BITS]   NAMES: one name per line, fid = line number.  "slots <n>", then per line of
//                                                    QUERIES the fid of the LAST equal name, or -1
//   extract_check chase PRT FIDS                     PRT: one parent per line (decimal), FIDS: one fid per line.  Per fid
//                                                    "<root> <steps bound>", root -1 when invalid (out of range, or no root
//                                                    within n steps)
//   extract_check filter TEXT NAMES PRT QUERIES ROOT [-T TYPES]
//                                                    the lines of TEXT (cut behind every '\n'; a non-empty rest is the last
//                                                    line) as lines of the block of root fid ROOT, the names of QUERIES
//                                                    requested, TYPES the raw -T string: per line "1" (kept) or "0"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/ids_core.hpp"
#include "../gffx_amd/csrc/host/text.hpp"

using namespace gffx;
using namespace gffx::ids;

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

// the lines of v without their '\n' (a non-empty rest after the last '\n' is a line)
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

std::vector<uint32_t> numbers_of(const std::vector<uint8_t> &v) {
    std::vector<uint32_t> out;
    for (const std::string &s : lines_of(v))
        if (!s.empty()) out.push_back((uint32_t)std::strtoull(s.c_str(), nullptr, 10));
    return out;
}

// an ID table on the heap, every part exactly its size
struct HostTable {
    std::unique_ptr<uint8_t[]> bytes;
    std::unique_ptr<u64[]> off, slot;
    std::unique_ptr<uint32_t[]> val;
    Table view{nullptr, nullptr, nullptr, nullptr, 0, 0};
    HostTable(const std::vector<std::string> &names, int hash_bits) {
        std::string cat;
        std::vector<u64> o{0};
        for (const std::string &s : names) {
            cat += s;
            o.push_back(cat.size());
        }
        std::vector<u64> sl;
        std::vector<uint32_t> va;
        bytes = exact(reinterpret_cast<const uint8_t *>(cat.data()), cat.size());
        off = exact(o.data(), o.size());
        table_build_host(names.size(), bytes.get(), off.get(), hash_bits, &sl, &va);
        slot = exact(sl.data(), sl.size());
        val = exact(va.data(), va.size());
        view = Table{slot.get(), val.get(), bytes.get(), off.get(), (uint32_t)sl.size() - 1, hash_mask_of(hash_bits)};
    }
    uint32_t find(const std::string &q) const {
        const std::unique_ptr<uint8_t[]> name = exact(reinterpret_cast<const uint8_t *>(q.data()), q.size());
        return table_find(view, name.get(), q.size());
    }
};
}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "lookup" && (argc == 4 || argc == 5)) {
        const std::vector<std::string> names = lines_of(read_file(argv[2])), queries = lines_of(read_file(argv[3]));
        const HostTable t(names, argc == 5 ? std::atoi(argv[4]) : 32);
        std::printf("slots %u\n", t.view.mask + 1);
        for (const std::string &q : queries) {
            const uint32_t f = t.find(q);
            if (f == kNone)
                std::printf("-1\n");
            else
                std::printf("%u\n", f);
        }
        return 0;
    }
    if (mode == "chase" && argc == 4) {
        const std::vector<uint32_t> prt_v = numbers_of(read_file(argv[2])), fids = numbers_of(read_file(argv[3]));
        const std::unique_ptr<uint32_t[]> prt = exact(prt_v.data(), prt_v.size());
        for (uint32_t f : fids) {
            const uint32_t r = chase_root(prt.get(), (uint32_t)prt_v.size(), f);
            if (r == kNone)
                std::printf("-1 %zu\n", prt_v.size());
            else
                std::printf("%u %zu\n", r, prt_v.size());
        }
        return 0;
    }
    if (mode == "filter" && (argc == 7 || (argc == 9 && std::string(argv[7]) == "-T"))) {
        const std::vector<uint8_t> text = read_file(argv[2]);
        const std::vector<std::string> names = lines_of(read_file(argv[3])), queries = lines_of(read_file(argv[5]));
        const std::vector<uint32_t> prt_v = numbers_of(read_file(argv[4]));
        const uint32_t root = (uint32_t)std::strtoull(argv[6], nullptr, 10);
        const HostTable t(names, 32);
        const std::unique_ptr<uint32_t[]> prt = exact(prt_v.data(), prt_v.size());
        const uint32_t n = (uint32_t)names.size(), n_prt = (uint32_t)prt_v.size();
        // what k_ids_resolve and k_ids_roots leave in the handle
        std::vector<uint32_t> req_v((std::max(n, n_prt) + 31) / 32 + 1, 0), fr_v(n ? n : 1, kNone);
        for (const std::string &q : queries) {
            const uint32_t f = t.find(q);
            if (f != kNone) req_v[f >> 5] |= 1u << (f & 31);
        }
        for (uint32_t f = 0; f < n; ++f) fr_v[f] = chase_root(prt.get(), n_prt, f);
        const std::unique_ptr<uint32_t[]> requested = exact(req_v.data(), req_v.size()), fid_root = exact(fr_v.data(), fr_v.size());
        std::string tcat;
        std::vector<uint32_t> toff_v{0};
        const bool by_type = argc == 9;
        if (by_type)
            for (const std::string &ty : split_types(std::optional<std::string>(argv[8]))) {
                tcat += ty;
                toff_v.push_back((uint32_t)tcat.size());
            }
        const std::unique_ptr<uint8_t[]> tbytes = exact(reinterpret_cast<const uint8_t *>(tcat.data()), tcat.size());
        const std::unique_ptr<uint32_t[]> toff = exact(toff_v.data(), toff_v.size());
        const Types types{tbytes.get(), toff.get(), (uint32_t)toff_v.size() - 1, by_type ? 1 : 0};
        const uint8_t key[2] = {'I', 'D'};
        for (size_t a = 0; a < text.size();) {
            size_t e = a;
            while (e < text.size() && text[e] != '\n') ++e;
            if (e < text.size()) ++e;  // with its '\n'
            const std::unique_ptr<uint8_t[]> line = exact(text.data() + a, e - a);
            std::printf("%d\n", keep_line(t.view, requested.get(), fid_root.get(), types, key, 2, line.get(), e - a, root) ? 1 : 0);
            a = e;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: extract_check lookup NAMES QUERIES [HASH_BITS] | chase PRT FIDS | filter TEXT NAMES PRT QUERIES ROOT [-T TYPES]\n");
    return 2;
}
