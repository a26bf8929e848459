// pileup_check.cpp -- the host build of device/pileup_core.hpp (the searches, B(x) and a segment's bases, as
// k_pileup_segments runs them) under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc pileup_check`),
// driven by tests/test_pileup_cpu.py.  The sorted keys, their prefix sums and the offsets are restated here on the host
// (std::sort, one running sum); every array the core reads is a heap allocation of exactly its size, so a read past it is
// reported.
//   pileup_check IN     IN holds one case: a line "n_seq N", then lines "row SEQ START END" and "seg SEQ START END" in any
//                       order.  One line out per seg line, in their order: "bases <total>"; then "rows <n> segs <n>".
//                       A row with SEQ >= N or START >= END, or a seg with SEQ >= N: "refused <what>" and exit 3.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../gffx_amd/csrc/device/pileup_core.hpp"

using namespace gffx;
using pileup::u64;

namespace {

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    std::unique_ptr<T[]> c(new T[v.size()]);  // (a zero-length allocation for an empty array: any read of it is reported)
    if (!v.empty()) std::memcpy(c.get(), v.data(), v.size() * sizeof(T));
    return c;
}

struct Triple {
    uint32_t seq, start, end;
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: pileup_check IN\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint64_t n_seq = 0;
    std::vector<Triple> rows, segs;
    char word[16];
    uint64_t a = 0, b = 0, c = 0;
    while (std::fscanf(f, "%15s", word) == 1) {
        if (!std::strcmp(word, "n_seq")) {
            if (std::fscanf(f, "%" SCNu64, &n_seq) != 1) return 2;
            continue;
        }
        if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) != 3 || a > 0xFFFFFFFFull || b > 0xFFFFFFFFull || c > 0xFFFFFFFFull) return 2;
        const Triple t{(uint32_t)a, (uint32_t)b, (uint32_t)c};
        if (!std::strcmp(word, "row"))
            rows.push_back(t);
        else if (!std::strcmp(word, "seg"))
            segs.push_back(t);
        else
            return 2;
    }
    std::fclose(f);
    for (const Triple &r : rows) {
        if (r.seq >= n_seq) return std::printf("refused row chr\n"), 3;
        if (r.start >= r.end) return std::printf("refused row interval\n"), 3;
    }
    for (const Triple &s : segs)
        if (s.seq >= n_seq) return std::printf("refused seg chr\n"), 3;
    // what one fold builds on the device: the two key arrays sorted by (seqid, coordinate), each on its own; n + 1 prefix
    // sums of the coordinates; off[c] = the keys with seqid < c
    const size_t n = rows.size();
    std::vector<std::pair<uint32_t, uint32_t>> ks(n), ke(n);
    for (size_t i = 0; i < n; ++i) ks[i] = {rows[i].seq, rows[i].start}, ke[i] = {rows[i].seq, rows[i].end};
    std::sort(ks.begin(), ks.end());
    std::sort(ke.begin(), ke.end());
    std::vector<uint32_t> co_s(n), co_e(n);
    std::vector<u64> pre_s(n + 1, 0), pre_e(n + 1, 0), off(n_seq + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        co_s[i] = ks[i].second, co_e[i] = ke[i].second;
        pre_s[i + 1] = pre_s[i] + co_s[i], pre_e[i + 1] = pre_e[i] + co_e[i];
        off[ks[i].first + 1]++;
    }
    for (uint64_t q = 0; q < n_seq; ++q) off[q + 1] += off[q];
    const auto x_s = exact(co_s), x_e = exact(co_e);
    const auto x_ps = exact(pre_s), x_pe = exact(pre_e), x_off = exact(off);
    const pileup::Keys K{x_s.get(), x_e.get(), x_ps.get(), x_pe.get()};
    for (const Triple &s : segs)
        std::printf("bases %llu\n", pileup::segment_bases(K, x_off[s.seq], x_off[s.seq + 1], s.start, s.end));
    std::printf("rows %zu segs %zu\n", rows.size(), segs.size());
    return 0;
}
