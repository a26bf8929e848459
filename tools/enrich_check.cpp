// enrich_check.cpp -- the host build of device/enrich_core.hpp (mix64, the permutation key and draw, the placement rule and a
// region in a row of the totals, as k_classmap_permute of enrich.hip runs them) under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc enrich_check`), driven by tests/test_enrich_cpu.py.  The class map comes in
// finished -- its points and running sums, as tools/classmap_check.cpp prints them --; every array the core reads is a heap
// allocation of exactly its size, so a read past it is reported.
//   enrich_check [--time] IN   IN: "n_seq N" and "layers T" first, then in any order "perms N", "seed S", "first_row F",
//                       "len SEQ L", "p SEQ POS CLASS" (the points, in their order), "cb I V0 .. V(T-1)" (point I's sums) and
//                       "q SEQ START END" (the regions, in their order; region j is global row F + j).
//                       Out: "mix A B C" (mix64(GOLD * n), n = 1, 2, 3, in hex), "B p V0 .. VT" and "R p V0 .. VT" per row
//                       p = 0 .. N, "unplaced U", "regions <n> perms <N>".  A region with SEQ >= N: "range", exit 3.  Totals
//                       that break their invariants (a row's regions not adding up to the region count, its bases not to
//                       the width of the non-empty regions): "inconsistent totals", exit 4.
//                       --time (the -O2 build `enrich_host_baseline`, tools/enrich_bench.py): no matrices but
//                       "regions <n> perms <N> ms <the placement loop, one core> checksum <c>".
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../gffx_amd/csrc/device/enrich_core.hpp"

using namespace gffx;
using enrich::u64;

namespace {

template <typename X>
std::unique_ptr<X[]> exact(const std::vector<X> &v) {
    std::unique_ptr<X[]> c(new X[v.size()]);  // (a zero-length allocation for an empty array: any read of it is reported)
    if (!v.empty()) std::memcpy(c.get(), v.data(), v.size() * sizeof(X));
    return c;
}

struct Query {
    uint32_t seq, start, end;
};

}  // namespace

int main(int argc, char **argv) {
    const bool timed = argc == 3 && !std::strcmp(argv[1], "--time");
    if (argc != 2 && !timed) {
        std::fprintf(stderr, "usage: enrich_check [--time] IN\n");
        return 2;
    }
    FILE *f = std::fopen(argv[argc - 1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[argc - 1]);
        return 2;
    }
    uint64_t n_seq = 0, layers = 0, n_perm = 0, seed = 0, first_row = 0;
    std::vector<uint32_t> len, p_seq, p_pos;
    std::vector<uint8_t> p_cls;
    std::vector<u64> cb;
    std::vector<Query> queries;
    char word[16];
    uint64_t v[4];
    auto u64s = [&](int n, uint64_t most) {
        for (int k = 0; k < n; ++k)
            if (std::fscanf(f, "%" SCNu64, &v[k]) != 1 || v[k] > most) return false;
        return true;
    };
    const uint64_t kU32 = 0xFFFFFFFFull, kAny = ~0ull;
    while (std::fscanf(f, "%15s", word) == 1) {
        if (!std::strcmp(word, "n_seq")) {
            if (!u64s(1, kU32)) return 2;
            n_seq = v[0];
            len.assign(n_seq, 0u);
        } else if (!std::strcmp(word, "layers")) {
            if (!u64s(1, classmap::kMaxLayers) || v[0] < 1) return 2;
            layers = v[0];
        } else if (!std::strcmp(word, "perms")) {
            if (!u64s(1, enrich::kMaxPerms)) return 2;
            n_perm = v[0];
        } else if (!std::strcmp(word, "seed")) {
            if (!u64s(1, kAny)) return 2;
            seed = v[0];
        } else if (!std::strcmp(word, "first_row")) {
            if (!u64s(1, kAny)) return 2;
            first_row = v[0];
        } else if (!std::strcmp(word, "len")) {
            if (!u64s(2, kU32) || v[0] >= n_seq) return 2;
            len[v[0]] = (uint32_t)v[1];
        } else if (!std::strcmp(word, "p")) {
            if (!u64s(3, kU32) || v[0] >= n_seq || v[2] > layers) return 2;
            p_seq.push_back((uint32_t)v[0]), p_pos.push_back((uint32_t)v[1]), p_cls.push_back((uint8_t)v[2]);
        } else if (!std::strcmp(word, "cb")) {
            if (!layers || !u64s(1, kAny) || v[0] * layers != cb.size()) return 2;  // (in the points' order)
            for (uint64_t k = 0; k < layers; ++k) {
                if (!u64s(1, kAny)) return 2;
                cb.push_back(v[0]);
            }
        } else if (!std::strcmp(word, "q")) {
            if (!u64s(3, kU32)) return 2;
            queries.push_back(Query{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]});
        } else {
            return 2;
        }
    }
    std::fclose(f);
    if (!layers) return 2;
    const uint32_t T = (uint32_t)layers, T1 = T + 1;
    const size_t np = p_pos.size();
    if (cb.size() != np * T) return 2;
    std::vector<u64> p_off(n_seq + 1, 0);
    for (size_t i = 0; i < np; ++i) {
        if (i && p_seq[i] < p_seq[i - 1]) return 2;
        p_off[p_seq[i] + 1]++;
    }
    for (uint64_t c = 0; c < n_seq; ++c) p_off[c + 1] += p_off[c];
    for (const Query &q : queries)
        if (q.seq >= n_seq) return std::printf("range\n"), 3;
    const auto x_pos = exact(p_pos);
    const auto x_cls = exact(p_cls);
    const auto x_cb = exact(cb);
    const auto x_len = exact(len);
    std::vector<u64> zero((n_perm + 1) * T1, 0);
    const auto B = exact(zero), R = exact(zero);
    u64 unplaced = 0, width = 0;
    for (const Query &q : queries)
        if (q.start < q.end) width += q.end - q.start;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t p = 0; p <= n_perm; ++p) {
        const u64 key = enrich::perm_key(seed, p);
        u64 *b = B.get() + (size_t)p * T1, *r = R.get() + (size_t)p * T1;
        for (size_t j = 0; j < queries.size(); ++j) {
            const Query &q = queries[j];
            const enrich::Placement how = enrich::region_in_row(
                x_pos.get(), x_cls.get(), x_cb.get(), T, p_off[q.seq], p_off[q.seq + 1], x_len.get()[q.seq], q.start, q.end, p == 0,
                enrich::perm_draw(key, first_row + j), [&](uint32_t k, uint32_t n) { b[k] += n; }, [&](uint32_t k) { r[k]++; });
            if (p == 0 && how == enrich::kUnplaceable) ++unplaced;
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    u64 checksum = unplaced;
    for (uint32_t p = 0; p <= n_perm; ++p) {
        u64 sb = 0, sr = 0;
        for (uint32_t k = 0; k < T1; ++k) sb += B.get()[(size_t)p * T1 + k], sr += R.get()[(size_t)p * T1 + k], checksum += (k + 1) * B.get()[(size_t)p * T1 + k];
        if (sb != width || sr != queries.size()) return std::printf("inconsistent totals\n"), 4;
    }
    if (timed) {
        std::printf("regions %zu perms %" PRIu64 " ms %.3f checksum %llu\n", queries.size(), n_perm, ms, checksum);
        return 0;
    }
    std::printf("mix %016llX %016llX %016llX\n", enrich::mix64(enrich::kGold), enrich::mix64(enrich::kGold * 2), enrich::mix64(enrich::kGold * 3));
    for (uint32_t p = 0; p <= n_perm; ++p)
        for (const auto *M : {&B, &R}) {
            std::printf("%s %" PRIu32, M == &B ? "B" : "R", p);
            for (uint32_t k = 0; k < T1; ++k) std::printf(" %llu", M->get()[(size_t)p * T1 + k]);
            std::printf("\n");
        }
    std::printf("unplaced %llu\nregions %zu perms %" PRIu64 "\n", unplaced, queries.size(), n_perm);
    return 0;
}
