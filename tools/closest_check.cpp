// closest_check.cpp -- the host build of device/closest_core.hpp (the class and gap of a root, the flag rules, the bounded
// searches and the tie walks, as k_closest_count / k_closest_emit run them) under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc closest_check`), driven by tests/test_closest_cpu.py.  The start-sorted
// roots, the running maximum of their ends and the end table are restated here on the host (std::stable_sort); every array the
// core reads is a heap allocation of exactly its size, so a read past it is reported.  Where the device enumerates a region's
// overlaps with Join A's skip links, this program walks back from p while the running maximum still exceeds the region's start.
//   closest_check [--time] IN   IN: a line "n_seq N", then lines "root SEQ START END" (a seqid's roots in builder order) and
//                       "q FLAGS SEQ START END" in any order.  One line out per q line, in their order:
//                       "a COUNT GAP POS..." (index positions over all seqids, ascending; GAP is "-" when COUNT is 0),
//                       "range" for SEQ >= N, "flags" for refused flags; then "roots <n> regions <n>".
//                       A root with SEQ >= N or END < START: "refused root" and exit 3.
//                       --time (the -O2 build `closest_host_baseline`, tools/closest_bench.py): no answer lines, but
//                       "pairs <n> ms <answer loop, one core>".
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../gffx_amd/csrc/device/closest_core.hpp"

using namespace gffx;

namespace {

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    std::unique_ptr<T[]> c(new T[v.size()]);  // (a zero-length allocation for an empty array: any read of it is reported)
    if (!v.empty()) std::memcpy(c.get(), v.data(), v.size() * sizeof(T));
    return c;
}

struct Root {
    uint32_t seq, start, end;
};
struct Query {
    uint32_t flags, seq, start, end;
};

}  // namespace

int main(int argc, char **argv) {
    const bool timed = argc == 3 && !std::strcmp(argv[1], "--time");
    if (argc != 2 && !timed) {
        std::fprintf(stderr, "usage: closest_check [--time] IN\n");
        return 2;
    }
    FILE *f = std::fopen(argv[argc - 1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[argc - 1]);
        return 2;
    }
    uint64_t n_seq = 0;
    std::vector<Root> roots;
    std::vector<Query> queries;
    char word[16];
    uint64_t v[4];
    auto u32s = [&](int n) {
        for (int k = 0; k < n; ++k)
            if (std::fscanf(f, "%" SCNu64, &v[k]) != 1 || v[k] > 0xFFFFFFFFull) return false;
        return true;
    };
    while (std::fscanf(f, "%15s", word) == 1) {
        if (!std::strcmp(word, "n_seq")) {
            if (std::fscanf(f, "%" SCNu64, &n_seq) != 1 || n_seq > 0xFFFFFFFFull) return 2;
        } else if (!std::strcmp(word, "root")) {
            if (!u32s(3)) return 2;
            roots.push_back(Root{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]});
        } else if (!std::strcmp(word, "q")) {
            if (!u32s(4)) return 2;
            queries.push_back(Query{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]});
        } else {
            return 2;
        }
    }
    std::fclose(f);
    for (const Root &r : roots)
        if (r.seq >= n_seq || r.end < r.start) return std::printf("refused root\n"), 3;
    // what the index holds: the roots seqid after seqid, each seqid stably by start; the running maximum of the ends up to and
    // including a position, restarting with every seqid; off[c] = the roots with seqid < c
    std::stable_sort(roots.begin(), roots.end(), [](const Root &a, const Root &b) { return a.seq != b.seq ? a.seq < b.seq : a.start < b.start; });
    const size_t n = roots.size();
    std::vector<uint32_t> start(n), end(n), pmax(n), off(n_seq + 1, 0), order(n), e_end(n), e_pos(n);
    for (size_t i = 0; i < n; ++i) {
        start[i] = roots[i].start, end[i] = roots[i].end;
        pmax[i] = (i && roots[i - 1].seq == roots[i].seq) ? std::max(pmax[i - 1], end[i]) : end[i];
        off[roots[i].seq + 1]++;
        order[i] = (uint32_t)i;
    }
    for (uint64_t c = 0; c < n_seq; ++c) off[c + 1] += off[c];
    // ... and the end table: stably by (seqid, end), so equal ends keep ascending position
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return roots[a].seq != roots[b].seq ? roots[a].seq < roots[b].seq : roots[a].end < roots[b].end;
    });
    for (size_t i = 0; i < n; ++i) e_end[i] = end[order[i]], e_pos[i] = order[i];
    const auto x_start = exact(start), x_end = exact(end), x_pmax = exact(pmax), x_off = exact(off), x_e_end = exact(e_end), x_e_pos = exact(e_pos);
    const uint32_t *p_start = x_start.get(), *p_end = x_end.get(), *p_pmax = x_pmax.get(), *p_e_end = x_e_end.get(), *p_e_pos = x_e_pos.get();
    auto start_at = [&](uint32_t i) { return p_start[i]; };
    auto e_end_at = [&](uint32_t j) { return p_e_end[j]; };

    std::vector<uint32_t> ans;
    uint64_t pairs = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (const Query &q : queries) {
        if (!closest::flags_ok(q.flags)) {
            if (!timed) std::printf("flags\n");
            continue;
        }
        if (q.seq >= n_seq) {
            if (!timed) std::printf("range\n");
            continue;
        }
        ans.clear();
        uint32_t gap = 0;
        const uint32_t first = x_off[q.seq], last = x_off[q.seq + 1];
        if (q.start < q.end && first < last) {
            const uint32_t qs = q.start, qe = q.end;
            const uint32_t p = closest::first_ge(first, last, qe, start_at);
            const bool over = p > first && p_pmax[p - 1] > qs;
            for (uint32_t i = p; i > first && p_pmax[i - 1] > qs; --i)
                if (closest::class_of(p_start[i - 1], p_end[i - 1], qs, qe) == closest::kOver) ans.push_back(i - 1);
            if (over && !(q.flags & closest::kIgnoreOverlaps)) {
                std::reverse(ans.begin(), ans.end());
            } else {
                const uint32_t n_over = static_cast<uint32_t>(ans.size());
                ans.clear();
                const closest::Nearest a = closest::nearest(first, last, p, n_over, qs, qe, q.flags, start_at, e_end_at);
                for (uint32_t j = a.l0; j < a.l1; ++j) ans.push_back(p_e_pos[j]);
                for (uint32_t k = a.r0; k < a.r1; ++k) ans.push_back(k);
                gap = a.gap;
                // the header's claims, on every answered root: a candidate of its class under the flags, at that gap
                for (uint32_t k : ans) {
                    const closest::Class c = closest::class_of(p_start[k], p_end[k], qs, qe);
                    if (c == closest::kOver || !closest::candidate(c, q.flags) || closest::gap_of(c, p_start[k], p_end[k], qs, qe) != gap)
                        return std::printf("inconsistent answer\n"), 4;
                }
            }
        }
        pairs += ans.size();
        if (timed) continue;
        std::printf("a %zu ", ans.size());
        if (ans.empty())
            std::printf("-");
        else
            std::printf("%" PRIu32, gap);
        for (uint32_t k : ans) std::printf(" %" PRIu32, k);
        std::printf("\n");
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (timed)
        std::printf("pairs %" PRIu64 " ms %.3f\n", pairs, ms);
    else
        std::printf("roots %zu regions %zu\n", roots.size(), queries.size());
    return 0;
}
