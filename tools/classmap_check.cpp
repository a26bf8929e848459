// classmap_check.cpp -- the host build of device/classmap_core.hpp (the class of a mask, the point rule, the canonical step,
// the bounded search and the region rule, as the kernels of classmap.hip run them) under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc classmap_check`), driven by tests/test_annotate_cpu.py.  The per-layer
// unions, the toggles and their order are restated here on the host (std::sort); every array the core reads is a heap
// allocation of exactly its size, so a read past it is reported.
//   classmap_check [--time] IN   IN: lines "n_seq N", "layers T", "row LAYER SEQ START END" and "q SEQ START END" in any
//                       order.  Out: "p SEQ POS CLASS" per point, "cb I V0 .. V(T-1)" per point, then one line per q line in
//                       their order: "a CLASS B0 .. BT" (CLASS is "." for none) or "range" for SEQ >= N; then
//                       "points <n> regions <n>".  A row with LAYER >= T, SEQ >= N or START >= END: "refused row", exit 3.
//                       A map that breaks its own invariants (a seqid's toggles not cancelling, a step that is not
//                       canonical, counts that do not add up): "inconsistent map", exit 4.
//                       --time (the -O2 build `classmap_host_baseline`, tools/annotate_bench.py): no lines but
//                       "points <n> regions <n> ms <answer loop, one core>".
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../gffx_amd/csrc/device/classmap_core.hpp"

using namespace gffx;
using classmap::u64;

namespace {

template <typename X>
std::unique_ptr<X[]> exact(const std::vector<X> &v) {
    std::unique_ptr<X[]> c(new X[v.size()]);  // (a zero-length allocation for an empty array: any read of it is reported)
    if (!v.empty()) std::memcpy(c.get(), v.data(), v.size() * sizeof(X));
    return c;
}

struct Row {
    uint32_t layer, seq, start, end;
};
struct Event {
    u64 key;
    uint32_t bit;
};
struct Query {
    uint32_t seq, start, end;
};

}  // namespace

int main(int argc, char **argv) {
    const bool timed = argc == 3 && !std::strcmp(argv[1], "--time");
    if (argc != 2 && !timed) {
        std::fprintf(stderr, "usage: classmap_check [--time] IN\n");
        return 2;
    }
    FILE *f = std::fopen(argv[argc - 1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[argc - 1]);
        return 2;
    }
    uint64_t n_seq = 0, layers = 0;
    std::vector<Row> rows;
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
            if (!u32s(1)) return 2;
            n_seq = v[0];
        } else if (!std::strcmp(word, "layers")) {
            if (!u32s(1)) return 2;
            layers = v[0];
        } else if (!std::strcmp(word, "row")) {
            if (!u32s(4)) return 2;
            rows.push_back(Row{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]});
        } else if (!std::strcmp(word, "q")) {
            if (!u32s(3)) return 2;
            queries.push_back(Query{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]});
        } else {
            return 2;
        }
    }
    std::fclose(f);
    if (layers < 1 || layers > classmap::kMaxLayers) return 2;
    const uint32_t T = (uint32_t)layers;
    for (const Row &r : rows)
        if (r.layer >= T || r.seq >= n_seq || r.start >= r.end) return std::printf("refused row\n"), 3;
    // one union per (layer, seqid): sorted by start, a row that begins at or before the current end extends the span
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
        return a.seq != b.seq ? a.seq < b.seq : a.layer != b.layer ? a.layer < b.layer : a.start < b.start;
    });
    std::vector<Event> ev;
    for (size_t i = 0; i < rows.size();) {
        uint32_t s = rows[i].start, e = rows[i].end;
        size_t j = i + 1;
        for (; j < rows.size() && rows[j].seq == rows[i].seq && rows[j].layer == rows[i].layer && rows[j].start <= e; ++j) e = std::max(e, rows[j].end);
        ev.push_back(Event{classmap::event_key(rows[i].seq, s), 1u << rows[i].layer});
        ev.push_back(Event{classmap::event_key(rows[i].seq, e), 1u << rows[i].layer});
        i = j;
    }
    std::sort(ev.begin(), ev.end(), [](const Event &a, const Event &b) { return a.key < b.key; });
    // the point rule over the sorted toggles
    std::vector<uint32_t> p_seq, p_pos;
    std::vector<uint8_t> p_cls;
    uint32_t run = 0, before = 0;
    for (size_t i = 0; i < ev.size(); ++i) {
        const bool has_next = i + 1 < ev.size();
        const u64 next = has_next ? ev[i + 1].key : 0;
        run ^= ev[i].bit;
        uint32_t cls = 0;
        if (classmap::point_here(ev[i].key, has_next, next, before, run, T, &cls))
            p_seq.push_back((uint32_t)(ev[i].key >> 32)), p_pos.push_back((uint32_t)ev[i].key), p_cls.push_back((uint8_t)cls);
        if (classmap::is_tail(ev[i].key, has_next, next)) before = run;
        if ((!has_next || (next >> 32) != (ev[i].key >> 32)) && run != 0) return std::printf("inconsistent map\n"), 4;  // a seqid's toggles cancel
    }
    const size_t np = p_pos.size();
    std::vector<u64> p_off(n_seq + 1, 0), cb(np * T, 0);
    for (size_t i = 0; i < np; ++i) p_off[p_seq[i] + 1]++;
    for (uint64_t c = 0; c < n_seq; ++c) p_off[c + 1] += p_off[c];
    std::vector<u64> acc(T, 0);
    for (size_t i = 0; i < np; ++i) {
        const bool first = i == 0 || p_seq[i - 1] != p_seq[i], last = i + 1 == np || p_seq[i + 1] != p_seq[i];
        if (!classmap::canonical_step(first, first ? 0u : p_pos[i - 1], first ? 0u : p_cls[i - 1], p_pos[i], p_cls[i], last, T))
            return std::printf("inconsistent map\n"), 4;
        for (uint32_t k = 0; k < T; ++k) cb[i * T + k] = acc[k];
        if (p_cls[i] < T) acc[p_cls[i]] += classmap::point_len(p_pos[i], !last, last ? 0u : p_pos[i + 1]);
    }
    if (!timed) {
        for (size_t i = 0; i < np; ++i) std::printf("p %" PRIu32 " %" PRIu32 " %u\n", p_seq[i], p_pos[i], (unsigned)p_cls[i]);
        for (size_t i = 0; i < np; ++i) {
            std::printf("cb %zu", i);
            for (uint32_t k = 0; k < T; ++k) std::printf(" %llu", cb[i * T + k]);
            std::printf("\n");
        }
    }
    const auto x_pos = exact(p_pos);
    const auto x_cls = exact(p_cls);
    const auto x_cb = exact(cb);
    std::vector<uint32_t> out_v(T + 1);
    const auto x_out = exact(out_v);
    uint64_t checksum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (const Query &q : queries) {
        if (q.seq >= n_seq) {
            if (!timed) std::printf("range\n");
            continue;
        }
        uint32_t *out = x_out.get();
        const uint32_t best = classmap::region_bases(x_pos.get(), x_cls.get(), x_cb.get(), T, p_off[q.seq], p_off[q.seq + 1], q.start, q.end, out);
        checksum += out[T] + best;
        if (timed) continue;
        uint64_t sum = 0;
        uint32_t lowest = T;
        for (uint32_t k = 0; k <= T; ++k) {
            sum += out[k];
            if (k < T && out[k] && lowest == T) lowest = k;
        }
        if (sum != (q.start < q.end ? (uint64_t)q.end - q.start : 0ull) || lowest != best) return std::printf("inconsistent map\n"), 4;
        if (best == T)
            std::printf("a .");
        else
            std::printf("a %" PRIu32, best);
        for (uint32_t k = 0; k <= T; ++k) std::printf(" %" PRIu32, out[k]);
        std::printf("\n");
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (timed)
        std::printf("points %zu regions %zu ms %.3f checksum %" PRIu64 "\n", np, queries.size(), ms, checksum);
    else
        std::printf("points %zu regions %zu\n", np, queries.size());
    return 0;
}
