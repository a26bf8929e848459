// profile_check.cpp -- the host build of device/profile_core.hpp (the point rule, the threshold rule and depth_at, as the
// kernels of profile.hip run them) under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc profile_check`),
// driven by tests/test_profile_cpu.py.  The events are built and sorted here on the host (std::sort); every array the core
// reads is a heap allocation of exactly its size, so a read past it is reported.
//   profile_check IN    IN holds one case: a line "n_seq N", then lines "row SEQ START END", "thr T", "seg SEQ START END" and
//                       "at SEQ X" in any order.  Out, in this order:
//                         "point SEQ POS DEPTH"      the canonical points, by (seqid, position)
//                         "span T SEQ START END"     per thr line in their order: the spans "depth >= T"
//                         "covered T BASES"          per thr line and seg line in their order: the segment's bases at depth >= T
//                         "depth D"                  per at line
//                         "rows <n> points <n>"
//                       A row with SEQ >= N or START >= END, a seg or at with SEQ >= N, or thr 0: "refused <what>" and exit 3.
//                       The tool also asserts what the device's one unsegmented scan rests on -- every seqid's deltas add up to
//                       zero and every seqid's last depth is 0 --: "broken <what>" and exit 4.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../gffx_amd/csrc/device/profile_core.hpp"

using namespace gffx;
using profile::u64;

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
struct Event {
    u64 key;
    uint32_t delta;
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: profile_check IN\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint64_t n_seq = 0;
    std::vector<Triple> rows, segs, ats;
    std::vector<uint32_t> thr;
    char word[16];
    uint64_t a = 0, b = 0, c = 0;
    const uint64_t kMax = 0xFFFFFFFFull;
    while (std::fscanf(f, "%15s", word) == 1) {
        if (!std::strcmp(word, "n_seq")) {
            if (std::fscanf(f, "%" SCNu64, &n_seq) != 1) return 2;
        } else if (!std::strcmp(word, "thr")) {
            if (std::fscanf(f, "%" SCNu64, &a) != 1 || a > kMax) return 2;
            thr.push_back((uint32_t)a);
        } else if (!std::strcmp(word, "at")) {
            if (std::fscanf(f, "%" SCNu64 " %" SCNu64, &a, &b) != 2 || a > kMax || b > kMax) return 2;
            ats.push_back(Triple{(uint32_t)a, (uint32_t)b, 0});
        } else if (!std::strcmp(word, "row") || !std::strcmp(word, "seg")) {
            if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) != 3 || a > kMax || b > kMax || c > kMax) return 2;
            (word[0] == 'r' ? rows : segs).push_back(Triple{(uint32_t)a, (uint32_t)b, (uint32_t)c});
        } else {
            return 2;
        }
    }
    std::fclose(f);
    for (const Triple &r : rows) {
        if (r.seq >= n_seq) return std::printf("refused row chr\n"), 3;
        if (r.start >= r.end) return std::printf("refused row interval\n"), 3;
    }
    for (const Triple &s : segs)
        if (s.seq >= n_seq) return std::printf("refused seg chr\n"), 3;
    for (const Triple &s : ats)
        if (s.seq >= n_seq) return std::printf("refused at chr\n"), 3;
    for (const uint32_t T : thr)
        if (!T) return std::printf("refused thr\n"), 3;
    // what one fold builds on the device: two events per row, sorted by (seqid, position)
    std::vector<Event> ev;
    ev.reserve(2 * rows.size());
    for (const Triple &r : rows) {
        ev.push_back(Event{profile::event_key(r.seq, r.start), 1u});
        ev.push_back(Event{profile::event_key(r.seq, r.end), 0xFFFFFFFFu});
    }
    std::sort(ev.begin(), ev.end(), [](const Event &x, const Event &y) { return x.key < y.key; });
    std::vector<u64> keys(ev.size());
    std::vector<uint32_t> deltas(ev.size());
    for (size_t i = 0; i < ev.size(); ++i) keys[i] = ev[i].key, deltas[i] = ev[i].delta;
    const auto x_key = exact(keys);
    const auto x_delta = exact(deltas);
    const size_t n = ev.size();
    // the invariant of the unsegmented scan: the running sum is 0 wherever the seqid changes, and at the end
    {
        uint32_t run = 0;
        for (size_t i = 0; i < n; ++i) {
            if (i && (x_key[i] >> 32) != (x_key[i - 1] >> 32) && run != 0) return std::printf("broken deltas of a seqid do not add up to zero\n"), 4;
            run += x_delta[i];
        }
        if (run != 0) return std::printf("broken deltas of a seqid do not add up to zero\n"), 4;
    }
    // the point rule over the sorted events: the running depth, and the depth behind the previous tail
    std::vector<uint32_t> p_seq, p_pos, p_depth;
    {
        uint32_t run = 0, before = 0;
        for (size_t i = 0; i < n; ++i) {
            run += x_delta[i];
            const bool has_next = i + 1 < n;
            const u64 next = has_next ? x_key[i + 1] : 0ull;
            uint32_t d = 0;
            if (profile::point_here(x_key[i], has_next, next, before, run, &d))
                p_seq.push_back((uint32_t)(x_key[i] >> 32)), p_pos.push_back((uint32_t)x_key[i]), p_depth.push_back(d);
            if (profile::is_tail(x_key[i], has_next, next)) before = run;
        }
    }
    const size_t np = p_pos.size();
    std::vector<u64> p_off(n_seq + 1, 0);
    for (size_t i = 0; i < np; ++i) p_off[p_seq[i] + 1]++;
    for (uint64_t q = 0; q < n_seq; ++q) p_off[q + 1] += p_off[q];
    const auto x_seq = exact(p_seq), x_pos = exact(p_pos), x_depth = exact(p_depth);
    const auto x_off = exact(p_off);
    for (size_t i = 0; i < np; ++i) {
        const bool first = i == 0 || x_seq[i - 1] != x_seq[i], last = i + 1 == np || x_seq[i + 1] != x_seq[i];
        if (last && x_depth[i] != 0) return std::printf("broken the last depth of a seqid is not 0\n"), 4;
        if (!profile::canonical_step(first, first ? 0u : x_pos[i - 1], first ? 0u : x_depth[i - 1], x_pos[i], x_depth[i], last))
            return std::printf("broken the points are not canonical\n"), 4;
        std::printf("point %u %u %u\n", x_seq[i], x_pos[i], x_depth[i]);
    }
    // the threshold rule: span k opens at the k-th opening point and closes at the close behind it
    std::vector<std::vector<Triple>> spans(thr.size());
    for (size_t k = 0; k < thr.size(); ++k) {
        for (size_t i = 0; i < np; ++i) {
            const bool first = i == 0 || x_seq[i - 1] != x_seq[i];
            const uint32_t d_prev = first ? 0u : x_depth[i - 1];
            if (profile::span_opens(thr[k], first, d_prev, x_depth[i])) spans[k].push_back(Triple{x_seq[i], x_pos[i], 0});
            if (profile::span_closes(thr[k], first, d_prev, x_depth[i])) {
                if (spans[k].empty() || spans[k].back().end != 0 || spans[k].back().seq != x_seq[i]) return std::printf("broken a span closes that is not open\n"), 4;
                spans[k].back().end = x_pos[i];
            }
        }
        for (const Triple &s : spans[k]) {
            if (s.end <= s.start) return std::printf("broken a span is not closed\n"), 4;
            std::printf("span %u %u %u %u\n", thr[k], s.seq, s.start, s.end);
        }
    }
    for (size_t k = 0; k < thr.size(); ++k)
        for (const Triple &g : segs) {
            u64 total = 0;
            for (const Triple &s : spans[k]) {
                if (s.seq != g.seq) continue;
                const uint32_t lo = std::max(s.start, g.start), hi = std::min(s.end, g.end);
                if (hi > lo) total += hi - lo;
            }
            std::printf("covered %u %llu\n", thr[k], total);
        }
    for (const Triple &s : ats) std::printf("depth %u\n", profile::depth_at(x_pos.get(), x_depth.get(), x_off[s.seq], x_off[s.seq + 1], s.start));
    std::printf("rows %zu points %zu\n", rows.size(), np);
    return 0;
}
