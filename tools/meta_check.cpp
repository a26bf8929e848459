// meta_check.cpp -- the host build of device/meta_core.hpp (the column boundaries of `gffx meta`, their clamp) with
// device/pileup_core.hpp's B(x) between them, evaluated the way k_pileup_meta does it -- the window's searches first, every
// boundary's searches inside them, a column as the difference of two neighbouring boundaries -- and of host/feature_rows.hpp,
// under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C gffx_amd/csrc meta_check`), driven by tests/test_meta_cpu.py.
// The sorted keys, their prefix sums and the offsets are restated here on the host; every array the cores read is a heap
// allocation of exactly its size, so a read past it is reported.
//   meta_check IN              IN holds one case: "n_seq N", "layout MODE ANCHOR UP DOWN BIN M", then in any order lines
//                              "len SEQ LENGTH" (a seqid without one is 2^32 - 1 long), "row SEQ START END" and
//                              "feat SEQ START END MINUS".  Out, per feat line in their order: "bases v0 .. v{B-1}" and
//                              "len v0 .. v{B-1}"; then "col_bases ..", "col_len ..", "col_features .." and
//                              "rows <n> feats <n> columns <B>".  A layout that is none: "refused layout", exit 3; a row or
//                              a feat with SEQ >= N or START >= END: "refused row" / "refused feat", exit 3.
//                              Results are stored first and printed afterwards; "ms <t>" on stderr is the time of the bases
//                              alone (boundaries, searches, differences, column sums: what k_pileup_meta does per fold),
//                              "geometry_ms <t>" that of the widths (what _meta_set does once).  The unsanitized build is
//                              tools/meta_bench.py's one-core yardstick.
//   meta_check --strand-id GFF per line of GFF that is not empty and no comment: "<+|-> <0|1: stranded> <id>"
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../gffx_amd/csrc/device/meta_core.hpp"
#include "../gffx_amd/csrc/device/pileup_core.hpp"
#include "../gffx_amd/csrc/host/feature_rows.hpp"

using namespace gffx;
using pileup::u64;

namespace {

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    std::unique_ptr<T[]> c(new T[v.size()]);  // (a zero-length allocation for an empty array: any read of it is reported)
    if (!v.empty()) std::memcpy(c.get(), v.data(), v.size() * sizeof(T));
    return c;
}

struct Feat {
    uint32_t seq, start, end, minus;
};

int strand_id(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", path), 2;
    std::vector<char> bytes;
    char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    const auto x = exact(bytes);
    const std::string_view text(x.get(), bytes.size());
    for (size_t at = 0; at < text.size();) {
        size_t nl = text.find('\n', at);
        if (nl == std::string_view::npos) nl = text.size();
        if (nl > at && text[at] != '#' && text[at] != '\r') {
            const commands::feature_rows::StrandId r = commands::feature_rows::read_strand_id(text, at);
            std::printf("%c %d %.*s\n", r.minus ? '-' : '+', r.stranded ? 1 : 0, (int)r.id.size(), r.id.data());
        }
        at = nl + 1;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--strand-id")) return strand_id(argv[2]);
    if (argc != 2) {
        std::fprintf(stderr, "usage: meta_check IN | meta_check --strand-id GFF\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint64_t n_seq = 0;
    meta::Layout lay{0, 0, 0, 0, 0, 0};
    std::vector<Feat> rows, feats;
    std::vector<std::pair<uint64_t, uint64_t>> lens;
    char word[16];
    uint64_t v[6];
    const auto numbers = [&](int n) {
        for (int i = 0; i < n; ++i)
            if (std::fscanf(f, "%" SCNu64, &v[i]) != 1 || v[i] > 0xFFFFFFFFull) return false;
        return true;
    };
    while (std::fscanf(f, "%15s", word) == 1) {
        if (!std::strcmp(word, "n_seq")) {
            if (!numbers(1)) return 2;
            n_seq = v[0];
        } else if (!std::strcmp(word, "layout")) {
            if (!numbers(6)) return 2;
            lay = meta::Layout{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]};
        } else if (!std::strcmp(word, "len")) {
            if (!numbers(2)) return 2;
            lens.emplace_back(v[0], v[1]);
        } else if (!std::strcmp(word, "row")) {
            if (!numbers(3)) return 2;
            rows.push_back(Feat{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], 0});
        } else if (!std::strcmp(word, "feat")) {
            if (!numbers(4)) return 2;
            feats.push_back(Feat{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]});
        } else {
            return 2;
        }
    }
    std::fclose(f);
    const u64 B = meta::columns(lay);
    if (!B) return std::printf("refused layout\n"), 3;
    for (const Feat &r : rows)
        if (r.seq >= n_seq || r.start >= r.end) return std::printf("refused row\n"), 3;
    for (const Feat &t : feats)
        if (t.seq >= n_seq || t.start >= t.end) return std::printf("refused feat\n"), 3;
    std::vector<uint32_t> seq_len(n_seq, 0xFFFFFFFFu);
    for (const auto &l : lens)
        if (l.first < n_seq) seq_len[l.first] = (uint32_t)l.second;
    // what one fold builds on the device (tools/pileup_check.cpp)
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
    const auto x_len = exact(seq_len);
    const pileup::Keys K{x_s.get(), x_e.get(), x_ps.get(), x_pe.get()};
    std::vector<u64> col_bases(B, 0), col_len(B, 0), col_features(B, 0), below(B + 1);
    std::vector<u64> all_bases(feats.size() * B, 0), all_width(feats.size() * B, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < feats.size(); ++i) {
        const Feat &t = feats[i];
        u64 *bases = all_bases.data() + i * B;
        const u64 lo = x_off[t.seq], hi = x_off[t.seq + 1];
        const uint32_t len = x_len[t.seq];
        const bool minus = t.minus != 0;
        const uint32_t x_first = meta::boundary(lay, t.start, t.end, minus, len, 0), x_last = meta::boundary(lay, t.start, t.end, minus, len, B);
        const uint32_t x_min = minus ? x_last : x_first, x_max = minus ? x_first : x_last;
        bool flat = lo >= hi;  // B(x) is the same all over the window: every column has 0 bases
        u64 s_lo = lo, s_hi = lo, e_lo = lo, e_hi = lo;
        if (!flat) {
            s_lo = pileup::lower_bound(K.starts, lo, hi, x_min), s_hi = pileup::lower_bound(K.starts, s_lo, hi, x_max);
            e_lo = pileup::lower_bound(K.ends, lo, hi, x_min);
            flat = s_hi == lo || e_lo == hi;
            if (!flat) e_hi = pileup::lower_bound(K.ends, e_lo, hi, x_max);
        }
        for (u64 k = 0; k <= B && !flat; ++k) {
            const uint32_t x = meta::boundary(lay, t.start, t.end, minus, len, k);
            const u64 ps = pileup::lower_bound(K.starts, s_lo, s_hi, x), pe = pileup::lower_bound(K.ends, e_lo, e_hi, x);
            below[k] = pileup::bases_below(x, ps - lo, K.pre_s[ps] - K.pre_s[lo], pe - lo, K.pre_e[pe] - K.pre_e[lo]);
        }
        for (u64 j = 0; j < B && !flat; ++j) {
            bases[j] = minus ? below[j] - below[j + 1] : below[j + 1] - below[j];
            col_bases[j] += bases[j];
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < feats.size(); ++i) {
        const Feat &t = feats[i];
        for (u64 j = 0; j < B; ++j) {
            uint32_t a, b;
            meta::column(lay, t.start, t.end, t.minus != 0, x_len[t.seq], j, &a, &b);
            all_width[i * B + j] = b - a;
            col_len[j] += b - a, col_features[j] += b > a;
        }
    }
    const auto t2 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "ms %.3f\ngeometry_ms %.3f\n", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                 std::chrono::duration<double, std::milli>(t2 - t1).count());
    std::string out;
    char num[32];
    for (size_t i = 0; i < feats.size(); ++i)
        for (const std::vector<u64> *all : {&all_bases, &all_width}) {
            out += all == &all_bases ? "bases" : "len";
            for (u64 j = 0; j < B; ++j) out.append(num, std::snprintf(num, sizeof num, " %llu", (*all)[i * B + j]));
            out.push_back('\n');
        }
    for (const std::vector<u64> *row : {&col_bases, &col_len, &col_features}) {
        out += row == &col_bases ? "col_bases" : row == &col_len ? "col_len" : "col_features";
        for (u64 j = 0; j < B; ++j) out.append(num, std::snprintf(num, sizeof num, " %llu", (*row)[j]));
        out.push_back('\n');
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::printf("rows %zu feats %zu columns %llu\n", rows.size(), feats.size(), B);
    return 0;
}
