// seq_check.cpp -- device/seq_core.hpp and the Parent / phase helpers of host/feature_rows.hpp on the host, without a GPU
// (tests/test_seq_cpu.py builds it under ASan + UBSan and holds its answers to tests/_seq_definition.py); built without the
// sanitizers it is seq_host_baseline, the one-core yardstick of tools/seq_bench.py: the same rules, one thread.
//
//   seq_check --complement                 the 256 entries, two hex digits each
//   seq_check --translate P FILE           the bytes of FILE from offset P in codons of three
//   seq_check --wrap C W B...              body_bytes(C, W), then per byte offset B the character it holds ('n': a newline)
//   seq_check --fasta FILE [PIECE]         the sequences (name, length, bases) as classify_line / name_end give them, the text
//                                          handed over in pieces of PIECE bytes the way the genome object cuts it; an error: "error LINE WHAT"
//   seq_check --fields FILE                per non-comment line: strand, phase, ID, and the Parent names
//   seq_check --run GFF FASTA TYPES JOIN TRANSLATE W OUT   the command on one core; the stage times to stderr
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <unordered_map>
#include <vector>

#include "../gffx_amd/csrc/device/seq_core.hpp"
#include "../gffx_amd/csrc/host/feature_rows.hpp"

namespace sq = gffx::seq;
namespace fr = gffx::commands::feature_rows;
typedef unsigned long long u64;

static std::string slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

struct Fasta {
    std::vector<std::string> names, seqs;
    u64 bad_line = 0;
    const char *bad = nullptr;
};

// The text in pieces of `piece` bytes (0: whole): per piece its lines are classified with the flags the genome object passes --
// a piece may end inside a bases line (the next begins with a continuation); an unfinished header line and a '\r' that may
// belong to a "\r\n" are held back.
static Fasta parse_fasta(const std::string &text, size_t piece) {
    Fasta F;
    std::unordered_map<std::string, int> seen;
    std::string held;
    bool mid = false;
    u64 lines_done = 0;
    auto pass = [&](std::string D, bool last) {
        if (!last && !D.empty()) {
            const size_t q = D.rfind('\n');
            const size_t t0 = q == std::string::npos ? 0 : q + 1;
            const bool tail_continues = q == std::string::npos && mid;
            if (t0 < D.size()) {
                if (!tail_continues && D[t0] == '>') held = D.substr(t0), D.resize(t0);
                else if (D.back() == '\r') held = "\r", D.pop_back();
            }
        }
        if (D.empty()) return true;
        const uint8_t *p = reinterpret_cast<const uint8_t *>(D.data());
        const u64 N = D.size();
        u64 ls = 0, i = 0;
        while (ls < N) {
            const void *e = std::memchr(p + ls, '\n', N - ls);
            const u64 le = e ? (u64)(static_cast<const uint8_t *>(e) - p) : N;
            const bool terminated = e != nullptr;
            const sq::LineClass c = sq::classify_line(p, ls, le, terminated, mid && i == 0);
            const u64 line_no = lines_done + i + 1;
            if (c.kind == sq::kLineHeader) {
                const u64 end = terminated && p[le - 1] == '\r' ? le - 1 : le;
                const u64 ne = sq::name_end(p, ls, end);
                std::string name(D, ls + 1, ne - ls - 1);
                if (name.empty()) return F.bad_line = line_no, F.bad = "no name", false;
                if (!seen.emplace(name, 1).second) return F.bad_line = line_no, F.bad = "twice", false;
                F.names.push_back(name), F.seqs.emplace_back();
            } else if (c.kind == sq::kLineBases && c.kept) {
                if (F.names.empty()) return F.bad_line = line_no, F.bad = "before the first >", false;
                F.seqs.back().append(D, ls, c.kept);
            }
            ls = le + 1, ++i;
        }
        const bool final_line = D.back() != '\n';
        lines_done += i - (final_line ? 1 : 0);
        mid = final_line;
        return true;
    };
    if (piece == 0) piece = text.size() ? text.size() : 1;
    for (size_t at = 0; at < text.size(); at += piece) {
        std::string D = held;
        held.clear();
        D.append(text, at, piece);
        if (!pass(std::move(D), false)) return F;
    }
    if (!held.empty()) {
        std::string D = held;
        held.clear();
        pass(std::move(D), true);
    }
    return F;
}

static std::string wrap(const std::string &chars, u64 W) {
    std::string out(sq::body_bytes(chars.size(), W), '\n');
    for (u64 b = 0; b < out.size(); ++b) {
        const u64 c = sq::body_char(b, chars.size(), W);
        if (c < chars.size()) out[b] = chars[c];
    }
    return out;
}

static std::string characters(std::string bases, bool minus, uint32_t p, bool translated) {
    if (minus) {
        std::reverse(bases.begin(), bases.end());
        for (char &ch : bases) ch = (char)sq::complement((uint8_t)ch);
    }
    if (!translated) return bases;
    const u64 C = sq::characters(bases.size(), p, true);
    std::string aa(C, 'X');
    for (u64 c = 0; c < C; ++c) aa[c] = (char)sq::translate((uint8_t)bases[p + 3 * c], (uint8_t)bases[p + 3 * c + 1], (uint8_t)bases[p + 3 * c + 2]);
    return aa;
}

struct Feature {
    std::string seqid;
    uint32_t start, end;
    fr::SeqFields f;
};

static int run(int argc, char **argv) {
    if (argc != 9) return 2;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string gff = slurp(argv[2]), fasta = slurp(argv[3]);
    std::vector<std::string> types;
    for (const char *p = argv[4];;) {
        const char *c = std::strchr(p, ',');
        types.emplace_back(p, c ? (size_t)(c - p) : std::strlen(p));
        if (!c) break;
        p = c + 1;
    }
    const bool join = std::atoi(argv[5]) != 0, translated = std::atoi(argv[6]) != 0;
    const u64 W = std::strtoull(argv[7], nullptr, 10);
    const auto t1 = std::chrono::steady_clock::now();
    const Fasta F = parse_fasta(fasta, 0);
    if (F.bad) {
        std::printf("error %llu %s\n", F.bad_line, F.bad);
        return 1;
    }
    std::unordered_map<std::string, const std::string *> genome;
    for (size_t i = 0; i < F.names.size(); ++i) genome[F.names[i]] = &F.seqs[i];
    const auto t2 = std::chrono::steady_clock::now();
    std::vector<Feature> feats;
    const std::string_view text(gff);
    for (size_t ls = 0; ls < text.size();) {
        size_t le = text.find('\n', ls);
        if (le == std::string_view::npos) le = text.size();
        std::string_view line = text.substr(ls, le - ls);
        const size_t line_start = ls;
        ls = le + 1;
        if (line.empty() || line[0] == '#') continue;
        std::string_view col[5];
        size_t at = 0;
        int n = 0;
        for (; n < 5; ++n) {
            const size_t tab = line.find('\t', at);
            if (tab == std::string_view::npos) break;
            col[n] = line.substr(at, tab - at);
            at = tab + 1;
        }
        if (n < 5 || std::find(types.begin(), types.end(), std::string(col[2])) == types.end()) continue;
        char *e1 = nullptr, *e2 = nullptr;
        const std::string a(col[3]), b(col[4]);
        const u64 s = std::strtoull(a.c_str(), &e1, 10), e = std::strtoull(b.c_str(), &e2, 10);
        if (a.empty() || b.empty() || *e1 || *e2 || s < 1 || s > e || e > 0xFFFFFFFFull) continue;
        feats.push_back(Feature{std::string(col[0]), (uint32_t)s, (uint32_t)e, fr::read_seq_fields(text, line_start)});
    }
    const auto t2f = std::chrono::steady_clock::now();
    const auto served = [&](const Feature &f) {
        const auto it = genome.find(f.seqid);
        return it != genome.end() && f.end <= it->second->size();
    };
    std::string out;
    char num[96];
    if (!join) {
        for (const Feature &f : feats) {
            if (!served(f)) continue;
            const std::string chars = characters(genome[f.seqid]->substr(f.start - 1, f.end - f.start + 1), f.f.si.minus, sq::phase_skip((uint8_t)f.f.phase), translated);
            out += ">" + std::string(f.f.si.id) + " " + f.seqid;
            out.append(num, std::snprintf(num, sizeof num, ":%u-%u(%c)\n", f.start, f.end, f.f.strand));
            out += wrap(chars, W);
        }
    } else {
        std::unordered_map<std::string_view, size_t> by_name;
        std::vector<std::pair<std::string_view, std::vector<size_t>>> recs;
        for (size_t i = 0; i < feats.size(); ++i)
            fr::for_each_parent(feats[i].f.parent, [&](std::string_view name) {
                const auto [it, fresh] = by_name.emplace(name, recs.size());
                if (fresh) recs.emplace_back(name, std::vector<size_t>());
                recs[it->second].second.push_back(i);
            });
        for (auto &[name, members] : recs) {
            const Feature &first = feats[members[0]];
            bool ok = true;
            uint32_t lo = first.start, hi = first.end;
            for (size_t i : members) {
                ok = ok && feats[i].seqid == first.seqid && feats[i].f.si.minus == first.f.si.minus && served(feats[i]);
                lo = std::min(lo, feats[i].start), hi = std::max(hi, feats[i].end);
            }
            if (!ok) continue;
            std::vector<size_t> order = members;
            std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return feats[x].start < feats[y].start; });
            std::string bases;
            for (size_t i : order) bases.append(*genome[first.seqid], feats[i].start - 1, feats[i].end - feats[i].start + 1);
            const Feature &lead = feats[first.f.si.minus ? order.back() : order.front()];
            const std::string chars = characters(std::move(bases), first.f.si.minus, sq::phase_skip((uint8_t)lead.f.phase), translated);
            out += ">" + std::string(name) + " " + first.seqid;
            out.append(num, std::snprintf(num, sizeof num, ":%u-%u(%c) segments=%zu\n", lo, hi, first.f.strand, members.size()));
            out += wrap(chars, W);
        }
    }
    const auto t3 = std::chrono::steady_clock::now();
    std::ofstream o(argv[8], std::ios::binary);
    o.write(out.data(), (std::streamsize)out.size());
    o.close();
    const auto t4 = std::chrono::steady_clock::now();
    const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    // (records_ms: grouping, gathering, complementing, translating and wrapping -- what the plan and the emit do on the device)
    std::fprintf(stderr, "read_ms %.3f fasta_ms %.3f features_ms %.3f records_ms %.3f write_ms %.3f total_ms %.3f bytes %zu\n", ms(t0, t1), ms(t1, t2), ms(t2, t2f),
                 ms(t2f, t3), ms(t3, t4), ms(t0, t4), out.size());
    return o ? 0 : 1;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "--complement") {
        for (int b = 0; b < 256; ++b) std::printf("%02x", sq::complement((uint8_t)b));
        std::printf("\n");
        return 0;
    }
    if (mode == "--translate" && argc == 4) {
        const std::string s = slurp(argv[3]);
        const uint32_t p = (uint32_t)std::atoi(argv[2]);
        const u64 C = sq::characters(s.size(), p, true);
        std::string aa;
        for (u64 c = 0; c < C; ++c) aa.push_back((char)sq::translate((uint8_t)s[p + 3 * c], (uint8_t)s[p + 3 * c + 1], (uint8_t)s[p + 3 * c + 2]));
        std::printf("%s\n", aa.c_str());
        return 0;
    }
    if (mode == "--wrap" && argc >= 4) {
        const u64 C = std::strtoull(argv[2], nullptr, 10), W = std::strtoull(argv[3], nullptr, 10);
        std::printf("%llu", sq::body_bytes(C, W));
        for (int k = 4; k < argc; ++k) {
            const u64 c = sq::body_char(std::strtoull(argv[k], nullptr, 10), C, W);
            if (c >= C) std::printf(" n");
            else std::printf(" %llu", c);
        }
        std::printf("\n");
        return 0;
    }
    if (mode == "--fasta" && argc >= 3) {
        const Fasta F = parse_fasta(slurp(argv[2]), argc > 3 ? (size_t)std::strtoull(argv[3], nullptr, 10) : 0);
        if (F.bad) {
            std::printf("error %llu %s\n", F.bad_line, F.bad);
            return 1;
        }
        for (size_t i = 0; i < F.names.size(); ++i) std::printf("%s %zu %s\n", F.names[i].c_str(), F.seqs[i].size(), F.seqs[i].c_str());
        return 0;
    }
    if (mode == "--fields" && argc == 3) {
        const std::string gff = slurp(argv[2]);
        const std::string_view text(gff);
        for (size_t ls = 0; ls < text.size();) {
            size_t le = text.find('\n', ls);
            if (le == std::string_view::npos) le = text.size();
            if (le > ls && text[ls] != '#') {
                const fr::SeqFields f = fr::read_seq_fields(text, ls);
                std::printf("%c %c %.*s |", f.strand, f.phase, (int)f.si.id.size(), f.si.id.data());
                size_t n = 0;
                fr::for_each_parent(f.parent, [&](std::string_view name) {
                    if (n++ < 3 || name.size() > 20) std::printf(" %.*s", (int)name.size(), name.data());
                });
                std::printf(" (%zu)\n", n);
            }
            ls = le + 1;
        }
        return 0;
    }
    if (mode == "--run") return run(argc, argv);
    std::fprintf(stderr, "usage: seq_check --complement | --translate P FILE | --wrap C W B... | --fasta FILE [PIECE] | --fields FILE | --run ...\n");
    return 2;
}
