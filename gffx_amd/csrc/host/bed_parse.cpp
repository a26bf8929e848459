// bed_parse.cpp -- the BED text parser of `gffx intersect` (commands/intersect.rs:201-230): whole files and the streaming CLI's chunks
#include <algorithm>
#include <cstring>
#include <exception>

#include "intersect_internal.hpp"

namespace gffx::commands::intersect {

// Cut [0, size) at line starts into about `parts` pieces (the file's lines, each piece whole lines).
std::vector<size_t> line_chunks(std::string_view d, size_t parts) {
    std::vector<size_t> cut{0};
    for (size_t p = 1; p < parts; ++p) {
        size_t at = d.size() * p / parts;
        if (at <= cut.back()) continue;
        const size_t nl = d.find('\n', at);
        if (nl == std::string_view::npos) break;
        if (nl + 1 > cut.back() && nl + 1 < d.size()) cut.push_back(nl + 1);
    }
    cut.push_back(d.size());
    return cut;
}

std::vector<uint32_t> flatten(const std::vector<Region> &regions) {
    std::vector<uint32_t> flat(regions.size() * 3);
    uint32_t *p = flat.data();
    for (const auto &[c, s, e] : regions) *p++ = c, *p++ = s, *p++ = e;
    return flat;
}

std::vector<Region> regions_of(const std::vector<std::vector<uint32_t>> &pieces) {
    size_t total = 0;
    for (const auto &v : pieces) total += v.size() / 3;
    std::vector<Region> regions;
    regions.reserve(total);
    for (const auto &v : pieces)
        for (size_t i = 0; i + 2 < v.size(); i += 3) regions.emplace_back(v[i], v[i + 1], v[i + 2]);
    return regions;
}

namespace {

// u8::is_ascii_whitespace as a table (split_ascii_whitespace, intersect.rs:214): space, \t, \n, \x0C, \r
struct WsTable {
    bool t[256] = {};
    constexpr explicit WsTable(bool newline = true) {
        t[' '] = t['\t'] = t['\x0C'] = t['\r'] = true;
        t['\n'] = newline;
    }
};
constexpr WsTable kWs{};
constexpr WsTable kBlank{false};  // the same without the newline: whitespace INSIDE a line

// lexical_core::parse::<u32>: optional '+', >= 1 digits, the whole field, no overflow
inline bool field_u32(const char *p, const char *e, uint32_t &out) {
    if (p < e && *p == '+') ++p;
    if (p == e) return false;
    uint64_t v = 0;
    for (; p < e; ++p) {
        const unsigned d = static_cast<unsigned char>(*p) - '0';
        if (d > 9) return false;
        v = v * 10 + d;
        if (v > 0xFFFFFFFFull) return false;
    }
    out = static_cast<uint32_t>(v);
    return true;
}

// intersect.rs:201-230 on the lines of d[a, z); z is a line start or the end of the file.  Rows as flat (chr, start, end)
// words -- the layout the device reads.  One pass per line: memchr for the newline, a word-wise scan for bytes >= 0x80 (only
// then the full UTF-8 validation the reference's from_utf8 implies), the first three whitespace-separated fields.
void parse_bed_chunk(std::string_view d, size_t a, size_t z, bool last, const SeqidTable &seqids, std::vector<uint32_t> &rows) {
    const char *base = d.data();
    const char *lim = base + z;
    // rows of the word-at-a-time path wait here, 64 at a time (three push_backs per row through a reference cost a third of
    // that path); every other way out of a line flushes first, so the order is the file's
    uint32_t pend[192];
    size_t n_pend = 0;
    auto flush = [&] {
        rows.insert(rows.end(), pend, pend + n_pend);
        n_pend = 0;
    };
    struct Flusher {
        decltype(flush) &f;
        ~Flusher() { f(); }  // (also on the way out of a parse error: the rows before it are the caller's, as before)
    } flusher{flush};
    while (last ? a <= z : a < z) {
        // The usual row in ONE pass over its bytes, without looking for the line end first: a name that starts the line (its
        // hash computed on the way), then two fields of 1-9 digits (no sign, no overflow possible), each ended by whitespace
        // or the end of the text; the rest of the line is only checked for bytes >= 0x80.  Anything else -- a comment, a
        // leading blank, a sign, 10 digits, a non-digit, a non-ASCII byte -- takes the general path below, which keeps the
        // reference's order: invalid UTF-8 -> error, fewer than 3 fields -> skipped, unknown seqid -> skipped, only then a
        // parse error.  (45 instead of 80 ns per row on one core.)
        // The plainest row -- a known-shape name of 1-7 bytes, TAB, 1-9 digits, TAB, 1-9 digits, then the line's end or more
        // whitespace-separated columns -- eight bytes at a time: the name is one word (its own hash key), a number is one word
        // and three multiplications.  Whatever does not look exactly like that falls through to the byte loop below, which
        // accepts a superset; both give the rows of the general path.  (72 -> ~25 ns per row and core on the GPU box.)
        if (a + 48 <= d.size()) {  // (every load below stays inside the text)
            const char *q = base + a;
            const uint64_t nw = load8(q);
            const unsigned nl = first_below_21(nw);
            if (nl >= 1 && nl <= 7 && q[nl] == '\t' && q[0] != '#') {
                const uint64_t key = nw & ((1ull << (8 * nl)) - 1);
                uint32_t v1, v2;
                const char *p1 = q + nl + 1;
                const unsigned n1 = (key & 0x8080808080808080ull) ? 0 : digits_1_to_9(p1, v1);
                if (n1 && p1[n1] == '\t') {
                    const char *p2 = p1 + n1 + 1;
                    const unsigned n2 = digits_1_to_9(p2, v2);
                    const unsigned char after = n2 ? static_cast<unsigned char>(p2[n2]) : 'x';
                    if (n2 && kWs.t[after] && p2 + n2 < lim) {
                        const char *e = p2 + n2;
                        bool ascii = true;
                        if (after != '\n') {  // more columns (or a CR): find the line's end, look for bytes >= 0x80
                            const char *nlp = static_cast<const char *>(std::memchr(e, '\n', static_cast<size_t>(lim - e)));
                            const char *e2 = nlp ? nlp : lim;
                            uint64_t hi = 0;
                            const char *r = e;
                            for (; r + 8 <= e2; r += 8) hi |= load8(r);
                            for (; r < e2; ++r) hi |= static_cast<unsigned char>(*r);
                            ascii = !(hi & 0x8080808080808080ull);
                            e = e2;
                        }
                        if (ascii) {
                            uint32_t chr;
                            if (seqids.find_word(key, chr)) {
                                pend[n_pend] = chr, pend[n_pend + 1] = v1, pend[n_pend + 2] = v2;
                                if ((n_pend += 3) == 192) flush();
                            }
                            a = static_cast<size_t>(e - base) + 1;
                            continue;
                        }
                    }
                }
            }
        }
        if (n_pend) flush();
        if (a < z) {
            const char *q = base + a;
            const unsigned char c0 = static_cast<unsigned char>(*q);
            if (c0 != '#' && !kWs.t[c0]) {
                uint64_t h = SeqidTable::kHashSeed;
                unsigned hib = 0;
                const char *n0 = q;
                while (q < lim && !kWs.t[static_cast<unsigned char>(*q)]) {
                    const unsigned char c = static_cast<unsigned char>(*q);
                    h = (h ^ c) * SeqidTable::kHashPrime;
                    hib |= c;
                    ++q;
                }
                const char *n1 = q;
                uint32_t val[2] = {0, 0};
                bool fast = true;
                for (int f = 0; f < 2 && fast; ++f) {
                    while (q < lim && kBlank.t[static_cast<unsigned char>(*q)]) ++q;
                    const char *b0 = q;
                    uint32_t v = 0;
                    while (q < lim) {
                        const unsigned dg = static_cast<unsigned char>(*q) - '0';
                        if (dg > 9) break;
                        v = v * 10 + dg;
                        ++q;
                    }
                    const size_t nd = static_cast<size_t>(q - b0);
                    fast = nd >= 1 && nd <= 9 && (q == lim || kWs.t[static_cast<unsigned char>(*q)]);
                    val[f] = v;
                }
                if (fast) {
                    const char *nlp = q < lim ? static_cast<const char *>(std::memchr(q, '\n', static_cast<size_t>(lim - q))) : nullptr;
                    const char *e = nlp ? nlp : lim;
                    uint64_t hi = hib;
                    for (; q + 8 <= e; q += 8) {
                        uint64_t w;
                        std::memcpy(&w, q, 8);
                        hi |= w;
                    }
                    for (; q < e; ++q) hi |= static_cast<unsigned char>(*q);
                    if (!(hi & 0x8080808080808080ull)) {
                        uint32_t chr;
                        if (seqids.find_hashed(n0, static_cast<size_t>(n1 - n0), h, chr)) {
                            rows.push_back(chr);
                            rows.push_back(val[0]);
                            rows.push_back(val[1]);
                        }
                        a = static_cast<size_t>(e - base) + 1;
                        continue;
                    }
                }
            }
        }
        const char *nlp = a < z ? static_cast<const char *>(std::memchr(base + a, '\n', z - a)) : nullptr;
        const size_t nl = nlp ? static_cast<size_t>(nlp - base) : z;
        const char *p = base + a, *e = base + nl;
        a = nl + 1;
        if (p == e || *p == '#') continue;
        {
            uint64_t hi = 0;
            const char *q = p;
            for (; q + 8 <= e; q += 8) {
                uint64_t w;
                std::memcpy(&w, q, 8);
                hi |= w;
            }
            for (; q < e; ++q) hi |= static_cast<unsigned char>(*q);
            if ((hi & 0x8080808080808080ull) && !utf8_valid(std::string_view(p, static_cast<size_t>(e - p))))
                throw Error("invalid utf-8 sequence in BED line");
        }
        const char *fb[3], *fe[3];
        int nf = 0;
        const char *q = p;
        while (q < e && nf < 3) {
            while (q < e && kWs.t[static_cast<unsigned char>(*q)]) ++q;
            if (q >= e) break;
            fb[nf] = q;
            while (q < e && !kWs.t[static_cast<unsigned char>(*q)]) ++q;
            fe[nf++] = q;
        }
        if (nf < 3) continue;
        uint32_t chr, s, en;
        if (!seqids.find(fb[0], static_cast<size_t>(fe[0] - fb[0]), chr)) continue;
        if (!field_u32(fb[1], fe[1], s) || !field_u32(fb[2], fe[2], en))  // lexical_core::parse::<u32>
            throw Error("lexical parse error: invalid BED coordinate in \"" + std::string(p, static_cast<size_t>(e - p)) + "\"");
        rows.push_back(chr);
        rows.push_back(s);
        rows.push_back(en);
    }
}
}  // namespace

// intersect.rs:201-230.  Rows with an unknown seqid or fewer than three fields are skipped;
// a row whose coordinates do not parse aborts the run; start >= end rows are kept as they are.
void parse_bed_pieces(std::string_view d, size_t a, size_t z, bool last, const SeqidTable &seqid_map, size_t threads,
                      std::vector<std::vector<uint32_t>> &piece, WorkerPool *workers) {
    const std::string_view sub = d.substr(a, z - a);
    // with a pool: four pieces per thread, taken in turn -- the slowest of 64 equal pieces took 1.7x the average (measured)
    const size_t per_thread = workers ? 4 : 1;
    const size_t parts = sub.size() < (1u << 20) ? 1 : std::max<size_t>(1, std::min<size_t>(threads, 64)) * per_thread;
    std::vector<size_t> cut = line_chunks(sub, parts);
    const size_t n = cut.size() - 1;
    piece.resize(n);
    auto work = [&](size_t c) {
        piece[c].clear();
        piece[c].reserve((cut[c + 1] - cut[c]) / 8);
        parse_bed_chunk(d, a + cut[c], a + cut[c + 1], last && c + 1 == n, seqid_map, piece[c]);
    };
    if (!workers) return parallel_for(n, n, work);
    std::vector<std::exception_ptr> err(n);  // (WorkerPool::run's callable must not throw)
    workers->run(n, [&](size_t c) {
        try {
            work(c);
        } catch (...) {
            err[c] = std::current_exception();
        }
    });
    for (size_t c = 0; c < n; ++c)
        if (err[c]) std::rethrow_exception(err[c]);
}

// The file is cut at line starts and parsed on `threads` host threads; rows keep the file's order and the error
// reported is the first one in file order, as in the serial loop of the reference.
std::vector<Region> parse_bed_file(const std::string &bed_path, const std::unordered_map<std::string, uint32_t> &seqid_map,
                                   size_t threads) {
    MappedFile f(bed_path);
    const std::string_view d = f.view();
    std::vector<std::vector<uint32_t>> piece;
    parse_bed_pieces(d, 0, d.size(), true, SeqidTable(seqid_map), threads, piece);
    return regions_of(piece);
}

// The rows of a BED file as the streaming CLI's parser thread produces them -- chunk by chunk (cut at line starts), every
// chunk as four pieces per thread on workers that live as long as the file, row buffers reused from chunk to chunk -- without
// a device: flat (chr, start, end) words in file order.  (Host-side check of that path: tests/test_host_cpu.py.)
std::vector<uint32_t> parse_bed_file_chunked(const std::string &bed_path, const std::unordered_map<std::string, uint32_t> &seqid_map,
                                             size_t threads, size_t chunk_bytes) {
    MappedFile f(bed_path);
    const std::string_view text = f.view();
    const SeqidTable seqids(seqid_map);
    WorkerPool workers(std::min<size_t>(std::max<size_t>(threads, 1), 64) - 1);
    std::vector<std::vector<uint32_t>> piece;  // (reused: keeps its capacity)
    std::vector<uint32_t> rows;
    for_each_line_chunk(text, chunk_bytes, [&](size_t pos, size_t z, bool last) {
        parse_bed_pieces(text, pos, z, last, seqids, threads, piece, &workers);
        for (const auto &v : piece) rows.insert(rows.end(), v.begin(), v.end());
        return true;
    });
    return rows;
}

}  // namespace gffx::commands::intersect
