// intersect_internal.hpp -- shared by the files of `gffx intersect` (bed_parse, shard, join_a_stream, match_lines), not in gffx.hpp
#pragma once
#include <cstdlib>
#include <cstring>

#include "fast_fields.hpp"
#include "gffx.hpp"

namespace gffx::commands::intersect {

// seqid name -> number without a std::string per row: open addressing over FNV-1a of the field bytes (a BED file in random
// order changes seqid on nearly every row; the reference pays a HashMap<String> probe there too, intersect.rs:219)
class SeqidTable {
  public:
    explicit SeqidTable(const std::unordered_map<std::string, uint32_t> &m) {
        size_t cap = 16;
        while (cap < 4 * m.size() + 4) cap <<= 1;
        slot_.assign(cap, Slot{nullptr, 0, 0, 0});
        mask_ = cap - 1;
        for (const auto &kv : m) {
            const uint64_t h = hash(kv.first.data(), kv.first.size());
            size_t i = h & mask_;
            while (slot_[i].p) i = (i + 1) & mask_;
            slot_[i] = Slot{kv.first.data(), static_cast<uint32_t>(kv.first.size()), kv.second, h};
        }
        short_.build(m);
    }
    static uint64_t hash(const char *p, size_t n) {
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<unsigned char>(p[i])) * 1099511628211ull;
        return h;
    }
    static constexpr uint64_t kHashSeed = 1469598103934665603ull, kHashPrime = 1099511628211ull;
    bool find(const char *p, size_t n, uint32_t &id) const { return find_hashed(p, n, hash(p, n), id); }
    // a name of 1-7 bytes given as the word of its bytes (zero above them): parse_bed_chunk's word-at-a-time path
    bool find_word(uint64_t w, uint32_t &id) const { return short_.find(w, id); }
    // h = hash(p, n), computed by the caller while it scanned the field
    bool find_hashed(const char *p, size_t n, uint64_t h, uint32_t &id) const {
        for (size_t i = h & mask_; slot_[i].p; i = (i + 1) & mask_)
            if (slot_[i].h == h && slot_[i].n == n && std::memcmp(slot_[i].p, p, n) == 0) {
                id = slot_[i].id;
                return true;
            }
        return false;
    }

  private:
    struct Slot {
        const char *p;
        uint32_t n, id;
        uint64_t h;
    };
    std::vector<Slot> slot_;
    size_t mask_ = 0;
    ShortNameTable short_;
};

// The rows of d[a, z) parsed on `threads` host threads (cut at line starts); piece[t] = the rows of the t-th cut, in file
// order (vectors that come in with capacity keep it: a streaming caller recycles them).  The error reported is the first one
// in file order, as in the serial loop of the reference.  (bed_parse.cpp)
void parse_bed_pieces(std::string_view d, size_t a, size_t z, bool last, const SeqidTable &seqid_map, size_t threads,
                      std::vector<std::vector<uint32_t>> &piece, WorkerPool *workers = nullptr);

// BED text per streamed chunk (join_a_stream.cpp has the measurements behind the 16 MB).  GFFX_CHUNK_MB (1..1024) overrides
// it for experiments.  GFFX_CHUNK_BYTES (a decimal number, 1..1 << 30; anything else is ignored) gives the size in bytes and goes
// before GFFX_CHUNK_MB: a few hundred bytes put a chunk boundary after every few rows of a small file; results never depend on either.
inline size_t stream_chunk_bytes() {
    if (const char *b = std::getenv("GFFX_CHUNK_BYTES"); b && *b >= '0' && *b <= '9') {  // (strtoull alone takes "-5" and " 7")
        char *end = nullptr;
        const unsigned long long v = std::strtoull(b, &end, 10);
        if (end && !*end && v >= 1 && v <= (1ull << 30)) return static_cast<size_t>(v);
    }
    const char *e = std::getenv("GFFX_CHUNK_MB");
    const long v = e ? std::atol(e) : 0;
    return static_cast<size_t>(v >= 1 && v <= 1024 ? v : 16) << 20;
}
constexpr size_t kMinBedRowBytes = 6;  // a row is at least "a\t1\t2\n"

// The text in chunks of about chunk_bytes that end at a line start (or at the end of the text): fn(pos, end, last) for each,
// in file order, until fn returns false.  An empty text is one empty, last chunk.
template <typename F>
void for_each_line_chunk(std::string_view text, size_t chunk_bytes, F &&fn) {
    chunk_bytes = std::max<size_t>(chunk_bytes, 1);
    size_t pos = 0;
    do {
        size_t z = std::min(text.size(), pos + chunk_bytes);
        if (z < text.size()) {
            const size_t nl = text.find('\n', z);
            z = nl == std::string_view::npos ? text.size() : nl + 1;
        }
        if (!fn(pos, z, z == text.size())) return;
        pos = z;
    } while (pos < text.size());
}

}  // namespace gffx::commands::intersect
