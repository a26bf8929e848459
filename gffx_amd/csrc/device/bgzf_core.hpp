// bgzf_core.hpp -- one DEFLATE (RFC 1951) / BGZF / BAM-record decoder for the host (g++) and the device (hipcc).
//
// A BAM file is BGZF: gzip members (RFC 1952) of at most 64 KiB of output, each an independent raw-DEFLATE stream, whose
// FEXTRA field carries the subfield `BC` = BSIZE (the member's total length - 1); an empty member (the 28-byte EOF marker)
// ends the file.  The decompressed stream is the BAM header, then records `int32 block_size` + block_size bytes (SAM spec
// §4.2).  Everything here is plain C++17 on flat byte pointers, so the same code inflates on the host (the BAM header, the
// sanitizer build of tools/bgzf_check.cpp) and in k_bgzf_inflate (bgzf.hip).
//
// The input is untrusted and the device must never fault on it: every input read is bounded by the member's length, every
// output write by the output capacity (ISIZE, at most 65536), every loop by the input or the output, and failures come back
// as a Status -- nothing asserts, aborts or traps on a condition the input decides.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GFFX_HD __host__ __device__
#else
#define GFFX_HD
#endif

namespace gffx {
namespace bgzf {

enum Status : int {
    kOk = 0,
    kTruncated = 1,  // the input ends inside a member / a DEFLATE stream
    kHeader = 2,     // not a BGZF member header (ID1/ID2/CM/FLG, no BC subfield)
    kBsize = 3,      // BSIZE too small for a header and a footer
    kBtype = 4,      // DEFLATE block type 3
    kStored = 5,     // stored block with NLEN != ~LEN
    kCodes = 6,      // over-subscribed or incomplete code-length set, bad repeat, no end-of-block code
    kSymbol = 7,     // a code that is not in the table, or length / distance symbol out of range
    kDistance = 8,   // a distance reaching before the start of the member's output
    kOverflow = 9,   // more output than the capacity (ISIZE)
    kIsize = 10,     // output length != ISIZE, or ISIZE > 65536
    kCrc = 11,       // CRC32 of the output != the footer's
    kTrailing = 12,  // the DEFLATE stream ends before the member's footer
};

GFFX_HD inline const char *status_name(int s) {
    switch (s) {
        case kOk: return "ok";
        case kTruncated: return "truncated member";
        case kHeader: return "not a BGZF member header";
        case kBsize: return "bad BSIZE";
        case kBtype: return "invalid DEFLATE block type 3";
        case kStored: return "stored block length check failed";
        case kCodes: return "invalid Huffman code lengths";
        case kSymbol: return "invalid Huffman code or symbol";
        case kDistance: return "distance too far back";
        case kOverflow: return "output exceeds ISIZE";
        case kIsize: return "ISIZE mismatch";
        case kCrc: return "CRC32 mismatch";
        case kTrailing: return "DEFLATE stream shorter than the member";
        default: return "unknown status";
    }
}

constexpr uint32_t kMaxIsize = 65536;
constexpr uint32_t kMaxSym = 288;
constexpr int kFastBits = 9;

GFFX_HD inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
GFFX_HD inline uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ---- member header ------------------------------------------------------------------------------------------------------
// p: the member's first byte, avail: bytes from p to the end of the input.  On kOk *total = BSIZE + 1 (the member's length,
// header and footer included) and *hdr = 12 + XLEN (where the DEFLATE stream begins); total <= avail is checked.
GFFX_HD inline int member_header(const uint8_t *p, uint64_t avail, uint32_t *total, uint32_t *hdr) {
    if (avail < 12) return kTruncated;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4) || (p[3] & ~5u)) return kHeader;  // FEXTRA; FTEXT tolerated
    const uint32_t xlen = le16(p + 10);
    if (12ull + xlen > avail) return kTruncated;
    uint32_t off = 12, bsize = 0;
    bool found = false;
    while (off + 4 <= 12 + xlen) {  // subfields: SI1 SI2 SLEN data (each step advances by >= 4)
        const uint32_t slen = le16(p + off + 2);
        if (off + 4 + slen > 12 + xlen) return kHeader;
        if (p[off] == 'B' && p[off + 1] == 'C' && slen == 2) {
            bsize = le16(p + off + 4);
            found = true;
        }
        off += 4 + slen;
    }
    if (!found) return kHeader;
    if (bsize + 1 < 12 + xlen + 8) return kBsize;
    if (bsize + 1ull > avail) return kTruncated;
    *total = bsize + 1;
    *hdr = 12 + xlen;
    return kOk;
}

// ---- CRC32 (reflected, polynomial 0xEDB88320) ---------------------------------------------------------------------------
GFFX_HD inline uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    return c;
}
// the raw register update: crc32(data) = raw(0xFFFFFFFF, data) ^ 0xFFFFFFFF
GFFX_HD inline uint32_t crc_raw(const uint32_t *table, uint32_t c, const uint8_t *p, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c;
}
// GF(2) polynomials mod P in the reflected bit order (bit 31 = x^0): a * b mod P
GFFX_HD inline uint32_t gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(8 n) mod P: the operator that moves a raw register over n zero bytes.  raw(c, A || B) = shift(c', |B|) ^ raw(0, B) with
// c' = raw(c, A), so stripes whose registers started at 0 combine with one multiplication each.
GFFX_HD inline uint32_t x8n_mod_p(uint64_t n) {
    uint32_t p = 0x80000000u, sq = 0x00800000u;  // x^0; x^8
    while (n) {
        if (n & 1) p = gf2_mul(sq, p);
        sq = gf2_mul(sq, sq);
        n >>= 1;
    }
    return p;
}

// ---- DEFLATE ------------------------------------------------------------------------------------------------------------
// Canonical Huffman code: count[len] codes per length, symbols in canonical order, and a fast table over the next
// kFastBits input bits (entry = len << 9 | symbol; 0 = the code is longer than kFastBits, take the canonical walk).
struct Huff {
    uint16_t count[16];
    uint16_t symbol[kMaxSym];
    uint16_t fast[1 << kFastBits];
};
struct Scratch {
    Huff lit, dist;
    uint16_t lengths[320];
};

// Builds h from n code lengths (0..15).  Returns < 0 over-subscribed, 0 complete, > 0 incomplete (codes left over).
GFFX_HD inline int huff_build(Huff *h, const uint16_t *length, int n) {
    for (int l = 0; l < 16; ++l) h->count[l] = 0;
    for (int s = 0; s < n; ++s) h->count[length[s]]++;
    for (int i = 0; i < (1 << kFastBits); ++i) h->fast[i] = 0;
    if (h->count[0] == n) return 0;  // no codes: complete, every decode fails
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h->count[l];
        if (left < 0) return left;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h->count[l]);
    for (int s = 0; s < n; ++s)
        if (length[s]) h->symbol[offs[length[s]]++] = (uint16_t)s;
    // fast table: walk the canonical codes in order, reversed into input bit order
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= kFastBits; ++l) {
        for (int k = 0; k < h->count[l]; ++k, ++idx, ++code) {
            uint32_t r = 0;
            for (int b = 0; b < l; ++b) r |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t f = r; f < (1u << kFastBits); f += 1u << l) h->fast[f] = (uint16_t)((l << 9) | h->symbol[idx]);
        }
        code <<= 1;
    }
    return left;
}

// LSB-first bit reader.  Past the end it feeds zero bytes and counts them; over() tells whether bits beyond the input were
// consumed (the stream is truncated), which every loop checks, so no loop outlives its input.
struct Bits {
    const uint8_t *in;
    uint32_t n, pos;  // pos: bytes loaded, including the virtual zero bytes past n
    uint64_t buf;
    uint32_t cnt;
    GFFX_HD void fill(uint32_t k) {
        while (cnt < k) {
            buf |= (uint64_t)(pos < n ? in[pos] : 0) << cnt;
            ++pos;
            cnt += 8;
        }
    }
    GFFX_HD uint32_t peek(uint32_t k) {
        fill(k);
        return (uint32_t)(buf & ((1ull << k) - 1));
    }
    GFFX_HD void drop(uint32_t k) {
        buf >>= k;
        cnt -= k;
    }
    GFFX_HD uint32_t get(uint32_t k) {
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    GFFX_HD bool over() const { return (uint64_t)pos * 8 - cnt > (uint64_t)n * 8; }
};

// the next symbol of h, or -1 (no such code)
GFFX_HD inline int huff_decode(Bits &br, const Huff *h) {
    const uint32_t f = h->fast[br.peek(kFastBits)];
    if (f) {
        br.drop(f >> 9);
        return (int)(f & 0x1FF);
    }
    br.fill(15);
    int code = 0, first = 0, index = 0;
    uint64_t bits = br.buf;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int count = h->count[l];
        if (code - count < first) {
            br.drop((uint32_t)l);
            return h->symbol[index + (code - first)];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

GFFX_HD inline int length_base(int s) {  // s = symbol - 257, 0..28
    const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    return base[s];
}
GFFX_HD inline int length_extra(int s) { return (s < 8 || s == 28) ? 0 : (s - 4) >> 2; }
GFFX_HD inline int dist_base(int s) {  // 0..29
    const uint16_t base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    return base[s];
}
GFFX_HD inline int dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }

// One Huffman-coded block into out[*o, cap).
GFFX_HD inline int inflate_codes(Bits &br, const Huff *lit, const Huff *dist, uint8_t *out, uint32_t cap, uint32_t *o) {
    uint32_t w = *o;
    for (;;) {  // each pass writes >= 1 byte (bounded by cap) or ends the block
        if (br.over()) return kTruncated;
        const int sym = huff_decode(br, lit);
        if (sym < 0) return br.over() ? kTruncated : kSymbol;
        if (sym < 256) {
            if (w >= cap) return kOverflow;
            out[w++] = (uint8_t)sym;
        } else if (sym == 256) {
            *o = w;
            return br.over() ? kTruncated : kOk;
        } else {
            const int ls = sym - 257;
            if (ls >= 29) return kSymbol;
            const uint32_t len = (uint32_t)length_base(ls) + br.get((uint32_t)length_extra(ls));
            const int ds = huff_decode(br, dist);
            if (ds < 0) return br.over() ? kTruncated : kSymbol;
            if (ds >= 30) return kSymbol;
            const uint32_t d = (uint32_t)dist_base(ds) + br.get((uint32_t)dist_extra(ds));
            if (br.over()) return kTruncated;
            if (d > w) return kDistance;
            if (len > cap - w) return kOverflow;
            for (uint32_t k = 0; k < len; ++k, ++w) out[w] = out[w - d];
        }
    }
}

GFFX_HD inline int fixed_tables(Scratch *s) {
    for (int i = 0; i < 144; ++i) s->lengths[i] = 8;
    for (int i = 144; i < 256; ++i) s->lengths[i] = 9;
    for (int i = 256; i < 280; ++i) s->lengths[i] = 7;
    for (int i = 280; i < 288; ++i) s->lengths[i] = 8;
    huff_build(&s->lit, s->lengths, 288);
    for (int i = 0; i < 30; ++i) s->lengths[i] = 5;
    huff_build(&s->dist, s->lengths, 30);
    return kOk;
}

GFFX_HD inline int dynamic_tables(Bits &br, Scratch *s) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int nlen = (int)br.get(5) + 257, ndist = (int)br.get(5) + 1, ncode = (int)br.get(4) + 4;
    if (nlen > 286 || ndist > 30) return kCodes;
    for (int i = 0; i < 19; ++i) s->lengths[order[i]] = 0;
    for (int i = 0; i < ncode; ++i) s->lengths[order[i]] = (uint16_t)br.get(3);
    if (br.over()) return kTruncated;
    if (huff_build(&s->lit, s->lengths, 19) != 0) return kCodes;  // the code-length code must be complete
    int i = 0;
    while (i < nlen + ndist) {  // each pass fills >= 1 length
        if (br.over()) return kTruncated;
        int sym = huff_decode(br, &s->lit);
        if (sym < 0) return br.over() ? kTruncated : kCodes;
        if (sym < 16) {
            s->lengths[i++] = (uint16_t)sym;
            continue;
        }
        uint16_t len = 0;
        int rep;
        if (sym == 16) {
            if (i == 0) return kCodes;
            len = s->lengths[i - 1];
            rep = 3 + (int)br.get(2);
        } else if (sym == 17) {
            rep = 3 + (int)br.get(3);
        } else {
            rep = 11 + (int)br.get(7);
        }
        if (i + rep > nlen + ndist) return kCodes;
        while (rep--) s->lengths[i++] = len;
    }
    if (br.over()) return kTruncated;
    if (s->lengths[256] == 0) return kCodes;  // no end-of-block code
    // an incomplete code is only allowed when it is a single code of length 1 (zlib's inflate_table: max length 1)
    int err = huff_build(&s->lit, s->lengths, nlen);
    if (err < 0 || (err > 0 && !(s->lit.count[1] == 1 && nlen - s->lit.count[0] == 1))) return kCodes;
    err = huff_build(&s->dist, s->lengths + nlen, ndist);
    if (err < 0 || (err > 0 && !(s->dist.count[1] == 1 && ndist - s->dist.count[0] == 1))) return kCodes;
    return kOk;
}

// Raw DEFLATE in[0, n) -> out[0, cap).  *produced = bytes written, *used = input bytes consumed (whole bytes).
GFFX_HD inline int inflate_raw(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *produced, uint32_t *used,
                               Scratch *s) {
    Bits br{in, n, 0, 0, 0};
    uint32_t o = 0;
    int last = 0;
    while (!last) {  // each block consumes >= 3 bits (bounded by the input through over())
        last = (int)br.get(1);
        const uint32_t type = br.get(2);
        if (br.over()) return kTruncated;
        int st;
        if (type == 0) {
            br.drop(br.cnt & 7);  // to a byte boundary; the whole bytes still buffered go back to the input
            uint32_t at = br.pos - br.cnt / 8;
            br.buf = 0;
            br.cnt = 0;
            if (at + 4 > n) return kTruncated;
            const uint32_t len = le16(in + at), nlen = le16(in + at + 2);
            if ((len ^ 0xFFFFu) != nlen) return kStored;
            at += 4;
            if (len > n - at) return kTruncated;
            if (len > cap - o) return kOverflow;
            for (uint32_t k = 0; k < len; ++k) out[o + k] = in[at + k];
            o += len;
            br.pos = at + len;
            st = kOk;
        } else if (type == 1) {
            fixed_tables(s);
            st = inflate_codes(br, &s->lit, &s->dist, out, cap, &o);
        } else if (type == 2) {
            st = dynamic_tables(br, s);
            if (st == kOk) st = inflate_codes(br, &s->lit, &s->dist, out, cap, &o);
        } else {
            return kBtype;
        }
        if (st != kOk) return st;
    }
    *produced = o;
    *used = br.pos - br.cnt / 8;
    return kOk;
}

// One BGZF member at p (avail bytes from p to the end of the input) into out (cap >= ISIZE, at most 65536 needed).
// *total = the member's length, *isize = its output length.  crc_table == nullptr skips the CRC check (the device
// checks it with the whole wave).
GFFX_HD inline int member_inflate(const uint8_t *p, uint64_t avail, uint8_t *out, uint32_t cap, uint32_t *total, uint32_t *isize,
                                  Scratch *s, const uint32_t *crc_table) {
    uint32_t t = 0, h = 0;
    int st = member_header(p, avail, &t, &h);
    if (st != kOk) return st;
    *total = t;
    const uint32_t want = le32(p + t - 4), crc = le32(p + t - 8);
    if (want > kMaxIsize || want > cap) return kIsize;
    uint32_t got = 0, used = 0;
    st = inflate_raw(p + h, t - h - 8, out, want, &got, &used, s);
    if (st == kOverflow) return kIsize;
    if (st != kOk) return st;
    if (got != want) return kIsize;
    if (used != t - h - 8) return kTrailing;
    *isize = got;
    if (crc_table && (crc_raw(crc_table, 0xFFFFFFFFu, out, got) ^ 0xFFFFFFFFu) != crc) return kCrc;
    return kOk;
}

// ---- BAM header (SAM spec §4.2) ------------------------------------------------------------------------------------------
// magic "BAM\1", l_text, text, n_ref, then n_ref x (l_name, name incl. NUL, l_ref).  d[0, n): the decompressed stream so
// far.  kOk: *bytes = the header's size (records begin there), *n_ref.  kTruncated: more of the stream is needed.
// kHeader: not a BAM header.
inline int bam_header_size(const uint8_t *d, uint64_t n, uint64_t *bytes, uint32_t *n_ref) {
    if (n < 4) return kTruncated;
    if (d[0] != 'B' || d[1] != 'A' || d[2] != 'M' || d[3] != 1) return kHeader;
    if (n < 8) return kTruncated;
    const int32_t l_text = (int32_t)le32(d + 4);
    if (l_text < 0) return kHeader;
    uint64_t at = 8 + (uint64_t)l_text;
    if (n < at + 4) return kTruncated;
    const int32_t nr = (int32_t)le32(d + at);
    if (nr < 0) return kHeader;
    at += 4;
    for (int32_t r = 0; r < nr; ++r) {  // each step advances by >= 8 bytes or returns
        if (n < at + 4) return kTruncated;
        const int32_t l_name = (int32_t)le32(d + at);
        if (l_name < 1) return kHeader;
        at += 8 + (uint64_t)l_name;
        if (n < at) return kTruncated;
    }
    *bytes = at;
    *n_ref = (uint32_t)nr;
    return kOk;
}

enum RecordStatus : int { kKeep = 0, kSkip = 1, kMalformed = 2 };  // bam_record(); kMalformed from frame_fix too

// ---- record framing ------------------------------------------------------------------------------------------------------
// D[0, N): a decompressed stream cut into segments seg[s] .. seg[s + 1] (s < n_seg; seg[0] = 0, seg[n_seg] = N): the carry
// (the unfinished record of the previous chunk) and then one segment per member.  Records are `int32 block_size` + that many
// bytes.  The device runs frame_guess for every segment in parallel (k_frame_guess) and frame_fix on one thread (k_frame_fix).
typedef unsigned long long u64;
constexpr u64 kNoChain = ~0ull;

// The chain on the guess that a record starts at the segment's first byte.  *end: the first record start at or past hi, or
// the start of the record that does not end inside D; kNoChain when the chain meets a block_size < 32.  *n: complete records
// that start in [lo, hi).  Each step advances by >= 36 bytes.
GFFX_HD inline void frame_guess(const uint8_t *D, u64 N, u64 lo, u64 hi, u64 *end, uint32_t *n) {
    u64 p = lo;
    uint32_t c = 0;
    while (p < hi) {
        if (p + 4 > N) break;
        const int32_t bs = (int32_t)le32(D + p);
        if (bs < 32) {
            p = kNoChain;
            break;
        }
        if (p + 4 + (u64)bs > N) break;
        p += 4 + (u64)bs;
        ++c;
    }
    *end = p;
    *n = c;
}

// The true chain from `start` (a known record start: the header's end or the carry's start), proven segment by segment:
// segment s's guess holds iff the true chain reaches seg[s] exactly; where it does not (records spanning members), the chain
// is walked here until it aligns with a segment start again.  entry[s] / count[s]: the first record start in segment s and
// the complete records starting there.  *tail: where the unfinished record begins (N when none).  kMalformed: a record with
// block_size < 32 at *err_off.
GFFX_HD inline int frame_fix(const uint8_t *D, u64 N, const u64 *seg, uint32_t n_seg, u64 start, const u64 *guess_end,
                             const uint32_t *guess_n, u64 *entry, uint32_t *count, u64 *tail, u64 *err_off) {
    u64 cur = start;
    bool stuck = false;  // cur is the start of a record that does not end inside D
    for (uint32_t s = 0; s < n_seg; ++s) {
        const u64 lo = seg[s], hi = seg[s + 1];
        entry[s] = cur;
        count[s] = 0;
        if (stuck || cur >= hi) continue;
        if (cur == lo && guess_end[s] != kNoChain) {
            count[s] = guess_n[s];
            cur = guess_end[s];
            stuck = cur < hi;
            continue;
        }
        uint32_t c = 0;
        while (cur < hi) {
            if (cur + 4 > N) {
                stuck = true;
                break;
            }
            const int32_t bs = (int32_t)le32(D + cur);
            if (bs < 32) {
                for (; s < n_seg; ++s) count[s] = 0;
                *err_off = cur;
                *tail = cur;
                return kMalformed;
            }
            if (cur + 4 + (u64)bs > N) {
                stuck = true;
                break;
            }
            cur += 4 + (u64)bs;
            ++c;
        }
        count[s] = c;
    }
    *tail = cur;
    return kOk;
}

// ---- BAM records (SAM spec §4.2.1) ---------------------------------------------------------------------------------------
//   0 block_size  4 refID  8 pos  12 l_read_name  13 mapq  14 bin  16 n_cigar_op  18 flag  20 l_seq  24 next_refID
//   28 next_pos  32 tlen  36 read_name[l_read_name]  cigar[n_cigar_op] (u32: len << 4 | op) ...
// Fields are read byte by byte: records are not 4-byte aligned.
struct Row {
    int32_t tid;
    uint32_t start, end;
    uint16_t flag;
};

// rec: the record's block_size field, with 4 + block_size bytes readable (framing checked that).  n_ref bounds tid.
// kKeep: *row is the (tid, start, end) the reference pushes (depth.rs:335-364, coverage.rs:157-168) before the tid -> seqid
// mapping.  kSkip: unmapped (flag 0x4), tid < 0 or pos < 0.  kMalformed: what htslib's bam_read1 / sam_read1 reject
// (block_size < 32, l_read_name == 0, read name + CIGAR beyond the record, refID outside [-1, n_ref)).
//
// ASSUMPTION (restated from memory of htslib's sam.c, whose source is not at hand): the end is bam_endpos() --
//   rlen = sum of the lengths of the CIGAR ops that consume the reference, M/D/N/=/X (op 0, 2, 3, 7, 8);
//   a reference length of 0 (no CIGAR, or only I/S/H/P) becomes 1;  end = pos + rlen.
// The long-CIGAR placeholder kSmN (real CIGAR in a CG tag) needs nothing special: its N op carries the reference length.
GFFX_HD inline int bam_record(const uint8_t *rec, uint32_t n_ref, Row *row) {
    const int32_t block_size = (int32_t)le32(rec);
    if (block_size < 32) return kMalformed;
    const uint32_t l_name = rec[12], n_cigar = le16(rec + 16);
    if (l_name == 0 || 32ull + l_name + 4ull * n_cigar > (uint32_t)block_size) return kMalformed;
    const int32_t tid = (int32_t)le32(rec + 4), pos = (int32_t)le32(rec + 8);
    const uint32_t flag = le16(rec + 18);
    if (tid < -1 || (tid >= 0 && (uint32_t)tid >= n_ref)) return kMalformed;
    row->tid = tid;
    row->flag = (uint16_t)flag;
    if ((flag & 0x4) || tid < 0 || pos < 0) return kSkip;
    const uint8_t *cig = rec + 36 + l_name;
    int64_t rlen = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t v = le32(cig + 4 * k), op = v & 0xF;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += v >> 4;
    }
    if (rlen == 0) rlen = 1;
    const int64_t end = (int64_t)pos + rlen;
    if (end <= pos) return kSkip;
    row->start = (uint32_t)pos;
    row->end = end > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)end;
    return kKeep;
}

}  // namespace bgzf
}  // namespace gffx
