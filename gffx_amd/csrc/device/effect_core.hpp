// effect_core.hpp -- the rules of `gffx effect` for the host (g++) and the device (hipcc): what a single-base
// substitution at base x (1-based) with alternate base ALT does to one transcript whose span contains x.
//
// TRANSCRIPT.  D: its CDS rows ordered by (start, line order), pre the exclusive sums of their lengths, L the total, p the phase
// of the leading segment, C = (L - p) / 3 for L > p (else 0).  E: its exon rows in the same order, or D when it has none; pmax
// the running maximum of the ends, kept for D and for E (each starts anew).  Rows are [start0, end) with start0 = start - 1.
//
// CLASS, the first rule that applies:
//   1 coding      x lies in a row of D; the first such row i is the first with pmax[i] >= x (pmax ascends, and the rows before
//                 it end before x), provided it starts at or before x.  xc = pre[i] + (x - start_i), q = xc on plus and
//                 L - 1 - xc on minus.  q outside [p, p + 3C): partial_codon.  Else c = (q - p) / 3, k = (q - p) % 3; the
//                 reference codon is the bases at transcription positions p + 3c .. p + 3c + 2, each located on its own
//                 (seq::locate_row) and complemented on minus; the alternate codon has byte k replaced by ALT (complemented on
//                 minus); the amino acids (seq::translate) decide among coding_unknown, stop_retained, synonymous, stop_gained,
//                 stop_lost, start_lost and missense.
//   2 exonic      j = the last row of E with start <= x exists and pmax[j] >= x: noncoding_exon without D; before the smallest
//                 CDS start 5_prime_UTR (3_prime_UTR on minus), behind the largest CDS end 3_prime_UTR (5_prime_UTR on minus),
//                 between them noncoding_exon.
//   3 between     no j, or no row j + 1: intron.  Else a = pmax[j] < x < b = start_{j+1}: x <= a + 2 splice_donor
//                 (splice_acceptor on minus), else x >= b - 2 splice_acceptor (splice_donor on minus), else intron.
//
// Plain C++17 (GFFX_HD inline, no allocation, no HIP calls): the same code runs in k_effect_pairs (effect.hip), in the sanitizer
// build of tools/effect_check.cpp and in its timed build, the one-core baseline.
#pragma once
#include <cstdint>

#include "seq_core.hpp"

namespace gffx {
namespace effect {

using seq::u64;

// in the order `--summary` lists them
enum : uint8_t {
    kPartialCodon = 0,
    kCodingUnknown = 1,
    kStopRetained = 2,
    kSynonymous = 3,
    kStopGained = 4,
    kStopLost = 5,
    kStartLost = 6,
    kMissense = 7,
    kNoncodingExon = 8,
    kUtr5 = 9,
    kUtr3 = 10,
    kIntron = 11,
    kSpliceDonor = 12,
    kSpliceAcceptor = 13,
    kIntergenic = 14,
    kClasses = 15
};
GFFX_HD inline const char *class_name(uint32_t cls) {
    switch (cls) {
        case kPartialCodon: return "partial_codon";
        case kCodingUnknown: return "coding_unknown";
        case kStopRetained: return "stop_retained";
        case kSynonymous: return "synonymous";
        case kStopGained: return "stop_gained";
        case kStopLost: return "stop_lost";
        case kStartLost: return "start_lost";
        case kMissense: return "missense";
        case kNoncodingExon: return "noncoding_exon";
        case kUtr5: return "5_prime_UTR";
        case kUtr3: return "3_prime_UTR";
        case kIntron: return "intron";
        case kSpliceDonor: return "splice_donor";
        case kSpliceAcceptor: return "splice_acceptor";
        case kIntergenic: return "intergenic";
        default: return "?";
    }
}
GFFX_HD inline bool is_coding(uint32_t cls) { return cls >= kCodingUnknown && cls <= kMissense; }  // (the four coding columns are filled)

enum : uint32_t { kFlagMinus = 1, kFlagPhase = 6, kFlagDropped = 8 };  // a transcript's flag byte, as seq's rec_flags

// what one (allele, transcript) pair gives: 32 bytes, two 16-byte stores.  Coding classes fill everything; partial_codon q
// only; every other class leaves the coding fields 0.  The codons are the genome's bytes as they are (not case folded).
struct Record {
    u64 q;  // transcription position in the CDS, 0-based (cds_pos = q + 1)
    u64 c;  // codon number, 0-based (aa_pos = c + 1)
    uint32_t transcript;
    uint8_t cls, k, ref_match, aa_ref, aa_alt;
    uint8_t codon_ref[3], codon_alt[3], pad;
};
static_assert(sizeof(Record) == 32, "Record is two 16-byte words");

// the rows of all transcripts, ordered by (transcript, kind, start, input order); kind 0: CDS, 1: exon
struct Rows {
    const uint32_t *start0, *end;  // [start0, end)
    const u64 *pre;                // the exclusive sums of the lengths over ALL rows (only differences inside a D are used)
    const uint32_t *pmax;          // the running maximum of end, anew in every D and every exon run
};
// one kept transcript: 48 bytes, three 16-byte loads
struct Transcript {
    uint32_t d0, d1, e0, e1;  // D = rows [d0, d1), E = rows [e0, e1) (= D when it has no exon row)
    uint32_t cmin, cmax;      // the smallest start (1-based) and largest end of D; undefined for an empty D
    uint32_t flags, seq;      // kFlag*; the sequence number
    u64 L;                    // bases of D
    u64 base;                 // where the sequence begins in the genome's arena
};
static_assert(sizeof(Transcript) == 48, "Transcript is three 16-byte words");

// both searches of a pair side by side (their loads are independent, iteration by iteration):
//   *i = the first row of [d0, d1) with pmax >= x, or d1;  *n_le = e0 + #{rows of [e0, e1) with start0 < x}
GFFX_HD inline void find_rows(const Rows &r, const Transcript &t, uint32_t x, uint32_t *i, uint32_t *n_le) {
    uint32_t a = t.d0, an = t.d1 - t.d0, b = t.e0, bn = t.e1 - t.e0;
    while (an | bn) {
        const uint32_t ha = an >> 1, hb = bn >> 1;
        const uint32_t va = an ? r.pmax[a + ha] : 0u, vb = bn ? r.start0[b + hb] : 0u;
        if (an) {
            if (va < x) a += ha + 1, an -= ha + 1;
            else an = ha;
        }
        if (bn) {
            if (vb < x) b += hb + 1, bn -= hb + 1;
            else bn = hb;
        }
    }
    *i = a, *n_le = b;
}

// rule 1's amino acid test
GFFX_HD inline uint8_t coding_class(uint8_t aa_ref, uint8_t aa_alt, u64 c, uint32_t p) {
    if (aa_ref == 'X' || aa_alt == 'X') return kCodingUnknown;
    if (aa_ref == aa_alt) return aa_ref == '*' ? kStopRetained : kSynonymous;
    if (aa_alt == '*') return kStopGained;
    if (aa_ref == '*') return kStopLost;
    if (c == 0 && p == 0 && aa_ref == 'M') return kStartLost;
    return kMissense;
}

// rules 2 and 3 for an x outside D: n_le as find_rows gives it
GFFX_HD inline uint8_t noncoding_class(const Rows &r, const Transcript &t, uint32_t x, uint32_t n_le) {
    const bool minus = t.flags & kFlagMinus;
    if (n_le > t.e0 && r.pmax[n_le - 1] >= x) {
        if (t.d0 == t.d1) return kNoncodingExon;
        if (x < t.cmin) return minus ? kUtr3 : kUtr5;
        if (x > t.cmax) return minus ? kUtr5 : kUtr3;
        return kNoncodingExon;
    }
    if (n_le == t.e0 || n_le == t.e1) return kIntron;
    const u64 a = r.pmax[n_le - 1], b = (u64)r.start0[n_le] + 1;  // a < x < b
    if (x <= a + 2) return minus ? kSpliceAcceptor : kSpliceDonor;
    if ((u64)x + 2 >= b) return minus ? kSpliceDonor : kSpliceAcceptor;
    return kIntron;
}

// the pair (x, alt) against transcript t, whose span contains x.  bases: the genome's arena.  transcript and ref_match are
// the caller's.
GFFX_HD inline Record classify(const Rows &r, const Transcript &t, const uint8_t *bases, uint32_t x, uint8_t alt) {
    Record o{};
    uint32_t i, n_le;
    find_rows(r, t, x, &i, &n_le);
    if (!(i < t.d1 && r.start0[i] < x)) {
        o.cls = noncoding_class(r, t, x, n_le);
        return o;
    }
    const bool minus = t.flags & kFlagMinus;
    const uint32_t p = (t.flags & kFlagPhase) >> 1;
    const u64 pre0 = r.pre[t.d0], lo = r.pre[i] - pre0, hi = r.pre[i + 1] - pre0;  // row i holds [lo, hi) of the concatenation
    const u64 xc = lo + (x - 1 - r.start0[i]);
    const u64 q = minus ? t.L - 1 - xc : xc;
    const u64 C = t.L > p ? (t.L - p) / 3 : 0;
    o.q = q;
    if (q < p || q >= p + 3 * C) {
        o.cls = kPartialCodon;
        return o;
    }
    const u64 c = (q - p) / 3;
    const uint32_t k = (uint32_t)((q - p) % 3);
    // where the three bases lie: in row i as a rule, else each by a search of its own
    u64 at[3];
    for (uint32_t m = 0; m < 3; ++m) {
        const u64 qm = p + 3 * c + m, xm = minus ? t.L - 1 - qm : qm;
        if (xm >= lo && xm < hi) {
            at[m] = (u64)r.start0[i] + (xm - lo);
        } else {
            const u64 row = seq::locate_row(r.pre, t.d0, t.d1, xm);
            at[m] = (u64)r.start0[row] + (xm - (r.pre[row] - pre0));
        }
    }
    const uint8_t g0 = bases[t.base + at[0]], g1 = bases[t.base + at[1]], g2 = bases[t.base + at[2]];  // three independent loads
    o.codon_ref[0] = minus ? seq::complement(g0) : g0;
    o.codon_ref[1] = minus ? seq::complement(g1) : g1;
    o.codon_ref[2] = minus ? seq::complement(g2) : g2;
    for (uint32_t m = 0; m < 3; ++m) o.codon_alt[m] = m == k ? (minus ? seq::complement(alt) : alt) : o.codon_ref[m];
    o.aa_ref = seq::translate(o.codon_ref[0], o.codon_ref[1], o.codon_ref[2]);
    o.aa_alt = seq::translate(o.codon_alt[0], o.codon_alt[1], o.codon_alt[2]);
    o.c = c;
    o.k = (uint8_t)k;
    o.cls = coding_class(o.aa_ref, o.aa_alt, c, p);
    return o;
}

// 1 when REF, case folded, is the genome's base, case folded (REF is a letter: no other byte folds onto one)
GFFX_HD inline uint8_t ref_match(uint8_t ref, uint8_t genome_base) { return (ref & 0xDFu) == (genome_base & 0xDFu) ? 1 : 0; }

// ---- what the build does per transcript, once: rows [f0, f2) are its own, [f0, f1) of kind 0.  Writes pmax for its rows and
// fills t (flags and base are the caller's); returns false for a transcript that cannot be kept: a member on another sequence
// than the first row's, on a sequence the genome lacks, or beyond its end.  *lo0 / *hi: the span [lo0, hi).
GFFX_HD inline bool build_transcript(const uint32_t *start0, const uint32_t *end, const uint32_t *row_seq, const u64 *pre, uint32_t *pmax, uint32_t f0, uint32_t f1,
                                     uint32_t f2, const uint32_t *seq_len, uint32_t n_seq, Transcript *t, uint32_t *lo0, uint32_t *hi) {
    bool ok = true;
    uint32_t lo = 0xFFFFFFFFu, top = 0;
    const uint32_t sq = row_seq[f0];
    for (uint32_t part = 0; part < 2; ++part) {
        uint32_t run = 0;
        for (uint32_t j = part ? f1 : f0; j < (part ? f2 : f1); ++j) {
            run = end[j] > run ? end[j] : run;
            pmax[j] = run;
            lo = start0[j] < lo ? start0[j] : lo;
            ok = ok && row_seq[j] == sq;
        }
        top = run > top ? run : top;
    }
    ok = ok && sq < n_seq && top <= seq_len[sq];
    t->d0 = f0, t->d1 = f1;
    t->e0 = f1 < f2 ? f1 : f0, t->e1 = f1 < f2 ? f2 : f1;
    t->cmin = f0 < f1 ? start0[f0] + 1 : 0, t->cmax = f0 < f1 ? pmax[f1 - 1] : 0;
    t->seq = sq;
    t->L = pre[f1] - pre[f0];
    *lo0 = lo, *hi = top;
    return ok;
}

}  // namespace effect
}  // namespace gffx
