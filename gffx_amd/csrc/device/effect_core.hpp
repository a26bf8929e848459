// effect_core.hpp -- the rules of `gffx effect` for the host (g++) and the device (hipcc): what a single-base
// substitution at base x (1-based) with alternate base ALT does to one transcript whose span contains x.  (What an insertion,
// a deletion or a multi-base substitution does, `--indels`, is classify_any further down)
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
    kClasses = 15,  // what the flagless command lists
    // --indels only (26.4), behind the 15 of the flagless path
    kFrameshift = 15,
    kInframeInsertion = 16,
    kInframeDeletion = 17,
    kTranscriptAblation = 18,
    kUnclassifiedModel = 19,
    kClassesAll = 20
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
        case kFrameshift: return "frameshift";
        case kInframeInsertion: return "inframe_insertion";
        case kInframeDeletion: return "inframe_deletion";
        case kTranscriptAblation: return "transcript_ablation";
        case kUnclassifiedModel: return "unclassified_model";
        default: return "?";
    }
}
GFFX_HD inline bool is_coding(uint32_t cls) { return cls >= kCodingUnknown && cls <= kMissense; }  // (the four coding columns are filled)

enum : uint32_t { kFlagMinus = 1, kFlagPhase = 6, kFlagDropped = 8 };  // a transcript's flag byte, as seq's rec_flags
// set by build_transcript, never by the caller: two rows of D or two rows of E overlap (touching rows do not).  Only classify_any
// reads it.
enum : uint32_t { kFlagOverlap = 16 };

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

// ---- --indels: an allele that covers an interval and carries inserted bytes.  After trimming, R' has d bases from
// x0 on and A' has m bytes (ins).  The footprint F is [x0, x0 + d - 1] for d > 0 and the two flanking bases [x0 - 1, x0] for
// d == 0; F' = [lo, hi] is F clipped to the span.  F' HITS a set of bases W when it meets W (d > 0) or lies inside W (d == 0).
// The first rule that applies:
//   0 unclassified_model   rows of D or of E overlap (kFlagOverlap): prefix sums cannot count an interval's bases then
//   1 transcript_ablation  d > 0 and F holds the whole span
//   2 splice               of the donor / acceptor windows (two bases at either end of every gap between E rows, fewer in a gap
//                          of fewer) that F' hits the one with the smallest first base, the left one on a tie
//   3 coding               F' hits D.  pos(x) = D bases below x; qa = pos(lo) for d > 0 and pos(x0) for d == 0 (where the bytes
//                          go in); dc = D bases in F' (d > 0; else 0); [ta, tb) is the run in transcription order.  Then
//                          partial_codon, start_lost, frameshift, or the windows of 3d (classify_any below)
//   4 exonic               F' hits E: rule 2 of the SNV at the smallest base of F' in E
//   5 intron
// With disjoint rows every count is one binary search over start0 and one difference of pre.

// the bases of rows [f0, ..) below x (1-based, x >= 1): n_lt = f0 + #{rows with start0 < x}, as count_starts gives it
GFFX_HD inline u64 bases_below(const Rows &r, uint32_t f0, uint32_t n_lt, u64 x) {
    if (n_lt == f0) return 0;
    const uint32_t j = n_lt - 1;
    const u64 e = r.end[j], cut = e < x - 1 ? e : x - 1;  // (start0[j] <= x - 1)
    return r.pre[j] - r.pre[f0] + (cut - r.start0[j]);
}

// four searches side by side, their loads independent iteration by iteration: out[l] = first + #{rows with start0 < key[l]},
// lanes 0 and 1 over D, lanes 2 and 3 over E
GFFX_HD inline void count_starts(const Rows &r, const Transcript &t, const u64 (&key)[4], uint32_t (&out)[4]) {
    uint32_t at[4] = {t.d0, t.d0, t.e0, t.e0};
    uint32_t n[4] = {t.d1 - t.d0, t.d1 - t.d0, t.e1 - t.e0, t.e1 - t.e0};
    while (n[0] | n[1] | n[2] | n[3]) {
        uint32_t v[4];
        for (int l = 0; l < 4; ++l) v[l] = n[l] ? r.start0[at[l] + (n[l] >> 1)] : 0u;
        for (int l = 0; l < 4; ++l) {
            const uint32_t h = n[l] >> 1;
            if (n[l]) {
                if (v[l] < key[l]) at[l] += h + 1, n[l] -= h + 1;
                else n[l] = h;
            }
        }
    }
    for (int l = 0; l < 4; ++l) out[l] = at[l];
}

// rule 2 for F' = [lo, hi]: the gap between E rows r - 1 and r that can hold the first window hit is the first one with bases
// that ends at or behind lo (every earlier window ends before lo; were a later one hit, this gap's right window would be too).
// n_lo = e0 + #{E rows with start0 < lo}.  Touching rows have no gap: start0 - pre ascends by the gaps' lengths, so the first
// row behind a chain of them is one more search.  Returns kIntron for "no window is hit".
GFFX_HD inline uint8_t splice_class(const Rows &r, const Transcript &t, u64 lo, u64 hi, bool inside, uint32_t n_lo) {
    uint32_t g = n_lo > t.e0 + 1 ? n_lo : t.e0 + 1;
    if (g >= t.e1) return kIntron;
    if (r.start0[g] == r.end[g - 1]) {  // (rare: a chain of touching rows)
        const u64 pre0 = r.pre[t.e0], f = (u64)r.start0[g - 1] - (r.pre[g - 1] - pre0);
        uint32_t at = g, n = t.e1 - g;
        while (n) {
            const uint32_t h = n >> 1;
            if ((u64)r.start0[at + h] - (r.pre[at + h] - pre0) <= f) at += h + 1, n -= h + 1;
            else n = h;
        }
        g = at;
        if (g >= t.e1) return kIntron;
    }
    const bool minus = t.flags & kFlagMinus;
    const u64 a = r.end[g - 1], b = (u64)r.start0[g] + 1;  // the gap's bases: a + 1 .. b - 1
    const u64 l0 = a + 1, l1 = a + 2 < b - 1 ? a + 2 : b - 1, r0 = b - 2 > a + 1 ? b - 2 : a + 1, r1 = b - 1;
    if (inside ? (l0 <= lo && hi <= l1) : (l0 <= hi && lo <= l1)) return minus ? kSpliceAcceptor : kSpliceDonor;
    if (inside ? (r0 <= lo && hi <= r1) : (r0 <= hi && lo <= r1)) return minus ? kSpliceDonor : kSpliceAcceptor;
    return kIntron;
}

// the byte at transcription position tq of the CDS (located on its own, complemented on minus)
GFFX_HD inline u64 cds_at(const Rows &r, const Transcript &t, u64 tq) {
    const u64 xm = (t.flags & kFlagMinus) ? t.L - 1 - tq : tq;
    const u64 row = seq::locate_row(r.pre, t.d0, t.d1, xm);
    return t.base + (u64)r.start0[row] + (xm - (r.pre[row] - r.pre[t.d0]));
}

// a non-SNV allele (d != 1 or m != 1, not both 0) against kept transcript t whose span overlaps F.  ins: A', m bytes.  The record's
// codon and amino-acid bytes stay 0; rule 3 fills q (partial_codon: q only), c and k.  transcript and ref_match are the caller's.
GFFX_HD inline Record classify_any(const Rows &r, const Transcript &t, const uint8_t *bases, uint32_t x0, uint32_t d, uint32_t m, const uint8_t *ins) {
    Record o{};
    if (t.flags & kFlagOverlap) {
        o.cls = kUnclassifiedModel;
        return o;
    }
    const bool minus = t.flags & kFlagMinus, del = d > 0, has_d = t.d1 > t.d0;
    // the span: D and E are sorted and disjoint, so their first starts and last ends give it
    const uint32_t s_d = has_d ? r.start0[t.d0] : 0xFFFFFFFFu, s_e = r.start0[t.e0], e_d = has_d ? r.end[t.d1 - 1] : 0u, e_e = r.end[t.e1 - 1];
    const u64 span_lo = (u64)(s_d < s_e ? s_d : s_e) + 1, span_hi = e_d > e_e ? e_d : e_e;
    const u64 f_lo = del ? (u64)x0 : (u64)x0 - 1, f_hi = del ? (u64)x0 + d - 1 : (u64)x0;
    if (del && f_lo <= span_lo && f_hi >= span_hi) {
        o.cls = kTranscriptAblation;
        return o;
    }
    const u64 lo = f_lo > span_lo ? f_lo : span_lo, hi = f_hi < span_hi ? f_hi : span_hi, width = hi - lo + 1;
    const u64 key[4] = {lo, hi + 1, lo, hi + 1};
    uint32_t n[4];
    count_starts(r, t, key, n);
    const u64 d_lo = bases_below(r, t.d0, n[0], lo), d_cov = bases_below(r, t.d0, n[1], hi + 1) - d_lo;
    const u64 e_lo = bases_below(r, t.e0, n[2], lo), e_cov = bases_below(r, t.e0, n[3], hi + 1) - e_lo;
    const uint8_t sp = splice_class(r, t, lo, hi, !del, n[2]);
    if (sp != kIntron) {
        o.cls = sp;
        return o;
    }
    if (del ? d_cov > 0 : d_cov == width) {
        const uint32_t p = (t.flags & kFlagPhase) >> 1;
        const u64 C = t.L > p ? (t.L - p) / 3 : 0, dc = del ? d_cov : 0;
        const u64 qa = del ? d_lo : d_lo + ((u64)x0 > lo ? 1 : 0);  // (d == 0: lo is in D, the bytes go in behind it unless lo == x0)
        const u64 ta = minus ? t.L - qa - dc : qa, tb = ta + dc;
        o.q = ta;
        if (ta < p || (del ? tb : ta) > p + 3 * C) {
            o.cls = kPartialCodon;
            return o;
        }
        const u64 c = (ta - p) / 3;
        const uint32_t k = (uint32_t)((ta - p) % 3);
        o.c = c, o.k = (uint8_t)k;
        if (p == 0 && (del ? ta < 3 : (ta == 1 || ta == 2))) {  // (C >= 1: ta + dc <= 3C with dc > 0, or 1 <= ta <= 3C)
            const u64 a0 = cds_at(r, t, 0), a1 = cds_at(r, t, 1), a2 = cds_at(r, t, 2);
            const uint8_t g0 = bases[a0], g1 = bases[a1], g2 = bases[a2];
            if ((minus ? seq::translate(seq::complement(g0), seq::complement(g1), seq::complement(g2)) : seq::translate(g0, g1, g2)) == 'M') {
                o.cls = kStartLost;
                return o;
            }
        }
        if (m % 3 != (uint32_t)(dc % 3)) {
            o.cls = kFrameshift;
            return o;
        }
        // 3d: the reference window's codons against the alternate window's; only what decides the class is kept
        const u64 n_ref = (k + dc + 2) / 3, w0 = p + 3 * c;  // the reference window: S[w0, w0 + 3 n_ref)
        const u64 n_alt = m >= dc ? n_ref + (m - dc) / 3 : n_ref - (dc - m) / 3;
        bool unknown = false, stop_ref = false, stop_alt = false, equal = n_ref == n_alt;
        const u64 n_max = n_ref > n_alt ? n_ref : n_alt;
        for (u64 j = 0; j < n_max; ++j) {
            uint8_t aa_r = 0, aa_a = 0;
            if (j < n_ref) {
                const u64 a0 = cds_at(r, t, w0 + 3 * j), a1 = cds_at(r, t, w0 + 3 * j + 1), a2 = cds_at(r, t, w0 + 3 * j + 2);
                const uint8_t g0 = bases[a0], g1 = bases[a1], g2 = bases[a2];  // three independent loads
                aa_r = minus ? seq::translate(seq::complement(g0), seq::complement(g1), seq::complement(g2)) : seq::translate(g0, g1, g2);
            }
            if (j < n_alt) {
                uint8_t b[3];
                for (uint32_t e = 0; e < 3; ++e) {
                    const u64 at = 3 * j + e;  // byte `at` of the alternate window: S[w0, ta) + I + S[tb, w0 + 3 n_ref)
                    if (at < k) {
                        const uint8_t g = bases[cds_at(r, t, w0 + at)];
                        b[e] = minus ? seq::complement(g) : g;
                    } else if (at < (u64)k + m) {
                        b[e] = minus ? seq::complement(ins[m - 1 - (at - k)]) : ins[at - k];
                    } else {
                        const uint8_t g = bases[cds_at(r, t, tb + (at - k - m))];
                        b[e] = minus ? seq::complement(g) : g;
                    }
                }
                aa_a = seq::translate(b[0], b[1], b[2]);
            }
            unknown = unknown || aa_r == 'X' || aa_a == 'X';
            stop_ref = stop_ref || aa_r == '*';
            stop_alt = stop_alt || aa_a == '*';
            equal = equal && aa_r == aa_a;
        }
        o.cls = unknown ? kCodingUnknown
                : equal ? (stop_ref ? kStopRetained : kSynonymous)
                : stop_alt && !stop_ref ? kStopGained
                : stop_ref && !stop_alt ? kStopLost
                : m > dc ? kInframeInsertion
                : m < dc ? kInframeDeletion
                         : kMissense;
        return o;
    }
    if (del ? e_cov > 0 : e_cov == width) {
        // the smallest base of F' in E: lo when a row holds it, else the start of the first row behind it
        const bool lo_in = n[2] > t.e0 && r.end[n[2] - 1] >= lo;
        const u64 u = lo_in ? lo : (u64)r.start0[n[2]] + 1;
        o.cls = !has_d ? kNoncodingExon : u < t.cmin ? (minus ? kUtr3 : kUtr5) : u > t.cmax ? (minus ? kUtr5 : kUtr3) : kNoncodingExon;
        return o;
    }
    o.cls = kIntron;
    return o;
}

// the trimming of --indels: the longest common prefix, case folded, then the longest common suffix of what remains
struct Trimmed {
    uint32_t pfx, d, m;
};
GFFX_HD inline Trimmed trim(const uint8_t *ref, uint32_t n_ref, const uint8_t *alt, uint32_t n_alt) {
    uint32_t pfx = 0;
    while (pfx < n_ref && pfx < n_alt && ((ref[pfx] ^ alt[pfx]) & 0xDFu) == 0) ++pfx;
    uint32_t d = n_ref - pfx, m = n_alt - pfx;
    while (d && m && ((ref[pfx + d - 1] ^ alt[pfx + m - 1]) & 0xDFu) == 0) --d, --m;
    return Trimmed{pfx, d, m};
}

// 1 when REF, case folded, is the genome's base, case folded (REF is a letter: no other byte folds onto one)
GFFX_HD inline uint8_t ref_match(uint8_t ref, uint8_t genome_base) { return (ref & 0xDFu) == (genome_base & 0xDFu) ? 1 : 0; }

// ref_match of an interval: R' (d bytes), case folded, against the genome's bases from g on; 1 for d == 0
GFFX_HD inline uint8_t ref_match_run(const uint8_t *ref, uint32_t d, const uint8_t *g) {
    uint8_t ok = 1;
    for (uint32_t i = 0; i < d; ++i) ok &= ref_match(ref[i], g[i]);
    return ok;
}

// ---- what the build does per transcript, once: rows [f0, f2) are its own, [f0, f1) of kind 0.  Writes pmax for its rows and
// fills t (base and the caller's bits of flags are the caller's: flags comes back as kFlagOverlap or 0); returns false for a transcript that cannot be kept: a member on another sequence
// than the first row's, on a sequence the genome lacks, or beyond its end.  *lo0 / *hi: the span [lo0, hi).
GFFX_HD inline bool build_transcript(const uint32_t *start0, const uint32_t *end, const uint32_t *row_seq, const u64 *pre, uint32_t *pmax, uint32_t f0, uint32_t f1,
                                     uint32_t f2, const uint32_t *seq_len, uint32_t n_seq, Transcript *t, uint32_t *lo0, uint32_t *hi) {
    bool ok = true, overlap = false;
    uint32_t lo = 0xFFFFFFFFu, top = 0;
    const uint32_t sq = row_seq[f0];
    for (uint32_t part = 0; part < 2; ++part) {
        uint32_t run = 0;
        for (uint32_t j = part ? f1 : f0; j < (part ? f2 : f1); ++j) {
            overlap = overlap || start0[j] < run;  // (run: the largest end of the rows before it; 0 for the first)
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
    t->flags = overlap ? kFlagOverlap : 0u;
    t->L = pre[f1] - pre[f0];
    *lo0 = lo, *hi = top;
    return ok;
}

}  // namespace effect
}  // namespace gffx
