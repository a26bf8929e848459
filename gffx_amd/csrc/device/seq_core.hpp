// seq_core.hpp -- the rules of `gffx seq` for the host (g++) and the device (hipcc): what a FASTA line gives, the
// complement of a base, the amino acid of a codon, where character c of a record lies among its segments and which byte of a
// wrapped body is which character.
//
// FASTA.  A line ends at '\n'; a '\r' directly before it is not part of the line.  Empty lines are ignored anywhere.  A line that
// begins with '>' opens a sequence named by the bytes after '>' up to the first blank, TAB or line end; every other line adds all
// of its bytes to the open sequence as they are.  Lines have any lengths.  A last line without '\n' counts.
//
// RECORD.  Its segments [s_i, e_i) (0-based, half-open), ordered by (start, line order), are concatenated: L = sum (e_i - s_i)
// bases, x = 0 .. L - 1.  Transcription position q is x = q on plus and x = L - 1 - q, complemented, on minus.  Without
// --translate the record has C = L characters, character c = base q = c.  With it C = (L - p) / 3 for L > p (else 0), p the phase,
// and character c is the amino acid of the bases q = p + 3c, p + 3c + 1, p + 3c + 2.
//
// BODY.  C characters in lines of W (W = 0: one line), each ended by '\n': C + ceil(C / W) bytes, none for C = 0.
//
// Plain C++17 (GFFX_HD inline, no allocation, no HIP calls): the same code runs in the kernels of genome.hip and seq.hip, in the
// sanitizer build of tools/seq_check.cpp and in its timed build, the one-core baseline.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace seq {

typedef unsigned long long u64;

// ---- the complement: A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H, the same in lower case; S, W, N and every other byte stay
GFFX_HD inline uint8_t complement(uint8_t b) {
    const uint8_t up = (uint8_t)(b & 0xDFu);  // (a letter's two cases differ in bit 5 only)
    if (up < 'A' || up > 'Z') return b;
    uint8_t c;
    switch (up) {
        case 'A': c = 'T'; break;
        case 'T': c = 'A'; break;
        case 'U': c = 'A'; break;
        case 'C': c = 'G'; break;
        case 'G': c = 'C'; break;
        case 'R': c = 'Y'; break;
        case 'Y': c = 'R'; break;
        case 'K': c = 'M'; break;
        case 'M': c = 'K'; break;
        case 'B': c = 'V'; break;
        case 'V': c = 'B'; break;
        case 'D': c = 'H'; break;
        case 'H': c = 'D'; break;
        default: return b;
    }
    return (uint8_t)(c | (b & 0x20u));
}

// ---- NCBI table 1 in TCAG order; stops are '*', a codon with a letter outside TCAG (U reads as T, case is folded) gives 'X'
GFFX_HD inline int base_rank(uint8_t b) {
    switch (b & 0xDFu) {  // (a letter's two cases differ in bit 5 only, and no other byte folds onto a letter)
        case 'T': case 'U': return 0;
        case 'C': return 1;
        case 'A': return 2;
        case 'G': return 3;
        default: return -1;
    }
}
GFFX_HD inline uint8_t amino(uint32_t codon_index) {  // 16 a + 4 b + c over the ranks
    const char *t = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    return (uint8_t)t[codon_index & 63u];
}
GFFX_HD inline uint8_t translate(uint8_t a, uint8_t b, uint8_t c) {
    const int x = base_rank(a), y = base_rank(b), z = base_rank(c);
    if ((x | y | z) < 0) return 'X';
    return amino((uint32_t)(16 * x + 4 * y + z));
}

// ---- characters and wrapped bytes
GFFX_HD inline uint32_t phase_skip(uint8_t col8) { return col8 == '1' ? 1u : col8 == '2' ? 2u : 0u; }
GFFX_HD inline u64 characters(u64 L, uint32_t p, bool translated) { return !translated ? L : L > p ? (L - p) / 3 : 0; }
GFFX_HD inline u64 body_bytes(u64 C, u64 W) { return C == 0 ? 0 : W == 0 ? C + 1 : C + (C + W - 1) / W; }
// byte b < body_bytes(C, W) of a body: the character it holds, or C for a '\n'
GFFX_HD inline u64 body_char(u64 b, u64 C, u64 W) {
    if (W == 0) return b;  // (b == C: the one newline)
    const u64 line = b / (W + 1), col = b % (W + 1), c = line * W + col;
    return col == W || c >= C ? C : c;
}

// ---- a FASTA line D[ls, le): le is its '\n' (terminated) or the end of the bytes at hand.  A continuation is the rest of a
// bases line whose beginning went before (the text is handed over in pieces): never a header.
enum : uint32_t { kLineEmpty = 0, kLineHeader = 1, kLineBases = 2 };
struct LineClass {
    uint32_t kind;
    u64 kept;  // bases lines: the bytes D[ls, ls + kept) join the open sequence
};
GFFX_HD inline LineClass classify_line(const uint8_t *D, u64 ls, u64 le, bool terminated, bool continuation) {
    if (terminated && le > ls && D[le - 1] == '\r') --le;
    if (continuation) return LineClass{kLineBases, le - ls};
    if (le == ls) return LineClass{kLineEmpty, 0};
    if (D[ls] == '>') return LineClass{kLineHeader, 0};
    return LineClass{kLineBases, le - ls};
}
// the name of the header line D[ls, le) (D[ls] == '>'; a '\r' before the '\n' taken off by the caller): D[ls + 1, name_end)
GFFX_HD inline u64 name_end(const uint8_t *D, u64 ls, u64 le) {
    u64 k = ls + 1;
    while (k < le && D[k] != ' ' && D[k] != '\t') ++k;
    return k;
}

// ---- where base x of a record lies: the last row i in [f0, f1) with pre[i] - pre[f0] <= x (pre: the exclusive sums of the rows'
// lengths, no row is empty)
GFFX_HD inline u64 locate_row(const u64 *pre, u64 f0, u64 f1, u64 x) {
    const u64 want = pre[f0] + x;
    u64 lo = f0, hi = f1;  // pre[lo] <= want < pre[hi]
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (pre[mid] <= want) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the last index i in [0, n) with off[i] <= x (off ascending, off[0] <= x)
GFFX_HD inline u64 last_le(const u64 *off, u64 n, u64 x) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace seq
}  // namespace gffx
