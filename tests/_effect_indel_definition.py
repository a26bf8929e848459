"""The definition of `gffx effect --indels` in plain Python (classify_any of device/effect_core.hpp is its C++ twin),
by brute force: the coding sequence S and the edited S' are built as Python strings, sliced and translated with the dict codon
table; sets of bases stand for D, E and the splice windows.  No prefix sums, no searches.

ALLELES.  REF and an ALT piece, each 1 .. 65 535 bytes of ACGTNacgtn, are trimmed case-folded: the longest common prefix (pfx
bytes), then the longest common suffix of the rest.  R' has d bases from x0 = POS + pfx on, A' has m bytes.  d == m == 1 is an
SNV at x0 and goes to _effect_definition.classify.  F = [x0, x0 + d - 1] for d > 0 and the flanking bases [x0 - 1, x0] for
d == 0; an allele pairs with every kept transcript whose span meets F, provided F lies inside the sequence.  F' is F clipped
to the span; F' HITS W when it meets W (d > 0) or lies inside W (d == 0).  The first rule that applies:
  0 unclassified_model   two rows of D or two rows of E overlap (touching rows do not)
  1 transcript_ablation  d > 0 and F holds the whole span
  2 splice               the windows are the first two and the last two bases of every gap between neighbouring E rows (fewer
                         in a gap of fewer); of those F' hits, the one with the smallest first base, the left one on a tie:
                         left is splice_donor on plus, right splice_acceptor, the other way round on minus
  3 coding               F' hits D.  S = D's bases in genomic order; the D bases of F' go, A' comes in where they stood (for
                         d == 0: in front of x0).  In transcription order the run is [ta, tb), dc = tb - ta, I = A' (reverse
                         complemented on minus); q = ta, and c, k = divmod(ta - p, 3)
       3a partial_codon  ta < p or tb > p + 3C (d == 0: ta > p + 3C); q only
       3b start_lost     p == 0, codon 0 is M, and ta < 3 (d == 0: ta in 1, 2)
       3c frameshift     (m - dc) % 3 != 0
       3d                codons c .. c + n_ref - 1, n_ref = ceil((k + dc) / 3), against S[p + 3c, ta) + I + S[tb, p + 3(c + n_ref)):
                         an X in either coding_unknown; equal stop_retained (with a *) or synonymous; a * only in the alternate
                         stop_gained; only in the reference stop_lost; else inframe_insertion (m > dc), inframe_deletion
                         (m < dc) or missense
  4 exonic               F' hits E: the SNV's rule 2 at the smallest base of F' in E
  5 intron
The genome is not consulted to left-align anything, and the residues an in-frame change replaces are not reported.

THE WORKED EXAMPLE (HAND_*), on chrA and the transcripts tP (+), tM (-) and tN of _effect_definition, plus
  tO (+)  CDS 50-54 and 53-57: its two rows overlap

    pos  1 AC GTCA GTAAG CC GATGCTN GTA TAATGG GCA CTTGACAT TTAG CCC ACGTA GGT TTC GA
           1  3    7     12 14      21  24     30  33       41   45  48    53  56  59
  tP  exons 3-6 12-20 24-29 33-44; CDS 14-20 24-29 33-40, L = 21, p = 1, C = 6: S = G ATG CTN TAA TGG CTT GAC AT
      pos(14) = 0, pos(24) = 7, pos(33) = 13
  tM  the same rows on minus, p = 0, C = 7: revcomp(S) = ATG TCA AGC CAT TAN AGC ATC; ta = 21 - qa - dc
  tN  exons 48-52 56-58, no CDS: the gap's windows are 53-54 and 54-55

  POS REF>ALT   trimmed        tP: class cds_pos aa_pos                          tM
   2 CGT>C      x0 3 d 2 m 0   F = 3-4 meets exon 3-6, before 14: 5_prime_UTR    3_prime_UTR
   2 C..G>C     x0 3 d 42      F = 3-44 holds the span: transcript_ablation      transcript_ablation
   3 G>GA       x0 4 d 0 m 1   F = 3-4 inside exon 3-6: 5_prime_UTR              3_prime_UTR
   6 AG>A       x0 7 d 1       F = 7 meets the left window 7-8: splice_donor     splice_acceptor
   8 TA>T       x0 9 d 1       F = 9: no window (7-8, 10-11), no row: intron     intron
   9 A>ATT      x0 10 d 0 m 2  F = 9-10 inside neither window: intron            intron
  10 A>AC       x0 11 d 0 m 1  F = 10-11 is the right window: splice_acceptor    splice_donor
  13 CG>C       x0 14 d 1      3a: ta = 0 < p: partial_codon 1 .                 ta = 20, tb = 21 = 3C; 3c: -1 % 3: frameshift 21 7
  15 A>AT       x0 16 d 0 m 1  qa = pos(16) = 2 = ta, k = 1, c = 0; p = 1, so    ta = 19: frameshift 20 7
                               no 3b; 3c: frameshift 3 1
  15 ATG>A      x0 16 d 2      ta = 2, dc = 2: frameshift 3 1                    ta = 17: frameshift 18 6
  15 ATGC>A     x0 16 d 3      ta = 2, k = 1, n_ref = 2: ATG CTN holds an X:     ta = 16, k = 1, n_ref = 2: AGC ATC (S I) against
                               coding_unknown 3 1                                A + TC = ATC (I): inframe_deletion 17 6
  16 TGC>TAC    x0 17 d 1 m 1  the SNV G>A at 17: missense 4 ATG>ATA 1 M>I       synonymous 18 AGC>AGT 6 S>S
  24 T>TTAA     x0 25 d 0 m 3  qa = pos(25) = 8, k = 1, c = 2, n_ref = 1: TAA    ta = 13, k = 1, c = 4: TAN holds an X:
                               (*) against T + TAA + AA = TTA AAA (L K):         coding_unknown 14 5
                               stop_lost 9 3
  26 A>AGGG     x0 27 d 0 m 3  qa = 10, k = 0, c = 3, n_ref = 0: "" against      ta = 11, k = 2, c = 3: CAT (H) against CA + CCC + T
                               GGG (G): inframe_insertion 11 4                   = CAC CCT (H P): inframe_insertion 12 4
  27 TGG>TAA    x0 28 d 2 m 2  qa = 11, dc = 2, k = 1, c = 3: TGG (W) against    ta = 8, k = 2, c = 2, n_ref = 2: AGC CAT (S H) against
                               T + AA = TAA (*): stop_gained 12 4                AG + TT + AT = AGT TAT (S Y): missense 9 3
  34 TTG>T      x0 35 d 2      qa = 15, k = 2, c = 4: frameshift 16 5            ta = 4: frameshift 5 2
  37 ACA>A      x0 38 d 2      qa = 18, tb = 20 > p + 3C = 19: partial_codon 19  ta = 1 < 3, p = 0, ATG: 3b start_lost 2 1
  38 C>CAAA     x0 39 d 0 m 3  qa = 19 = p + 3C (not beyond), k = 0, c = 6,      ta = 2, in (1, 2): start_lost 3 1
                               n_ref = 0: "" against AAA (K): inframe_insertion 20 7
  39 AT>A       x0 40 d 1      qa = 20, tb = 21 > 19: partial_codon 21           ta = 0 < 3: start_lost 1 1
  49 C>CA       x0 50 d 0 m 1  tN: F = 49-50 inside exon 48-52, no CDS: noncoding_exon;  tO: unclassified_model
  51 TAG>T      x0 52 d 2      tN: F = 52-53 meets the window 53-54 (rule 2 comes before rule 4): splice_donor;  tO: unclassified_model
"""
import random

import _effect_definition as D
from _seq_definition import revcomp

CLASSES_ALL = D.CLASSES + ("frameshift", "inframe_insertion", "inframe_deletion", "transcript_ablation", "unclassified_model")
RULE3 = ("partial_codon",) + D.CODING + ("frameshift", "inframe_insertion", "inframe_deletion")  # cds_pos (and aa_pos) are filled
MAX_LEN = 65535
BASES = b"ACGTNacgtn"


def trim(pos: int, ref: bytes, alt: bytes):
    """(x0, d, m, R', A') of REF / ALT piece at POS."""
    r, a = ref.upper(), alt.upper()
    pfx = 0
    while pfx < len(r) and pfx < len(a) and r[pfx] == a[pfx]:
        pfx += 1
    d, m = len(r) - pfx, len(a) - pfx
    while d and m and r[pfx + d - 1] == a[pfx + m - 1]:
        d, m = d - 1, m - 1
    return pos + pfx, d, m, ref[pfx:pfx + d], alt[pfx:pfx + m]


def overlapping(rows) -> bool:
    """Some row starts before the largest end of the rows before it (rows: (start - 1, end) by start)."""
    top = 0
    for s, e in rows:
        if s < top:
            return True
        top = max(top, e)
    return False


def footprint(x0, d):
    return (x0, x0 + d - 1) if d else (x0 - 1, x0)


def windows_hit(tr, x0: int, d: int):
    """The splice windows that F' hits: (first base, 0 for a left and 1 for a right window) each."""
    f_lo, f_hi = footprint(x0, d)
    F = [b for b in range(f_lo, f_hi + 1) if tr["lo"] <= b <= tr["hi"]]
    hits = (lambda W: any(b in W for b in F)) if d else (lambda W: bool(W) and all(b in W for b in F))
    found = []
    for (s, e), (s2, e2) in zip(tr["E"], tr["E"][1:]):
        a, b = e, s2 + 1
        left, right = list(range(a + 1, min(a + 2, b - 1) + 1)), list(range(max(b - 2, a + 1), b))
        for side, w in ((0, left), (1, right)):
            if w and hits(set(w)):
                found.append((w[0], side))
    return found


def classify_any(tr, seq: bytes, x0: int, d: int, ins: bytes):
    """(class, q, c, k) of the non-SNV allele (x0, d, ins) against kept transcript tr whose span meets F."""
    D_, E, minus, p = tr["D"], tr["E"], tr["minus"], tr["p"]
    m = len(ins)
    if overlapping(D_) or overlapping(E):
        return ("unclassified_model", 0, 0, 0)
    f_lo, f_hi = footprint(x0, d)
    if d and f_lo <= tr["lo"] and f_hi >= tr["hi"]:
        return ("transcript_ablation", 0, 0, 0)
    F = [b for b in range(f_lo, f_hi + 1) if tr["lo"] <= b <= tr["hi"]]  # F'
    hits = (lambda W: any(b in W for b in F)) if d else (lambda W: bool(W) and all(b in W for b in F))
    # 2: the windows
    found = windows_hit(tr, x0, d)
    if found:
        side = min(found)[1]
        return ("splice_donor" if (side == 0) != minus else "splice_acceptor", 0, 0, 0)
    # 3: coding
    coords = [b for s, e in D_ for b in range(s + 1, e + 1)]  # the genomic base behind every byte of S
    in_d = set(coords)
    if hits(in_d):
        S = bytes(seq[b - 1] for b in coords)
        in_f = set(F)
        gone = [i for i, b in enumerate(coords) if b in in_f] if d else []
        qa = gone[0] if d else sum(1 for b in coords if b < x0)
        dc = len(gone)
        S2 = S[:qa] + ins + S[qa + dc:]
        L = len(S)
        if minus:
            S, S2, I, ta = revcomp(S), revcomp(S2), revcomp(ins), L - qa - dc
        else:
            I, ta = ins, qa
        tb = ta + dc
        assert S2 == S[:ta] + I + S[tb:]
        C = (L - p) // 3 if L > p else 0
        if ta < p or (tb if d else ta) > p + 3 * C:
            return ("partial_codon", ta, 0, 0)
        c, k = divmod(ta - p, 3)
        if p == 0 and D.amino(S[0:3]) == "M" and len(S) >= 3 and (ta < 3 if d else ta in (1, 2)):
            return ("start_lost", ta, c, k)
        if (m - dc) % 3:
            return ("frameshift", ta, c, k)
        n_ref = -(-(k + dc) // 3)
        w0, w1 = p + 3 * c, p + 3 * (c + n_ref)
        ref_w, alt_w = S[w0:w1], S[w0:ta] + I + S[tb:w1]
        assert len(ref_w) == 3 * n_ref and len(alt_w) == 3 * n_ref + m - dc
        ra = "".join(D.amino(ref_w[i:i + 3]) for i in range(0, len(ref_w), 3))
        aa = "".join(D.amino(alt_w[i:i + 3]) for i in range(0, len(alt_w), 3))
        if "X" in ra or "X" in aa:
            cls = "coding_unknown"
        elif ra == aa:
            cls = "stop_retained" if "*" in ra else "synonymous"
        elif "*" in aa and "*" not in ra:
            cls = "stop_gained"
        elif "*" in ra and "*" not in aa:
            cls = "stop_lost"
        else:
            cls = "inframe_insertion" if m > dc else "inframe_deletion" if m < dc else "missense"
        return (cls, ta, c, k)
    # 4: exonic
    in_e = {b for s, e in E for b in range(s + 1, e + 1)}
    if hits(in_e):
        u = min(b for b in F if b in in_e)
        if not D_:
            return ("noncoding_exon", 0, 0, 0)
        cmin, cmax = min(s for s, e in D_) + 1, max(e for s, e in D_)
        if u < cmin:
            return ("3_prime_UTR" if minus else "5_prime_UTR", 0, 0, 0)
        if u > cmax:
            return ("5_prime_UTR" if minus else "3_prime_UTR", 0, 0, 0)
        return ("noncoding_exon", 0, 0, 0)
    return ("intron", 0, 0, 0)


def served(seqs, q, x0, d) -> bool:
    lo, hi = footprint(x0, d)
    return q < len(seqs) and lo >= 1 and hi <= len(seqs[q])


def ref_match(seqs, q, x0, d, ref: bytes) -> int:
    if not served(seqs, q, x0, d):
        return 0
    if d == 0:
        return 1
    return 1 if seqs[q][x0 - 1:x0 - 1 + d].upper() == ref.upper() else 0


def pairs_any(seqs, rows, tr_flags, alleles):
    """(offsets, ref_match, records) for alleles (sequence number, x0, R', A'): records as _effect_definition.pairs gives them
    (transcript, class, q, c, k, codon_ref, codon_alt, aa_ref, aa_alt, ref_match); an allele with d == m == 1 takes the SNV's
    definition."""
    trs = D.transcripts(seqs, rows, tr_flags)
    off, rms, recs = [0], [], []
    for q, x0, ref, ins in alleles:
        d = len(ref)
        rm = ref_match(seqs, q, x0, d, ref)
        rms.append(rm)
        lo, hi = footprint(x0, d)
        if served(seqs, q, x0, d):
            for t, tr in enumerate(trs):
                if tr["kept"] and tr["seq"] == q and lo <= tr["hi"] and hi >= tr["lo"]:
                    if d == 1 and len(ins) == 1:
                        recs.append((t,) + D.classify(tr, seqs[q], x0, ins) + (rm,))
                    else:
                        recs.append((t,) + classify_any(tr, seqs[q], x0, d, ins) + (b"", b"", "", "", rm))
        off.append(len(recs))
    return off, rms, recs


def device_records(recs):
    """As _effect_definition.device_records, over the 20 classes."""
    out = []
    for t, cls, q, c, k, cr, ca, ar, aa, rm in recs:
        out.append((q, c, t, CLASSES_ALL.index(cls), k, rm, ord(ar) if ar else 0, ord(aa) if aa else 0, tuple(cr) if cr else (0, 0, 0), tuple(ca) if ca else (0, 0, 0)))
    return out


def device_rows(alleles):
    """((n, 6) rows (sequence number, x0, d, m, offset low, offset high), the arena: R' then A' per allele) for Effect.run_any."""
    rows, arena = [], bytearray()
    for q, x0, ref, ins in alleles:
        rows.append((q, x0, len(ref), len(ins), len(arena) & 0xFFFFFFFF, len(arena) >> 32))
        arena += ref + ins
    return rows, bytes(arena)


# ---- the command with --indels -----------------------------------------------------------------------------------------------------

COUNTS = ("other", "too_long", "same", "ins_at_1")
WARNINGS = {"other": b"alleles are not sequences of ACGTN (*, ., symbolic, breakend or another byte) and were left out",
            "too_long": b"alleles have a REF or an ALT longer than 65535 bytes and were left out",
            "same": b"alleles are equal to REF and were left out",
            "ins_at_1": b"alleles are insertions in front of a sequence's first base and were left out"}


def parse_vcf_indels(data: bytes):
    """(alleles, counts): alleles (line number, chrom, POS, REF, piece) of the taken ones; counts by COUNTS."""
    out, cnt = [], dict.fromkeys(COUNTS, 0)
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for n, line in enumerate(lines, 1):
        if line.endswith(b"\r") and (n < len(lines) or data.endswith(b"\n")):
            line = line[:-1]
        if not line or line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        if len(f) < 5:
            raise D.VcfError(n, "fewer than 5 fields")
        if not (1 <= len(f[1]) <= 10 and f[1].isdigit() and 1 <= int(f[1]) <= 2 ** 32 - 1):
            raise D.VcfError(n, "POS")
        for piece in f[4].split(b","):
            if not f[3] or not piece or any(b not in BASES for b in f[3]) or any(b not in BASES for b in piece):
                cnt["other"] += 1
            elif len(f[3]) > MAX_LEN or len(piece) > MAX_LEN:
                cnt["too_long"] += 1
            else:
                x0, d, m, _, _ = trim(int(f[1]), f[3], piece)
                if d == 0 and m == 0:
                    cnt["same"] += 1
                elif d == 0 and x0 == 1:
                    cnt["ins_at_1"] += 1
                else:
                    out.append((n, f[0], int(f[1]), f[3], piece))
    return out, cnt


def render_indels(gff: bytes, fasta: bytes, vcf: bytes, cds_type="CDS", exon_type="exon"):
    """(the table, the summary of 20 lines, counts) of `gffx effect --indels`."""
    from _seq_definition import parse_fasta
    names, seqs = parse_fasta(fasta)
    number = {n: i for i, n in enumerate(names)}
    known = set(D.gff_seqids(gff))
    rows, flags, tnames, strands, cnt = D.gff_transcripts(gff, names, seqs, cds_type, exon_type)
    taken, c2 = parse_vcf_indels(vcf)
    cnt.update(c2)
    cnt["no_chrom"] = sum(1 for a in taken if a[1] not in known)
    taken = [a for a in taken if a[1] in known]
    alleles = []
    for _, chrom, pos, ref, alt in taken:
        x0, d, m, rp, ap = trim(pos, ref, alt)
        alleles.append((number.get(chrom, D.NO_SEQ), x0, rp, ap))
    off, rms, recs = pairs_any(seqs, rows, flags, alleles)
    out = ["#chrom\tpos\tref\talt\ttranscript\tstrand\tclass\tcds_pos\tcodons\taa_pos\taa\tref_match\n"]
    n_alleles, n_pairs = {c: 0 for c in CLASSES_ALL}, {c: 0 for c in CLASSES_ALL}
    for i, (_, chrom, pos, ref, alt) in enumerate(taken):
        snv = len(alleles[i][2]) == 1 and len(alleles[i][3]) == 1
        head = "%s\t%d\t%s\t%s\t" % (chrom.decode("latin-1"), pos, ref.decode(), alt.decode())
        if off[i] == off[i + 1]:
            out.append(head + ".\t.\tintergenic\t.\t.\t.\t.\t%d\n" % rms[i])
            n_alleles["intergenic"] += 1
            n_pairs["intergenic"] += 1
        seen = set()
        for t, cls, q, c, k, cr, ca, ar, aa, rm in recs[off[i]:off[i + 1]]:
            if snv:
                coding = "%d\t%s>%s\t%d\t%s>%s" % (q + 1, cr.upper().decode("latin-1"), ca.upper().decode("latin-1"), c + 1, ar, aa) if cls in D.CODING else ".\t.\t.\t."
            elif cls in RULE3:
                coding = "%d\t.\t%s\t." % (q + 1, "." if cls == "partial_codon" else "%d" % (c + 1))
            else:
                coding = ".\t.\t.\t."
            out.append(head + "%s\t%s\t%s\t%s\t%d\n" % (tnames[t], strands[t], cls, coding, rm))
            n_pairs[cls] += 1
            if cls not in seen:
                n_alleles[cls] += 1
                seen.add(cls)
    summary = "".join("%s\t%d\t%d\n" % (c, n_alleles[c], n_pairs[c]) for c in CLASSES_ALL)
    return "".join(out).encode("latin-1"), summary.encode(), cnt


# ---- random inputs ----------------------------------------------------------------------------------------------------------------

def random_disjoint_case(seed, n_seq=2, seq_len=(300, 180), n_tr=12, n_alleles=200, alphabet=b"ACGTACGTACGTacgtN", gaps=(0, 1, 2, 3, 4, 5, 6), snv=0.15,
                         max_len=7):
    """(seqs, rows, tr_flags, alleles): transcripts whose rows do not overlap (touching ones with the gap 0), as random_case
    makes them without the kind "messy" and without dropped ones; alleles (sequence number, x0, R', A') with d, m in
    0 .. max_len, some of them SNVs, R' mostly the genome's."""
    seqs, rows, flags, _ = D.random_case(seed, n_seq=n_seq, seq_len=seq_len, n_tr=n_tr, n_alleles=0, alphabet=alphabet, bad=False,
                                         kinds=("coding", "coding", "coding+exons", "coding+utr", "noncoding"), gaps=gaps)
    rng = random.Random(seed * 7919 + 1)
    alleles = []
    while len(alleles) < n_alleles:
        q = rng.randrange(n_seq)
        n = len(seqs[q])
        if rng.random() < snv:
            d, m = 1, 1
        else:
            d, m = rng.randint(0, max_len), rng.randint(0, max_len)
        x0 = rng.randint(1, n)
        if rng.random() < 0.6 and rows:  # (near a row's edge)
            t, qq, s, e, k = rng.choice(rows)
            q, n = qq, len(seqs[qq])
            x0 = min(n, max(1, rng.choice((s + 1, e)) + rng.randint(-d - 2, 2)))
        ref = seqs[q][x0 - 1:x0 - 1 + d]
        if len(ref) < d or (d == 0 and x0 == 1):
            continue
        if rng.random() < 0.1:
            ref = bytes(rng.choice(b"ACGT") for _ in range(d))
        ins = bytes(rng.choice(b"ACGTacgtN" if rng.random() < 0.1 else b"ACGT") for _ in range(m))
        if d and m and (ref[:1].upper() == ins[:1].upper() or ref[-1:].upper() == ins[-1:].upper()):
            continue  # (not trimmed)
        if d == 0 and m == 0:
            continue
        alleles.append((q, x0, ref, ins))
    return seqs, rows, flags, alleles


# ---- the cases that the host tool (test_effect_indel_cpu.py) and the device (test_effect_indel_gpu.py) are both held to ------------

def fill(d_or_m, avoid_first=b"", avoid_last=b"", salt=0):
    """d_or_m bases whose first and last differ (case folded) from the given ones: an allele made of them stays trimmed."""
    out = bytearray(b"ACGT"[(i + salt) % 4] for i in range(d_or_m))
    if out and avoid_first and bytes(out[:1]).upper() == avoid_first.upper():
        out[0] = b"ACGT"[(b"ACGT".index(out[0]) + 1) % 4]
    if out and avoid_last:
        for _ in range(3):
            if bytes(out[-1:]).upper() == avoid_last.upper() or (len(out) == 1 and avoid_first and bytes(out[:1]).upper() == avoid_first.upper()):
                out[-1] = b"ACGT"[(b"ACGT".index(out[-1]) + 1) % 4]
    return bytes(out)


def allele(seqs, q, x0, d, m, salt=0):
    """The allele that deletes the genome's own d bases at x0 and brings m bases in; None when it would leave the sequence or
    be an insertion in front of base 1."""
    if x0 < 1 or x0 - 1 + d > len(seqs[q]) or (d == 0 and (x0 < 2 or m == 0 or x0 > len(seqs[q]))):
        return None
    ref = seqs[q][x0 - 1:x0 - 1 + d]
    return (q, x0, ref, fill(m, ref[:1], ref[-1:], salt))


def alleles_at(seqs, xs, shapes, q=0):
    out = []
    for x0 in xs:
        for k, (d, m) in enumerate(shapes):
            a = allele(seqs, q, x0, d, m, salt=x0 + k)
            if a:
                out.append(a)
    return out


GENOME = bytes(b"ATGGCCTAAGGTNACTGACCATGAAACGT"[i % 29] for i in range(240))
SHAPES_SMALL = ((1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (0, 2), (0, 3), (2, 2), (3, 1), (1, 4))


def case_introns():
    """Introns of 0 (touching rows) to 5 bases, as exon-only, CDS-only and CDS + exon transcripts on both strands."""
    segs, at = [], 5
    for gap in (1, 2, 3, 4, 5, 0, 0, 2, 1):
        segs.append((at, at + 4))
        at += 4 + gap
    segs.append((at, at + 6))
    rows, flags = [], []
    for kinds in ((1,), (0,), (0, 1)):
        for minus in (0, 1):
            rows += [(len(flags), 0, s, e, k) for k in kinds for s, e in segs]
            flags.append(minus | (len(flags) % 3) << 1)
    return [GENOME], rows, flags, alleles_at([GENOME], range(2, at + 10), SHAPES_SMALL + ((9, 0), (14, 3)))


def case_one_base_exons():
    """Five one-base segments a base apart, then a longer one: windows across three of them, every phase, both strands."""
    segs = [(s, s + 1) for s in (10, 12, 14, 16, 18)] + [(20, 31)]
    rows, flags = [], []
    for p in (0, 1, 2):
        for minus in (0, 1):
            rows += [(len(flags), 0, s, e, 0) for s, e in segs]
            flags.append(minus | p << 1)
    return [GENOME], rows, flags, alleles_at([GENOME], range(8, 34), [(d, m) for d in range(8) for m in range(8) if (d, m) != (0, 0)])


def case_phases():
    """Every phase against k = 0, 1, 2 and d, m in 0 .. 7: one segment of 30 bases from the start codon at base 1."""
    rows, flags = [], []
    for p in (0, 1, 2):
        for minus in (0, 1):
            rows.append((len(flags), 0, 0, 30, 0))
            flags.append(minus | p << 1)
    rows.append((len(flags), 0, 203, 233, 0))  # (ATG AAA CGT ... on plus from base 204)
    flags.append(0)
    xs = list(range(1, 12)) + list(range(24, 33)) + list(range(203, 210))
    return [GENOME], rows, flags, alleles_at([GENOME], xs, [(d, m) for d in range(8) for m in range(8) if (d, m) != (0, 0)])


def case_edges():
    """Deletions that end (and begin) on, one before and one past every row's edge, cmin, cmax and the span's edges, insertions
    at every such junction, F equal to the span and one base short of it; both strands, with UTR exons and without exon lines."""
    cds = [(49, 60), (70, 71), (80, 95), (95, 101)]  # (the last two touch)
    exons = [(39, 60), (70, 71), (80, 101), (110, 120)]
    rows, flags = [], []
    for minus in (0, 1):
        rows += [(len(flags), 0, s, e, 0) for s, e in cds] + [(len(flags), 0, s, e, 1) for s, e in exons]
        flags.append(minus | 2)
        rows += [(len(flags), 0, s, e, 0) for s, e in cds]
        flags.append(minus)
    marks = sorted({v for s, e in cds + exons for v in (s + 1, e)})
    alleles = []
    for b in marks:
        for d in (1, 2, 3, 4, 6, 12):
            for end in (b - 1, b, b + 1):
                alleles += [allele([GENOME], 0, end - d + 1, d, 0), allele([GENOME], 0, end - d + 1, d, 2, salt=b)]
            for start in (b - 1, b, b + 1):
                alleles += [allele([GENOME], 0, start, d, 0), allele([GENOME], 0, start, d, d, salt=b)]
        for x0 in (b - 1, b, b + 1, b + 2):
            alleles += [allele([GENOME], 0, x0, 0, m, salt=b) for m in (1, 2, 3, 6)]
    for lo, hi in ((40, 120), (50, 101)):  # the two spans
        for a, b in ((lo, hi), (lo + 1, hi), (lo, hi - 1), (lo - 1, hi + 1), (lo - 1, hi - 1), (lo + 1, hi + 1)):
            alleles += [allele([GENOME], 0, a, b - a + 1, 0), allele([GENOME], 0, a, b - a + 1, 4)]
    return [GENOME], rows, flags, [a for a in alleles if a]


def case_overlapping_between_clean():
    """t1 has two CDS rows that overlap, t3 two exon rows; t0, t2 and t4 around them are classified.  An SNV still is."""
    rows = [(0, 0, 20, 40, 0), (1, 0, 22, 30, 0), (1, 0, 28, 38, 0), (2, 0, 24, 36, 0), (3, 0, 21, 25, 0), (3, 0, 18, 26, 1), (3, 0, 25, 39, 1), (4, 0, 19, 41, 1),
            (5, 0, 22, 30, 0), (5, 0, 30, 38, 0)]  # t5: t1 with touching rows
    alleles = alleles_at([GENOME], range(17, 44), ((1, 0), (3, 0), (0, 1), (0, 3), (2, 5), (1, 1), (30, 0)))
    return [GENOME], rows, [0, 1, 2, 0, 1, 1], alleles


CASES = {"introns": case_introns, "one_base_exons": case_one_base_exons, "phases": case_phases, "edges": case_edges, "overlapping": case_overlapping_between_clean}


# ---- the worked example -------------------------------------------------------------------------------------------------------------
HAND_GFF = D.HAND_GFF + b"chrA\th\tCDS\t50\t54\t.\t+\t0\tID=tO.c1;Parent=tO\nchrA\th\tCDS\t53\t57\t.\t+\t0\tID=tO.c2;Parent=tO\n"
# pos ref alt, then per transcript hit: name strand class cds_pos codons aa_pos aa; ref_match last
_HAND = """
2 CGT C tP + 5_prime_UTR . . . . tM - 3_prime_UTR . . . . | 1
2 %s C tP + transcript_ablation . . . . tM - transcript_ablation . . . . | 1
3 G GA tP + 5_prime_UTR . . . . tM - 3_prime_UTR . . . . | 1
6 AG A tP + splice_donor . . . . tM - splice_acceptor . . . . | 1
8 TA T tP + intron . . . . tM - intron . . . . | 1
9 A ATT tP + intron . . . . tM - intron . . . . | 1
10 A AC tP + splice_acceptor . . . . tM - splice_donor . . . . | 1
13 CG C tP + partial_codon 1 . . . tM - frameshift 21 . 7 . | 1
15 A AT tP + frameshift 3 . 1 . tM - frameshift 20 . 7 . | 1
15 ATG A tP + frameshift 3 . 1 . tM - frameshift 18 . 6 . | 1
15 ATGC A tP + coding_unknown 3 . 1 . tM - inframe_deletion 17 . 6 . | 1
16 TGC TAC tP + missense 4 ATG>ATA 1 M>I tM - synonymous 18 AGC>AGT 6 S>S | 1
24 T TTAA tP + stop_lost 9 . 3 . tM - coding_unknown 14 . 5 . | 1
26 A AGGG tP + inframe_insertion 11 . 4 . tM - inframe_insertion 12 . 4 . | 1
27 TGG TAA tP + stop_gained 12 . 4 . tM - missense 9 . 3 . | 1
34 TTG T tP + frameshift 16 . 5 . tM - frameshift 5 . 2 . | 1
37 ACA A tP + partial_codon 19 . . . tM - start_lost 2 . 1 . | 1
38 C CAAA tP + inframe_insertion 20 . 7 . tM - start_lost 3 . 1 . | 1
39 AT A tP + partial_codon 21 . . . tM - start_lost 1 . 1 . | 1
49 C CA tN + noncoding_exon . . . . tO + unclassified_model . . . . | 1
51 TAG T tN + splice_donor . . . . tO + unclassified_model . . . . | 1
""" % D.HAND_CHRA[1:44].decode()


def _hand():
    out, vcf = ["#chrom\tpos\tref\talt\ttranscript\tstrand\tclass\tcds_pos\tcodons\taa_pos\taa\tref_match\n"], ["##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n"]
    for line in _HAND.strip().split("\n"):
        left, rm = line.split("|")
        w = left.split()
        head = "chrA\t%s\t%s\t%s\t" % tuple(w[:3])
        vcf.append("chrA\t%s\t.\t%s\t%s\n" % tuple(w[:3]))
        for h in (w[i:i + 7] for i in range(3, len(w), 7)):
            out.append(head + "\t".join(h) + "\t" + rm.strip() + "\n")
    return "".join(out).encode(), "".join(vcf).encode()


HAND_OUT, HAND_VCF = _hand()


def random_files(seed, crlf=False):
    """(gff, fasta, vcf): the annotation and the genome of _effect_definition.random_files (Parent lists, orphans, transcripts on
    two strands or seqids, on a seqid the FASTA lacks, beyond a sequence's end, rows that overlap) with variants of every kind:
    REF mostly the genome's own bases, deletions, insertions, MNVs, untrimmed pieces, pieces equal to REF, insertions at POS 1,
    '*', '.', symbolic pieces, an unknown CHROM."""
    from _seq_definition import parse_fasta
    gff, fasta, _ = D.random_files(seed, crlf)
    names, seqs = parse_fasta(fasta)
    by_name = dict(zip(names, seqs))
    spots = []
    for line in gff.split(b"\n"):
        f = line.split(b"\t")
        if len(f) > 8 and f[2] in (b"CDS", b"exon"):
            spots.append((f[0].decode(), int(f[3]), int(f[4])))
    rng = random.Random(seed * 31 + 5)
    vcf = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL"]
    for _ in range(300):
        chrom = rng.choice(("chrA", "chrA", "chrB", "chrC", "chrD", "chrZ"))
        x = rng.randint(1, 60)
        if rng.random() < 0.75:
            chrom, lo, hi = rng.choice(spots)
            x = max(1, rng.choice((lo, hi)) + rng.randint(-5, 3))
        if rng.random() < 0.05:
            x = 1
        seq = by_name.get(chrom, b"")
        n = rng.choice((1, 1, 1, 2, 3, 4, 7))
        ref = seq[x - 1:x - 1 + n].decode() if len(seq) >= x - 1 + n and rng.random() < 0.85 else "".join(rng.choice("ACGT") for _ in range(n))
        alts = []
        for _ in range(rng.choice((1, 1, 1, 2, 3))):
            how = rng.random()
            if how < 0.3:
                alts.append(ref[:1] + "".join(rng.choice("ACGTacgtN") for _ in range(rng.randint(0, 5))))
            elif how < 0.5:
                alts.append("".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4))) + ref)
            elif how < 0.8:
                alts.append("".join(rng.choice("ACGT") for _ in range(rng.randint(1, 6))))
            else:
                alts.append(rng.choice(("*", ".", "<DEL>", ref, ref.lower(), "A]chr2:7]", "")))
        vcf.append("%s\t%d\t.\t%s\t%s\t50" % (chrom, x, ref, ",".join(alts)))
    nl = "\r\n" if crlf else "\n"
    return gff, fasta, (nl.join(vcf) + nl).encode()


# what `gffx effect --indels --help` prints
HELP = (b"Usage: gffx effect --indels [OPTIONS] --input <FILE> --fasta <FILE> --variants <FILE>\n\nOptions:\n"
        b"  -i, --input <FILE>       Input GFF file path\n"
        b"  -f, --fasta <FILE>       The genome as plain FASTA (lines of any lengths; a compressed file is refused)\n"
        b"  -V, --variants <FILE>    The variants as plain text, CHROM POS ID REF ALT per line as in VCF ('#' lines are skipped; a\n"
        b"                           compressed file is refused).  ALT is split at ','\n"
        b"      --indels             Take insertions, deletions and multi-base substitutions as well: REF and an ALT piece of 1 to\n"
        b"                           65535 bases of ACGTN each\n"
        b"  -o, --output <FILE>      Output file (stdout if not provided)\n"
        b"      --cds-type <TYPE>    Feature type (column 3) whose lines give a transcript's coding segments [default: CDS]\n"
        b"      --exon-type <TYPE>   Feature type whose lines give its exons [default: exon]\n"
        b"      --summary <FILE>     Write 'class<TAB>alleles<TAB>pairs' for every class\n"
        b"  -t, --threads <NUM>      Number of threads for parallel processing [default: 12]\n"
        b"  -v, --verbose            Enable verbose output\n"
        b"      --device <N>         HIP device to run on [default: 0]\n"
        b"      --stats-json <FILE>  Write the run's stage timers and counts as one JSON object\n\n"
        b"Output: one TAB-separated line per allele and transcript whose span it meets, the alleles in file order, an allele's\n"
        b"  transcripts in order of first appearance: chrom pos ref alt transcript strand class cds_pos codons aa_pos aa ref_match;\n"
        b"  pos, ref and alt are the file's own.  REF and the piece are trimmed (case folded; the common prefix first, then the common\n"
        b"  suffix); the genome is not consulted, so nothing is left-aligned.  One base against one base is a single-base substitution\n"
        b"  and gets the lines of the command without --indels.  Every other allele covers its reference bases, an insertion the two\n"
        b"  bases around it, and takes the first of: unclassified_model (rows of the transcript overlap), transcript_ablation (the\n"
        b"  whole span is deleted), splice_donor or splice_acceptor (a deletion meets the two bases next to an exon, an insertion lies\n"
        b"  inside them), then in coding sequence partial_codon, start_lost, frameshift, coding_unknown, stop_retained, synonymous,\n"
        b"  stop_gained, stop_lost, inframe_insertion, inframe_deletion or missense, then noncoding_exon, 5_prime_UTR or 3_prime_UTR,\n"
        b"  then intron; intergenic without a transcript.  For these alleles cds_pos and aa_pos are where the change begins in the\n"
        b"  transcribed coding sequence; codons and aa print '.': the residues an in-frame change replaces are not reported.\n"
        b"  ref_match says whether the trimmed REF is the genome's.  Left out, each kind under a warning of its own: '*', '.', symbolic\n"
        b"  and breakend pieces and any other byte; a REF or piece longer than 65535 bytes; a piece equal to REF; an insertion in front\n"
        b"  of a sequence's first base.  --summary has 20 lines.\n")


def case_long_pieces():
    """Pieces of 65 535 bytes over a CDS that holds them (and its minus twin in one row): a deletion of 65 534 bases, an
    insertion of 65 534, a deletion of 65 535 with ref_match over all of them, and 65 535 bases against 65 532 in frame, whose
    windows are 21 845 codons against 21 844."""
    rng = random.Random(9)
    long_ref = bytes(rng.choice(b"ACGT") for _ in range(65535))
    genome = b"G" * 50 + long_ref + b"T" * 80
    ins = bytes(rng.choice(b"ACG") for _ in range(65533)) + b"A"
    rows = [(0, 0, 30, 40, 0), (0, 0, 45, 50 + 65535 + 40, 0), (1, 0, 30, 50 + 65535 + 40, 0)]
    mnv = bytes(b"ACGT"[(b"ACGT".index(b) + 1) % 4] for b in long_ref[:65532])  # (every base another one: first and last differ from R')
    alleles = [(0, 52, long_ref[1:], b""), (0, 51, b"", ins), (0, 51, long_ref, b""), (0, 51, long_ref[:-1] + bytes([long_ref[-1] ^ 6]), b""),
               (0, 51, long_ref, mnv), (0, 49, b"", ins[:3])]
    return [genome], rows, [0, 1 | 2], alleles
