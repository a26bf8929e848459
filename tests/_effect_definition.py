"""The definition of `gffx effect` in plain Python (device/effect_core.hpp is its C++ twin), by brute force: every
transcript against every allele, every segment tested by comparison, no search; Python strings and the dict codon table of
_seq_definition.py.  The tests hold the device, the host check tool and the command to it, bit for bit.

A transcript is a Parent name of CDS and exon lines.  D: its CDS rows by (start, line order); E: its exon rows likewise, or D.
An allele (x, ALT) against a kept transcript whose span [min start, max end] contains x takes the first rule that applies:
  1 coding   x lies in a row of D, the first such row i: xc = (bases of the rows before i) + (x - start_i), q = xc on plus and
             L - 1 - xc on minus; q outside [p, p + 3C) is partial_codon, else codon c = (q - p) // 3, byte k = (q - p) % 3 of the
             transcribed CDS (the rows concatenated, reverse-complemented on minus) and ALT (complemented on minus) in its place
  2 exonic   the last row j of E with start <= x exists and the largest end of rows 0 .. j reaches x: noncoding_exon, or a UTR
             when x lies before the smallest CDS start / behind the largest CDS end
  3 between  intron, or within two bases of the exon edges a < x < b around it: splice_donor / splice_acceptor (left test first)

THE WORKED EXAMPLE (HAND_*).  chrA, 60 bases:

    pos  1 AC GTCA GTAAG CC GATGCTN GTA TAATGG GCA CTTGACAT TTAG CCC ACGTA GGT TTC GA
           1  3    7     12 14      21  24     30  33       41   45  48    53  56  59

  tP (+)  exons 3-6, 12-20, 24-29, 33-44;  CDS 14-20 (phase 1), 24-29, 33-40:  L = 21, p = 1, C = 6
          CDS = G ATG CTN TAA TGG CTT GAC AT -> M X * W L D; q = 0 and q = 19, 20 belong to no codon
  tM (-)  the same lines on the minus strand; the leading segment is 33-40, phase 0:  p = 0, C = 7
          transcribed = revcomp(CDS) = ATG TCA AGC CAT TAN AGC ATC -> M S S H X S I; codon 2 (AGC) lies across 33 | 29,
          codon 4 (TAN) across 24 | 20
  tN (+)  exons 48-52, 56-58, no CDS

    x  REF>ALT   tP                                   tM
    1  A>G       (no transcript: intergenic)
    4  T>C       5_prime_UTR (exon 3-6, before 14)    3_prime_UTR
    7  G>A       splice_donor (6 < 7 <= 8)            splice_acceptor
    9  C>T       intron (REF is not the genome's A: ref_match 0)
   11  G>T       splice_acceptor (11 >= 12 - 2)       splice_donor
   13  C>T       5_prime_UTR (exon 12-20)             3_prime_UTR
   14  G>A       q = 0 < p: partial_codon             q = 20, codon 6 byte 2: ATC>ATT I>I synonymous
   16  T>C       q = 2, codon 0 byte 1: ATG>ACG M>T   q = 18, codon 6 byte 0: ATC>GTC I>V missense
                 missense (p = 1: no start_lost)
   18  C>G       q = 4, codon 1 byte 0: CTN>GTN X>X   q = 16, codon 5 byte 1: AGC>ACC S>T missense
                 coding_unknown
   24  T>C       q = 7, codon 2 byte 0: TAA>CAA *>Q   q = 13, codon 4 byte 1: TAN>TGN X>X coding_unknown
                 stop_lost
   26  A>G       q = 9, codon 2 byte 2: TAA>TAG *>*   q = 11, codon 3 byte 2: CAT>CAC H>H synonymous
                 stop_retained
   29  G>A       q = 12, codon 3 byte 2: TGG>TGA W>*  q = 8, codon 2 byte 2: AGC>AGT S>S synonymous
                 stop_gained
   35  T>C       q = 15, codon 4 byte 2: CTT>CTC L>L  q = 5, codon 1 byte 2: TCA>TCG S>S synonymous
                 synonymous
   39  A>C       q = 19 >= p + 3C: partial_codon      q = 1, codon 0 byte 1: ATG>AGG M>R start_lost
   42  T>A       3_prime_UTR (exon 33-44, behind 40)  5_prime_UTR
   50  G>T       tN: noncoding_exon
   54  G>C       tN: splice_donor (52 < 54 <= 54)
   60  A>T       intergenic
"""
import random

from _seq_definition import CODON, COMPLEMENT, features, parse_fasta, phase_skip, random_genome, revcomp

CLASSES = ("partial_codon", "coding_unknown", "stop_retained", "synonymous", "stop_gained", "stop_lost", "start_lost", "missense",
           "noncoding_exon", "5_prime_UTR", "3_prime_UTR", "intron", "splice_donor", "splice_acceptor", "intergenic")
CODING = CLASSES[1:8]
NO_SEQ = 0xFFFFFFFF


def amino(codon: bytes) -> str:
    return CODON.get(codon.decode("latin-1").upper().replace("U", "T"), "X")


def comp(b: bytes) -> bytes:
    return b.translate(COMPLEMENT)


# ---- transcripts from numeric rows: what the device is handed -----------------------------------------------------------------

def transcripts(seqs, rows, tr_flags):
    """Per transcript a dict (kept, minus, p, seq, D, E, lo, hi), D and E lists of (start - 1, end); rows: (transcript, sequence
    number, start - 1, end, kind) in input order, kind 0 CDS and 1 exon; tr_flags: minus | phase << 1 | 8 (dropped by the caller)."""
    per = [[] for _ in tr_flags]
    for k, (t, q, s, e, kind) in enumerate(rows):
        per[t].append((k, q, s, e, kind))
    out = []
    for t, fl in enumerate(tr_flags):
        m = per[t]
        sq = m[0][1]
        kept = not fl & 8 and all(x[1] == sq for x in m) and sq < len(seqs) and all(x[3] <= len(seqs[sq]) for x in m)
        order = sorted(m, key=lambda x: (x[2], x[0]))
        D = [(x[2], x[3]) for x in order if x[4] == 0]
        E = [(x[2], x[3]) for x in order if x[4] == 1] or D
        out.append(dict(kept=kept, minus=bool(fl & 1), p=(fl >> 1) & 3, seq=sq, D=D, E=E, lo=min(x[2] for x in m) + 1, hi=max(x[3] for x in m)))
    return out


def classify(tr, seq: bytes, x: int, alt: bytes):
    """(class, q, c, k, codon_ref, codon_alt, aa_ref, aa_alt) of allele (x, alt) against kept transcript tr whose span contains
    x; the fields a class does not fill are 0 / b"" / ""."""
    D, E, minus, p = tr["D"], tr["E"], tr["minus"], tr["p"]
    none = (0, 0, 0, b"", b"", "", "")
    for i, (s, e) in enumerate(D):
        if s < x <= e:
            L = sum(b - a for a, b in D)
            xc = sum(b - a for a, b in D[:i]) + (x - 1 - s)
            q = L - 1 - xc if minus else xc
            C = (L - p) // 3 if L > p else 0
            if q < p or q >= p + 3 * C:
                return ("partial_codon", q) + none[1:]
            c, k = divmod(q - p, 3)
            cds = b"".join(seq[a:b] for a, b in D)
            if minus:
                cds = revcomp(cds)
            ref = cds[p + 3 * c:p + 3 * c + 3]
            new = ref[:k] + (comp(alt) if minus else alt) + ref[k + 1:]
            ra, aa = amino(ref), amino(new)
            if "X" in (ra, aa):
                cls = "coding_unknown"
            elif ra == aa:
                cls = "stop_retained" if ra == "*" else "synonymous"
            elif aa == "*":
                cls = "stop_gained"
            elif ra == "*":
                cls = "stop_lost"
            elif c == 0 and p == 0 and ra == "M":
                cls = "start_lost"
            else:
                cls = "missense"
            return (cls, q, c, k, ref, new, ra, aa)
    js = [j for j, (s, e) in enumerate(E) if s < x]
    j = max(js) if js else None
    if j is not None and max(e for s, e in E[:j + 1]) >= x:
        if not D:
            return ("noncoding_exon",) + none
        cmin, cmax = min(s for s, e in D) + 1, max(e for s, e in D)
        if x < cmin:
            return ("3_prime_UTR" if minus else "5_prime_UTR",) + none
        if x > cmax:
            return ("5_prime_UTR" if minus else "3_prime_UTR",) + none
        return ("noncoding_exon",) + none
    if j is None or j + 1 == len(E):
        return ("intron",) + none
    a, b = max(e for s, e in E[:j + 1]), E[j + 1][0] + 1
    assert a < x < b
    if x <= a + 2:
        return ("splice_acceptor" if minus else "splice_donor",) + none
    if x >= b - 2:
        return ("splice_donor" if minus else "splice_acceptor",) + none
    return ("intron",) + none


def ref_match(seqs, q, x, ref) -> int:
    if q >= len(seqs) or x > len(seqs[q]):
        return 0
    return 1 if seqs[q][x - 1:x].upper() == bytes([ref]).upper() else 0


def pairs(seqs, rows, tr_flags, alleles):
    """(offsets, ref_match, records) for alleles (sequence number, x, REF | ALT << 8): records (transcript, class, q, c, k,
    codon_ref, codon_alt, aa_ref, aa_alt, ref_match), the alleles in order, an allele's transcripts by number."""
    trs = transcripts(seqs, rows, tr_flags)
    off, rms, recs = [0], [], []
    for q, x, ra in alleles:
        rm = ref_match(seqs, q, x, ra & 255)
        rms.append(rm)
        for t, tr in enumerate(trs):
            if tr["kept"] and tr["seq"] == q and tr["lo"] <= x <= tr["hi"] and x <= len(seqs[q]):
                recs.append((t,) + classify(tr, seqs[q], x, bytes([ra >> 8])) + (rm,))
        off.append(len(recs))
    return off, rms, recs


def dropped(seqs, rows, tr_flags):
    return [0 if tr["kept"] else 1 for tr in transcripts(seqs, rows, tr_flags)]


def device_records(recs):
    """The records as the device's 32-byte structs give them: (q, c, transcript, class number, k, ref_match, aa_ref, aa_alt,
    codon_ref, codon_alt)."""
    out = []
    for t, cls, q, c, k, cr, ca, ar, aa, rm in recs:
        out.append((q, c, t, CLASSES.index(cls), k, rm, ord(ar) if ar else 0, ord(aa) if aa else 0, tuple(cr) if cr else (0, 0, 0), tuple(ca) if ca else (0, 0, 0)))
    return out


# ---- the command: transcripts from GFF text, alleles from VCF text, the table it writes --------------------------------------

class VcfError(ValueError):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what))
        self.line, self.what = line, what


def parse_vcf(data: bytes):
    """(alleles, not_snv): alleles (line number, chrom, x, ref, alt piece) of the taken ones, in file order."""
    out, not_snv = [], 0
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
            raise VcfError(n, "fewer than 5 fields")
        if not (1 <= len(f[1]) <= 10 and f[1].isdigit() and 1 <= int(f[1]) <= 2 ** 32 - 1):
            raise VcfError(n, "POS")
        for piece in f[4].split(b","):
            if len(f[3]) == 1 and len(piece) == 1 and f[3] in b"ACGTNacgtn" and piece in b"ACGTNacgtn":
                out.append((n, f[0], int(f[1]), f[3], piece))
            else:
                not_snv += 1
    return out, not_snv


def gff_seqids(gff: bytes):
    """The seqids the index knows: column 1 of every feature line."""
    ids = []
    for line in gff.split(b"\n"):
        f = line.split(b"\t")
        if line.startswith(b"#") or len(f) < 9 or f[0] in ids:
            continue
        ids.append(f[0])
    return ids


def gff_transcripts(gff: bytes, names, seqs, cds_type="CDS", exon_type="exon"):
    """(rows, tr_flags, transcript names, strands, counts) for pairs(): what the command hands to the device.  Sequence numbers
    are the FASTA's (NO_SEQ for a seqid it lacks).  The lines are taken as _seq_definition.features takes them, one by one."""
    number = {n.decode("latin-1"): i for i, n in enumerate(names)}
    feats = []
    for line in gff.split(b"\n"):
        for f in features(line, (cds_type, exon_type)):
            f["kind"] = 0 if line.split(b"\t")[2].decode("latin-1") == cds_type else 1
            feats.append(f)
    cnt = dict(orphans=0, mixed=0, unservable=0)
    by_name, members, rows = {}, [], []
    for k, f in enumerate(feats):
        if not f["parents"]:
            cnt["orphans"] += 1
        for name in f["parents"]:
            t = by_name.setdefault(name, len(by_name))
            if t == len(members):
                members.append([])
            members[t].append((k, f))
            rows.append((t, number.get(f["seqid"], NO_SEQ), f["start"] - 1, f["end"], f["kind"]))
    flags, strands = [], []
    for m in members:
        first = m[0][1]
        mixed = any(f["seqid"] != first["seqid"] or f["minus"] != first["minus"] for _, f in m)
        cds = sorted(((k, f) for k, f in m if f["kind"] == 0), key=lambda x: (x[1]["start"], x[0]))
        lead = (cds[-1][1] if first["minus"] else cds[0][1]) if cds else None
        flags.append((1 if first["minus"] else 0) | (phase_skip(lead["phase"]) if lead else 0) << 1 | (8 if mixed else 0))
        strands.append("-" if first["minus"] else "+")
        cnt["mixed"] += mixed
    trs = transcripts(seqs, rows, flags)
    cnt["unservable"] = sum(1 for fl, tr in zip(flags, trs) if not fl & 8 and not tr["kept"])
    return rows, flags, list(by_name), strands, cnt


def render(gff: bytes, fasta: bytes, vcf: bytes, cds_type="CDS", exon_type="exon"):
    """(the table, the summary, counts) of `gffx effect`; counts: not_snv, no_chrom, orphans, mixed, unservable."""
    names, seqs = parse_fasta(fasta)
    number = {n: i for i, n in enumerate(names)}
    known = set(gff_seqids(gff))
    rows, flags, tnames, strands, cnt = gff_transcripts(gff, names, seqs, cds_type, exon_type)
    taken, cnt["not_snv"] = parse_vcf(vcf)
    cnt["no_chrom"] = sum(1 for a in taken if a[1] not in known)
    taken = [a for a in taken if a[1] in known]
    alleles = [(number.get(chrom, NO_SEQ), x, ref[0] | alt[0] << 8) for _, chrom, x, ref, alt in taken]
    off, rms, recs = pairs(seqs, rows, flags, alleles)
    out = ["#chrom\tpos\tref\talt\ttranscript\tstrand\tclass\tcds_pos\tcodons\taa_pos\taa\tref_match\n"]
    n_alleles, n_pairs = {c: 0 for c in CLASSES}, {c: 0 for c in CLASSES}
    for i, (_, chrom, x, ref, alt) in enumerate(taken):
        head = "%s\t%d\t%s\t%s\t" % (chrom.decode("latin-1"), x, ref.decode(), alt.decode())
        if off[i] == off[i + 1]:
            out.append(head + ".\t.\tintergenic\t.\t.\t.\t.\t%d\n" % rms[i])
            n_alleles["intergenic"] += 1
            n_pairs["intergenic"] += 1
        seen = set()
        for t, cls, q, c, k, cr, ca, ar, aa, rm in recs[off[i]:off[i + 1]]:
            coding = "%d\t%s>%s\t%d\t%s>%s" % (q + 1, cr.upper().decode("latin-1"), ca.upper().decode("latin-1"), c + 1, ar, aa) if cls in CODING else ".\t.\t.\t."
            out.append(head + "%s\t%s\t%s\t%s\t%d\n" % (tnames[t], strands[t], cls, coding, rm))
            n_pairs[cls] += 1
            if cls not in seen:
                n_alleles[cls] += 1
                seen.add(cls)
    summary = "".join("%s\t%d\t%d\n" % (c, n_alleles[c], n_pairs[c]) for c in CLASSES)
    return "".join(out).encode("latin-1"), summary.encode(), cnt


# ---- random inputs ----------------------------------------------------------------------------------------------------------------

def random_case(seed, n_seq=2, seq_len=(300, 180), n_tr=12, n_alleles=200, alphabet=b"ACGTACGTACGTacgtN", max_segments=5, bad=True,
                kinds=("coding", "coding", "coding+exons", "coding+utr", "noncoding", "messy"), gaps=(1, 2, 3, 4, 5, 6)):
    """(seqs, rows, tr_flags, alleles): transcripts of 1 .. max_segments CDS segments with gaps of 1 .. 6 bases, UTR exons on
    some, exon lines missing on some, non-coding ones, duplicates and overlaps, every phase, both strands; with `bad`, some
    dropped: by the caller, on two sequences, on a missing sequence, beyond the end.  Without the kind "messy" no two rows of a
    kind overlap."""
    rng = random.Random(seed)
    seqs = [bytes(rng.choice(alphabet) for _ in range(n)) for n in seq_len[:n_seq]]
    rows, flags = [], []
    for t in range(n_tr):
        q = rng.randrange(n_seq)
        n = len(seqs[q])
        at = rng.randrange(1, max(2, n // 2))
        segs = []
        for _ in range(rng.randint(1, max_segments)):
            ln = rng.choice((1, 1, 2, 3, 4, 7, 11))
            if at + ln > n:
                break
            segs.append((at - 1, at - 1 + ln))
            at += ln + rng.choice(gaps)
        if not segs:
            segs = [(0, min(3, n))]
        kind = rng.choice(kinds)
        mine = []
        if kind == "noncoding":
            mine = [(s, e, 1) for s, e in segs]
        else:
            mine = [(s, e, 0) for s, e in segs]
            if kind == "coding+exons":
                mine += [(s, e, 1) for s, e in segs]
            elif kind == "coding+utr":
                mine += [(max(0, s - rng.randint(0, 3)) if i == 0 else s, min(n, e + rng.randint(0, 3)) if i + 1 == len(segs) else e, 1) for i, (s, e) in enumerate(segs)]
                if segs[0][0] > 8:
                    mine.append((segs[0][0] - 8, segs[0][0] - 5, 1))
            elif kind == "messy":
                mine += [mine[0], (segs[0][0], min(n, segs[0][1] + 2), 0)]
                mine += [(s, min(n, e + 1), 1) for s, e in segs[::2]]
        rng.shuffle(mine)
        fl = rng.randrange(2) | rng.randrange(3) << 1
        seq_of = [q] * len(mine)
        if bad and rng.random() < 0.25:
            how = rng.choice(("caller", "mixed", "missing", "beyond"))
            if how == "caller":
                fl |= 8
            elif how == "mixed" and n_seq > 1 and len(mine) > 1:
                seq_of[-1] = (q + 1) % n_seq
            elif how == "missing":
                seq_of = [NO_SEQ] * len(mine)
            elif how == "beyond":
                mine[-1] = (mine[-1][0], n + 1, mine[-1][2])
        rows += [(t, sq, s, e, k) for sq, (s, e, k) in zip(seq_of, mine)]
        flags.append(fl)
    alleles = []
    for _ in range(n_alleles):
        q = rng.randrange(n_seq)
        x = rng.randint(1, len(seqs[q]))
        ref = seqs[q][x - 1] if rng.random() < 0.8 else rng.choice(b"ACGTN")
        alleles.append((q, x, ref | rng.choice(b"ACGTNacgt") << 8))
    return seqs, rows, flags, alleles


def random_files(seed, crlf=False):
    """(gff, fasta, vcf): a small random annotation with Parent lists, orphans, transcripts on two strands or seqids, on a seqid
    the FASTA lacks and beyond a sequence's end; variants with several ALT pieces, indels, an unknown CHROM."""
    rng = random.Random(seed)
    fasta, seqs = random_genome(seed, names=("chrA", "chrB"), lengths=(400, 250), alphabet=b"ACGTACGTacgtNn")
    lens = {"chrA": 400, "chrB": 250, "chrC": 300}
    lines, spots = ["##gff-version 3"], []
    for t in range(16):
        chrom = rng.choice(("chrA", "chrA", "chrB", "chrC"))
        strand = rng.choice("+-")
        at = rng.randrange(1, lens[chrom] - 120)
        hi = lens[chrom]
        mine = []
        for k in range(rng.randrange(1, 6)):
            ln = rng.choice((1, 2, 3, 5, 8, 13))
            if at + ln > hi:
                break
            parent = "t%d" % t if rng.random() < 0.9 else "t%d,,t%d" % (t, (t + 1) % 16)
            if rng.random() < 0.8:
                mine.append("%s\tr\tCDS\t%d\t%d\t.\t%s\t%s\tID=c%d.%d;Parent=%s" % (chrom, at, at + ln - 1, strand, rng.choice(".012"), t, k, parent))
            if rng.random() < 0.7:
                lo = at - rng.choice((0, 0, 2)) if at > 2 else at
                mine.append("%s\tr\texon\t%d\t%d\t.\t%s\t.\tParent=%s;ID=e%d.%d" % (chrom, lo, at + ln - 1 + rng.choice((0, 0, 3)), strand, parent, t, k))
            spots.append((chrom, at, at + ln - 1))
            at += ln + rng.choice((1, 2, 3, 4, 5, 9))
        if t == 3 and mine:
            mine.append(mine[0].replace("\t%s\t" % strand, "\t%s\t" % ("+" if strand == "-" else "-"), 1))
        if t == 5:
            mine.append("chrA\tr\texon\t3\t9\t.\t+\t.\tID=orphan")
        if t == 7:
            mine.append("%s\tr\texon\t%d\t%d\t.\t%s\t.\tID=far;Parent=t7" % (chrom, lens[chrom] - 5, lens[chrom] + 10, strand))
        rng.shuffle(mine)
        lines += mine
    lines.append("chrD\tr\tgene\t1\t5\t.\t+\t.\tID=lonely")
    vcf = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL"]
    for _ in range(250):
        chrom = rng.choice(("chrA", "chrA", "chrB", "chrC", "chrD", "chrZ"))
        x = rng.randint(1, lens.get(chrom, 50) + 3)
        if rng.random() < 0.7:  # (near a member line)
            chrom, lo, hi = rng.choice(spots)
            x = max(1, rng.randint(lo - 4, hi + 4))
        alts = ",".join(rng.choice(("A", "C", "G", "T", "a", "N", "AT", "<DEL>", "*")) for _ in range(rng.choice((1, 1, 1, 2, 3))))
        vcf.append("%s\t%d\t.\t%s\t%s\t50" % (chrom, x, rng.choice(("A", "C", "G", "T", "n", "AC")), alts))
    nl = "\r\n" if crlf else "\n"
    return (nl.join(lines) + nl).encode(), fasta.replace(b"\n", b"\r\n") if crlf else fasta, (nl.join(vcf) + nl).encode()



# ---- the worked example -------------------------------------------------------------------------------------------------------------
HAND_CHRA = b"AC" b"GTCA" b"GTAAG" b"CC" b"GATGCTN" b"GTA" b"TAATGG" b"GCA" b"CTTGACAT" b"TTAG" b"CCC" b"ACGTA" b"GGT" b"TTC" b"GA"
HAND_FASTA = b">chrA hand example\n" + HAND_CHRA[:25] + b"\n" + HAND_CHRA[25:] + b"\n"


def _hand_gff():
    out = ["##gff-version 3\n"]
    for name, strand, phases in (("tP", "+", "1 0 0"), ("tM", "-", "2 1 0")):
        out.append("chrA\th\tmRNA\t3\t44\t.\t%s\t.\tID=%s\n" % (strand, name))
        for s, e in ((3, 6), (12, 20), (24, 29), (33, 44)):
            out.append("chrA\th\texon\t%d\t%d\t.\t%s\t.\tID=%s.e%d;Parent=%s\n" % (s, e, strand, name, s, name))
        for (s, e), ph in zip(((14, 20), (24, 29), (33, 40)), phases.split()):
            out.append("chrA\th\tCDS\t%d\t%d\t.\t%s\t%s\tID=%s.c%d;Parent=%s\n" % (s, e, strand, ph, name, s, name))
    out.append("chrA\th\tlnc_RNA\t48\t58\t.\t+\t.\tID=tN\n")
    out.append("chrA\th\texon\t48\t52\t.\t+\t.\tID=tN.e1;Parent=tN\n")
    out.append("chrA\th\texon\t56\t58\t.\t+\t.\tParent=tN;ID=tN.e2\n")
    return "".join(out).encode()


HAND_GFF = _hand_gff()
HAND_VCF = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n"
            b"chrA\t1\t.\tA\tG\nchrA\t4\t.\tT\tC\nchrA\t7\t.\tG\tA\nchrA\t9\t.\tC\tT\nchrA\t11\t.\tG\tT\nchrA\t13\t.\tC\tT\n"
            b"chrA\t14\t.\tG\tA\nchrA\t16\t.\tT\tC\nchrA\t18\t.\tC\tG\nchrA\t24\t.\tT\tC\nchrA\t26\t.\tA\tG\nchrA\t29\t.\tG\tA\n"
            b"chrA\t35\t.\tT\tC\nchrA\t39\t.\tA\tC\nchrA\t42\t.\tT\tA\nchrA\t50\t.\tG\tT\nchrA\t54\t.\tG\tC\nchrA\t60\t.\tA\tT\n")
# pos ref alt, then per transcript hit: name strand class cds_pos codons aa_pos aa; ref_match last
_HAND = """
1 A G | 1
4 T C tP + 5_prime_UTR . . . . tM - 3_prime_UTR . . . . | 1
7 G A tP + splice_donor . . . . tM - splice_acceptor . . . . | 1
9 C T tP + intron . . . . tM - intron . . . . | 0
11 G T tP + splice_acceptor . . . . tM - splice_donor . . . . | 1
13 C T tP + 5_prime_UTR . . . . tM - 3_prime_UTR . . . . | 1
14 G A tP + partial_codon . . . . tM - synonymous 21 ATC>ATT 7 I>I | 1
16 T C tP + missense 3 ATG>ACG 1 M>T tM - missense 19 ATC>GTC 7 I>V | 1
18 C G tP + coding_unknown 5 CTN>GTN 2 X>X tM - missense 17 AGC>ACC 6 S>T | 1
24 T C tP + stop_lost 8 TAA>CAA 3 *>Q tM - coding_unknown 14 TAN>TGN 5 X>X | 1
26 A G tP + stop_retained 10 TAA>TAG 3 *>* tM - synonymous 12 CAT>CAC 4 H>H | 1
29 G A tP + stop_gained 13 TGG>TGA 4 W>* tM - synonymous 9 AGC>AGT 3 S>S | 1
35 T C tP + synonymous 16 CTT>CTC 5 L>L tM - synonymous 6 TCA>TCG 2 S>S | 1
39 A C tP + partial_codon . . . . tM - start_lost 2 ATG>AGG 1 M>R | 1
42 T A tP + 3_prime_UTR . . . . tM - 5_prime_UTR . . . . | 1
50 G T tN + noncoding_exon . . . . | 1
54 G C tN + splice_donor . . . . | 1
60 A T | 1
"""


def _hand_out():
    out = ["#chrom\tpos\tref\talt\ttranscript\tstrand\tclass\tcds_pos\tcodons\taa_pos\taa\tref_match\n"]
    for line in _HAND.strip().split("\n"):
        left, rm = line.split("|")
        w = left.split()
        head = "chrA\t%s\t%s\t%s\t" % tuple(w[:3])
        hits = [w[i:i + 7] for i in range(3, len(w), 7)]
        if not hits:
            out.append(head + ".\t.\tintergenic\t.\t.\t.\t.\t" + rm.strip() + "\n")
        for h in hits:
            out.append(head + "\t".join(h) + "\t" + rm.strip() + "\n")
    return "".join(out).encode()


HAND_OUT = _hand_out()
