"""The definition of `gffx seq` in plain Python (device/seq_core.hpp is its C++ twin): string slicing, a dict codon
table built from the 64-letter string of NCBI table 1, a translation-table complement.  The tests hold the device, the host check
tool and the command to it, bit for bit.

FASTA: a line ends at "\\n", a "\\r" directly before it is not part of it; empty lines are ignored; ">" opens a sequence named up
to the first blank, TAB or line end; every other line adds all of its bytes as they are.  A feature's bases are positions
start .. end (1-based, inclusive) of the sequence named like its seqid; a minus feature is the reverse complement.  With join, a
record per Parent name in order of first appearance: its segments by (start, line order), concatenated, reverse-complemented as a
whole on minus; dropped whole when a member is on another seqid or strand than the first, or cannot be served.  translate: skip
the phase of the first segment in transcription order, read codons of three, drop the rest.  The body is the characters in lines
of W ("\\n" after each; W = 0: one line; no characters: no line)."""
import random

_PAIRS = "AT CG RY KM BV DH"
_FROM = "".join(a + b for a, b in _PAIRS.split()) + "U" + "SWN"
_TO = "".join(b + a for a, b in _PAIRS.split()) + "A" + "SWN"
COMPLEMENT = bytes.maketrans((_FROM + _FROM.lower()).encode(), (_TO + _TO.lower()).encode())

TABLE1 = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODON = {a + b + c: TABLE1[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}


class FastaError(ValueError):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what))
        self.line, self.what = line, what


def parse_fasta(data: bytes):
    """(names, sequences) in file order; FastaError names the line (1-based) of the first error."""
    names, seqs, seen = [], [], set()
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # (the text ended with "\n": no further line)
    n = len(lines)
    for i, line in enumerate(lines):
        terminated = i + 1 < n or data.endswith(b"\n")
        if terminated and line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        if line.startswith(b">"):
            name = line[1:].split(b" ")[0].split(b"\t")[0]
            if not name:
                raise FastaError(i + 1, "no name")
            if name in seen:
                raise FastaError(i + 1, "twice")
            seen.add(name)
            names.append(name)
            seqs.append([])
        elif not names:
            raise FastaError(i + 1, "before the first >")
        else:
            seqs[-1].append(line)
    return names, [b"".join(s) for s in seqs]


def revcomp(s: bytes) -> bytes:
    return s.translate(COMPLEMENT)[::-1]


def phase_skip(col8) -> int:
    return {"1": 1, "2": 2, b"1": 1, b"2": 2, 1: 1, 2: 2}.get(col8, 0)


def translate(bases: bytes, p: int = 0) -> bytes:
    s = bases[p:].decode("latin-1").upper().replace("U", "T")
    return "".join(CODON.get(s[i:i + 3], "X") for i in range(0, len(s) - 2, 3)).encode()


def wrap(chars: bytes, w: int) -> bytes:
    if not chars:
        return b""
    if w == 0:
        return chars + b"\n"
    return b"".join(chars[i:i + w] + b"\n" for i in range(0, len(chars), w))


def body_bytes(c: int, w: int) -> int:
    return 0 if c == 0 else c + 1 if w == 0 else c + -(-c // w)


# ---- records from numeric rows: what the device is handed -------------------------------------------------------------------

def record_chars(seqs, segments, minus, p, translated):
    """The characters of one record, or None when a member cannot be served.  seqs: the sequences by number; segments:
    (sequence number, start - 1, end) in input order."""
    parts = []
    for k, (q, s, e) in sorted(enumerate(segments), key=lambda x: (x[1][1], x[0])):
        if q >= len(seqs) or e > len(seqs[q]):
            return None
        parts.append(seqs[q][s:e])
    bases = b"".join(parts)
    if minus:
        bases = revcomp(bases)
    return translate(bases, p) if translated else bases


def bodies(seqs, rows, rec_flags, translated, w):
    """(the concatenated bodies, body_off, dropped) for rows (record, sequence number, start - 1, end) and per record
    flags = minus | phase << 1 | 8 (dropped by the caller)."""
    per = [[] for _ in rec_flags]
    for r, q, s, e in rows:
        per[r].append((q, s, e))
    out, off, dropped = [], [0], []
    for r, fl in enumerate(rec_flags):
        chars = None if fl & 8 else record_chars(seqs, per[r], bool(fl & 1), (fl >> 1) & 3, translated)
        dropped.append(1 if chars is None else 0)
        out.append(wrap(chars or b"", w))
        off.append(off[-1] + len(out[-1]))
    return b"".join(out), off, dropped


# ---- the command: features from GFF text, the FASTA file it writes ---------------------------------------------------------------

def _attr(col9: str, key: str):
    for item in col9.split(";"):
        if item.startswith(key + "="):
            return item[len(key) + 1:]
    return None


def features(gff: bytes, types):
    """The lines of the types with 1 <= start <= end, in file order."""
    out = []
    for line in gff.decode("latin-1").split("\n"):
        line = line[:-1] if line.endswith("\r") else line
        f = line.split("\t")
        if line.startswith("#") or len(f) < 8 or f[2] not in types:
            continue
        try:
            start, end = int(f[3]), int(f[4])
        except ValueError:
            continue
        if not 1 <= start <= end:
            continue
        col9 = f[8] if len(f) > 8 else ""
        parent = _attr(col9, "Parent") or ""
        out.append(dict(seqid=f[0], start=start, end=end, minus=f[6] == "-", strand=f[6] if f[6] in "+-" and len(f[6]) == 1 else ".",
                        phase=f[7], id=_attr(col9, "ID") or ".", parents=[x for x in parent.split(",") if x]))
    return out


def render(gff: bytes, fasta: bytes, types=("exon",), join=False, translated=False, w=60):
    """(the output file, counts) of `gffx seq`; counts: no_seq, beyond, orphans, mixed, unservable."""
    names, seqs = parse_fasta(fasta)
    genome = dict(zip((n.decode("latin-1") for n in names), seqs))
    feats = features(gff, types)
    cnt = dict(no_seq=0, beyond=0, orphans=0, mixed=0, unservable=0)

    def served(f):
        return f["seqid"] in genome and f["end"] <= len(genome[f["seqid"]])

    for f in feats:
        if f["seqid"] not in genome:
            cnt["no_seq"] += 1
        elif f["end"] > len(genome[f["seqid"]]):
            cnt["beyond"] += 1
    out = []
    if not join:
        for f in feats:
            if not served(f):
                continue
            bases = genome[f["seqid"]][f["start"] - 1:f["end"]]
            bases = revcomp(bases) if f["minus"] else bases
            chars = translate(bases, phase_skip(f["phase"])) if translated else bases
            out.append((">%s %s:%d-%d(%s)\n" % (f["id"], f["seqid"], f["start"], f["end"], f["strand"])).encode("latin-1") + wrap(chars, w))
        return b"".join(out), cnt
    recs = {}
    for k, f in enumerate(feats):
        if not f["parents"]:
            cnt["orphans"] += 1
        for name in f["parents"]:
            recs.setdefault(name, []).append((k, f))
    for name, members in recs.items():  # (a dict keeps the order of first appearance)
        first = members[0][1]
        if any(f["seqid"] != first["seqid"] or f["minus"] != first["minus"] for _, f in members):
            cnt["mixed"] += 1
            continue
        if not all(served(f) for _, f in members):
            cnt["unservable"] += 1
            continue
        order = sorted(members, key=lambda m: (m[1]["start"], m[0]))
        bases = b"".join(genome[f["seqid"]][f["start"] - 1:f["end"]] for _, f in order)
        lead = order[0][1]
        if first["minus"]:
            bases, lead = revcomp(bases), order[-1][1]
        chars = translate(bases, phase_skip(lead["phase"])) if translated else bases
        head = ">%s %s:%d-%d(%s) segments=%d\n" % (name, first["seqid"], min(f["start"] for _, f in members), max(f["end"] for _, f in members),
                                                     first["strand"], len(members))
        out.append(head.encode("latin-1") + wrap(chars, w))
    return b"".join(out), cnt


def random_genome(seed, names=("chrA", "chrB"), lengths=(400, 250), alphabet=b"ACGTacgtNnRYKMBVDHSWU", width=None):
    """(the FASTA text, the sequences) with ragged line lengths (or lines of `width`)."""
    rng = random.Random(seed)
    text, seqs = [], []
    for name, n in zip(names, lengths):
        s = bytes(rng.choice(alphabet) for _ in range(n))
        seqs.append(s)
        text.append(b">" + name.encode() + b" some description\n")
        at = 0
        while at < n:
            k = width or rng.choice((1, 2, 7, 60, 61, 80))
            text.append(s[at:at + k] + b"\n")
            at += k
    return b"".join(text), seqs


# ---- the worked example, its answers written out by hand ---------------------------------------------------------------------
HAND_FASTA = b">chrA x\nACGTACGTAC\nGTTTGACCAT\n>chrB\nttgcaN\n"
HAND_CHRA = b"ACGTACGTACGTTTGACCAT"
HAND_GFF = (b"##gff-version 3\n"
            b"chrA\tt\tgene\t2\t12\t.\t+\t.\tID=g1\n"
            b"chrA\tt\tmRNA\t2\t12\t.\t+\t.\tID=t1;Parent=g1\n"
            b"chrA\tt\texon\t9\t12\t.\t+\t.\tID=e2;Parent=t1\n"
            b"chrA\tt\texon\t2\t4\t.\t+\t.\tID=e1;Parent=t1\n"
            b"chrA\tt\tCDS\t2\t4\t.\t+\t1\tID=c1;Parent=t1\n"
            b"chrA\tt\tCDS\t9\t12\t.\t+\t0\tID=c1;Parent=t1\n"
            b"chrA\tt\tgene\t15\t20\t.\t-\t.\tID=g2\n"
            b"chrA\tt\tmRNA\t15\t20\t.\t-\t.\tID=t2;Parent=g2\n"
            b"chrA\tt\texon\t15\t17\t.\t-\t.\tID=e3;Parent=t2\n"
            b"chrA\tt\texon\t19\t20\t.\t-\t.\tParent=t2;ID=e4\n"
            b"chrB\tt\tregion\t1\t6\t.\t.\t.\tName=whole\n"
            b"chrB\tt\tgene\t1\t6\t.\t-\t.\tID=gB\n"
            b"chrB\tt\tgene\t1\t7\t.\t-\t.\tID=gLong\n")
HAND_T1_JOINED, HAND_T1_PHASE0, HAND_T1_PHASE1 = b"CGTACGT", b"RT", b"VR"
HAND_T2_JOINED, HAND_T2_TRANSLATED = b"ATGTC", b"M"
HAND_CHRB_MINUS = b"Ntgcaa"
# gffx seq -j (exons): t1 then t2, by first appearance
HAND_JOIN = b">t1 chrA:2-12(+) segments=2\nCGTACGT\n>t2 chrA:15-20(-) segments=2\nATGTC\n"
# gffx seq (exons, one record per line, file order)
HAND_PLAIN = b">e2 chrA:9-12(+)\nACGT\n>e1 chrA:2-4(+)\nCGT\n>e3 chrA:15-17(-)\nGTC\n>e4 chrA:19-20(-)\nAT\n"
# gffx seq -j --translate -T CDS: the first segment in transcription order is 2-4, phase 1
HAND_CDS_TRANSLATED = b">t1 chrA:2-12(+) segments=2\nVR\n"
# gffx seq -T gene -w 4: gLong reaches beyond chrB and gives no record
HAND_GENES_W4 = b">g1 chrA:2-12(+)\nCGTA\nCGTA\nCGT\n>g2 chrA:15-20(-)\nATGG\nTC\n>gB chrB:1-6(-)\nNtgc\naa\n"
# gffx seq -T region: a line without ID (the index skips that type, so it may have none) and without a strand
HAND_REGION = b">. chrB:1-6(.)\nttgcaN\n"
