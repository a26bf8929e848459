"""`gffx effect` where no GPU is needed: the definition (tests/_effect_definition.py) on the worked example with its hand-written
answers and under its two laws on random inputs; device/effect_core.hpp and host/effect_text.hpp in their host build under
AddressSanitizer + UndefinedBehaviorSanitizer (tools/effect_check.cpp, a stand-alone program) on every class, all 64 codons x 3
positions x 4 alternates, the first and the last base of a sequence, coordinates at 2^32 - 1, an L beyond 2^32, gaps of 1 to 5
bases, every phase against every L - p mod 3, duplicate and overlapping CDS segments and transcripts without exon lines; the
variants file in any number of parts; the whole command on one core against the definition."""
import os
import random
import subprocess

import pytest

import _effect_definition as D
import _seq_definition as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "effect_check")
BIG = 2 ** 32 - 1


# ---- the definition -----------------------------------------------------------------------------------------------------

def test_the_worked_example():
    out, summary, cnt = D.render(D.HAND_GFF, D.HAND_FASTA, D.HAND_VCF)
    assert out == D.HAND_OUT and not any(cnt.values())
    classes = [line.split(b"\t")[6].decode() for line in D.HAND_OUT.split(b"\n")[1:-1]]
    assert set(classes) == set(D.CLASSES)  # alleles that land on every class name at least once
    rows = dict(line.split("\t")[0:1] + [tuple(int(v) for v in line.split("\t")[1:])] for line in summary.decode().split("\n")[:-1])
    assert list(rows) == list(D.CLASSES) and rows["synonymous"] == (4, 5) and rows["intergenic"] == (2, 2) and rows["intron"] == (1, 2)
    assert sum(p for _, p in rows.values()) == len(classes)


def _clean(seed, **kw):
    return D.random_case(seed, kinds=("coding", "coding", "coding+exons", "noncoding"), gaps=(4, 5, 6, 9), bad=False, alphabet=b"ACGTACGTacgtN", **kw)


@pytest.mark.parametrize("seed", range(5))
def test_the_mirror_law(seed):
    """Reverse-complement the genome and mirror every coordinate and strand: every pair keeps its class, cds_pos, codons and
    amino acids.  (Transcripts whose rows do not overlap and whose gaps have four bases or more: "the first such segment" and
    "the left test is made first" are not symmetric.)"""
    seqs, rows, flags, alleles = _clean(40 + seed)
    n = [len(s) for s in seqs]
    m_seqs = [S.revcomp(s) for s in seqs]
    m_rows = [(t, q, n[q] - e, n[q] - s, k) for t, q, s, e, k in rows]
    m_flags = [f ^ 1 for f in flags]
    m_alleles = [(q, n[q] + 1 - x, D.comp(bytes([ra & 255]))[0] | D.comp(bytes([ra >> 8]))[0] << 8) for q, x, ra in alleles]
    off, rm, recs = D.pairs(seqs, rows, flags, alleles)
    m_off, m_rm, m_recs = D.pairs(m_seqs, m_rows, m_flags, m_alleles)
    assert off == m_off and rm == m_rm and len(recs) > 50
    assert recs == m_recs  # (transcript, class, q, c, k, both codons, both amino acids, ref_match)
    assert len({r[1] for r in recs}) >= 8


@pytest.mark.parametrize("seed", range(5))
def test_the_protein_law(seed):
    """For every coding pair the translated record of the transcript over the genome with ALT written in differs from the
    original's at character c exactly as aa says, and nowhere else."""
    seqs, rows, flags, alleles = _clean(60 + seed, n_tr=20, n_alleles=500)
    _, _, recs = D.pairs(seqs, rows, flags, alleles)
    off, _, _ = D.pairs(seqs, rows, flags, alleles)
    n_coding = 0
    for i, (q, x, ra) in enumerate(alleles):
        for t, cls, _, c, _, _, _, aa_ref, aa_alt, _ in recs[off[i]:off[i + 1]]:
            if cls not in D.CODING:
                continue
            edited = list(seqs)
            edited[q] = seqs[q][:x - 1] + bytes([ra >> 8]) + seqs[q][x:]
            cds = [(qq, s, e) for tt, qq, s, e, k in rows if tt == t and k == 0]
            a = S.record_chars(seqs, cds, bool(flags[t] & 1), (flags[t] >> 1) & 3, True)
            b = S.record_chars(edited, cds, bool(flags[t] & 1), (flags[t] >> 1) & 3, True)
            assert a[c:c + 1] == aa_ref.encode() and b[c:c + 1] == aa_alt.encode() and a[:c] == b[:c] and a[c + 1:] == b[c + 1:]
            n_coding += 1
    assert n_coding > 20


@pytest.mark.parametrize("text,line", [(b"c\t1\t.\tA\n", 1), (b"#h\n\nc\t5\t.\tA\tC\nc\t0\t.\tA\tC\n", 4), (b"c\t4294967296\t.\tA\tC\n", 1), (b"c\t1x\t.\tA\tC\n", 1),
                                       (b"c\t\t.\tA\tC\n", 1), (b"c\t00000000001\t.\tA\tC\n", 1), (b"c\t+1\t.\tA\tC\n", 1)])
def test_the_variants_errors_name_their_line(text, line):
    with pytest.raises(D.VcfError) as ei:
        D.parse_vcf(text)
    assert ei.value.line == line


def test_the_alleles_of_a_variants_file():
    text = b"##x\n#CHROM\tPOS\nc\t4294967295\tid\tA\tC,G,AT,*,.,<DEL>,n\textra\tmore\r\n\r\nd\t0000000007\t.\tAC\tG\nd\t7\t.\tn\tt"
    taken, not_snv = D.parse_vcf(text)
    assert taken == [(3, b"c", BIG, b"A", b"C"), (3, b"c", BIG, b"A", b"G"), (3, b"c", BIG, b"A", b"n"), (6, b"d", 7, b"n", b"t")] and not_snv == 5


# ---- device/effect_core.hpp and host/effect_text.hpp under the sanitizers ----------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "effect_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, args, ok=(0,)):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, env=env, timeout=600)
    assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode in ok, r.stderr[-3000:]
    return r


class Virtual(bytes):
    """A sequence of which only the length is known: the cases over it ask for no base."""
    def __new__(cls, n):
        self = super().__new__(cls, b"")
        self.n = n
        return self

    def __len__(self):
        return self.n


def _rules(tool, tmp_path, seqs, rows, flags, alleles):
    """The case through `effect_check --rules`, held to the definition; returns the classes it met."""
    lines = ["S %d %s" % (len(s), "-" if isinstance(s, Virtual) else s.decode("latin-1")) for s in seqs]
    lines += ["T %d" % f for f in flags] + ["R %d %d %d %d %d" % r for r in rows]
    lines += ["A %d %d %s %s" % (q, x, chr(ra & 255), chr(ra >> 8)) for q, x, ra in alleles]
    path = tmp_path / "case.txt"
    path.write_bytes(("\n".join(lines) + "\n").encode("latin-1"))
    got = _run_tool(tool, ["--rules", path]).stdout.decode("latin-1").split("\n")[:-1]
    trs = D.transcripts(seqs, rows, flags)
    want = ["t %d %d %d" % (0 if t["kept"] else 1, t["lo"], t["hi"]) for t in trs]
    off, rms, recs = D.pairs(seqs, rows, flags, alleles)
    for i in range(len(alleles)):
        want.append("a %d %d" % (off[i + 1] - off[i], rms[i]))
        for t, cls, q, c, k, cr, ca, ar, aa, _ in recs[off[i]:off[i + 1]]:
            tail = "%s %s %s %s" % (cr.decode("latin-1"), ca.decode("latin-1"), ar, aa) if cls in D.CODING else "- - - -"
            want.append("p %d %s %d %d %d %s" % (t, cls, q, c, k, tail))
    assert got == want
    return {r[1] for r in recs}


def al(q, x, ref, alt):
    return (q, x, ref | alt << 8)


def test_the_class_names(tool):
    assert _run_tool(tool, ["--classes"]).stdout.decode().split() == list(D.CLASSES)


def test_every_class_on_the_worked_example(tool, tmp_path):
    names, seqs = S.parse_fasta(D.HAND_FASTA)
    rows, flags, tnames, _, _ = D.gff_transcripts(D.HAND_GFF, names, seqs)
    assert tnames == ["tP", "tM", "tN"] and flags == [2, 1, 0]
    alleles = [al(0, x, ref[0], alt[0]) for _, _, x, ref, alt in D.parse_vcf(D.HAND_VCF)[0]]
    assert _rules(tool, tmp_path, seqs, rows, flags, alleles) == set(D.CLASSES) - {"intergenic"}


@pytest.mark.parametrize("layout", ["one_segment", "one_base_segments"])
def test_all_64_codons_3_positions_4_alternates(tool, tmp_path, layout):
    codons = "".join(a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG").encode()  # (x = 1 and x = 192: the sequence's ends)
    seg = [(0, 192)] if layout == "one_segment" else [(i, i + 1) for i in range(192)]
    rows = [(t, 0, s, e, 0) for t in (0, 1) for s, e in seg]
    alleles = [al(0, x, codons[x - 1], alt) for x in range(1, 193) for alt in b"ACGT"]
    classes = _rules(tool, tmp_path, [codons], rows, [0, 1], alleles)
    assert classes == {"stop_retained", "synonymous", "stop_gained", "stop_lost", "missense"}
    _, _, recs = D.pairs([codons], rows, [0, 1], alleles)
    plus = [r for r in recs if r[0] == 0]
    assert [r[7] + ">" + r[8] for r in plus[:4]] == ["F>I", "F>L", "F>V", "F>F"]
    assert sorted({(r[5].decode(), r[7]) for r in plus}) == sorted(S.CODON.items())  # every codon against the dict table


@pytest.mark.parametrize("p", [0, 1, 2])
def test_every_phase_against_every_length(tool, tmp_path, p):
    seq = bytes(b"ATGGCCTAAGGTNACTGA"[i % 18] for i in range(120))
    rows, flags = [], []
    for L in range(1, 8):  # L - p = 0 .. 3 mod 3, and L <= p
        for minus in (0, 1):
            rows += [(len(flags), 0, 10 * L, 10 * L + L, 0)]
            flags.append(minus | p << 1)
    alleles = [al(0, x, seq[x - 1], b"ACGTN"[x % 5]) for x in range(1, 121)]
    assert "partial_codon" in _rules(tool, tmp_path, [seq], rows, flags, alleles)


def test_gaps_of_one_to_five_bases(tool, tmp_path):
    seq = bytes(b"ACGTTGCA"[i % 8] for i in range(80))
    ends, at = [], 5
    for gap in (1, 2, 3, 4, 5, 1):
        ends.append((at, at + 3))
        at += 3 + gap
    rows = [(t, 0, s, e, 1) for t in (0, 1) for s, e in ends] + [(2, 0, s, e, 0) for s, e in ends] + [(3, 0, s, e, 0) for s, e in ends]
    alleles = [al(0, x, seq[x - 1], ord("A")) for x in range(1, 45)]
    assert {"intron", "splice_donor", "splice_acceptor", "noncoding_exon"} <= _rules(tool, tmp_path, [seq], rows, [0, 1, 2, 1 | 4], alleles)


def test_duplicate_and_overlapping_segments_and_no_exon_lines(tool, tmp_path):
    seq = bytes(b"ATGGCCTAAGGTAACTGACC"[i % 20] for i in range(100))
    rows = [(0, 0, 10, 20, 0), (0, 0, 10, 20, 0), (0, 0, 15, 30, 0), (0, 0, 12, 14, 0), (0, 0, 40, 41, 0),  # t0: no exon line
            (1, 0, 10, 20, 0), (1, 0, 15, 30, 0), (1, 0, 5, 50, 1), (1, 0, 5, 50, 1), (1, 0, 20, 60, 1), (1, 0, 70, 80, 1),
            (2, 0, 30, 40, 1), (2, 0, 10, 90, 1), (2, 0, 35, 36, 0)]  # t2: an exon inside a longer one that starts before it
    alleles = [al(0, x, seq[x - 1], b"ACGT"[x % 4]) for x in range(1, 101)]
    for flags in ([0, 1 | 2, 4], [1, 2, 1]):
        _rules(tool, tmp_path, [seq], rows, flags, alleles)
    for seed in range(4):
        _rules(tool, tmp_path, *D.random_case(80 + seed, n_tr=25, n_alleles=250))


def test_coordinates_at_the_end_of_32_bits_and_a_length_beyond(tool, tmp_path):
    seqs = [Virtual(BIG), Virtual(BIG - 1)]
    rows = [(0, 0, BIG - 12, BIG - 8, 1), (0, 0, BIG - 1, BIG, 1),                            # exons ... and the last base alone
            (1, 0, BIG - 6, BIG - 4, 0), (1, 0, BIG - 20, BIG, 1),                              # a CDS of two bases: no codon
            (2, 0, 0, BIG, 0), (2, 0, 0, BIG, 0), (2, 0, 0, BIG, 0),                            # L = 3 (2^32 - 1)
            (3, 0, 0, BIG, 0), (3, 0, 0, BIG, 0), (3, 0, 0, BIG, 0),
            (4, 1, BIG - 2, BIG, 1), (5, 1, BIG - 3, BIG - 1, 1)]                               # beyond the end of s1; its last base
    flags = [0, 1, 2, 1 | 4, 0, 1]
    xs = [BIG - 13, BIG - 12, BIG - 11, BIG - 8, BIG - 7, BIG - 6, BIG - 5, BIG - 4, BIG - 3, BIG - 2, BIG - 1, BIG]
    alleles = [al(0, x, ord("A"), ord("C")) for x in xs] + [al(0, 1, ord("A"), ord("C")), al(1, BIG - 1, ord("A"), ord("G")), al(1, BIG, ord("A"), ord("G"))]
    # (of t2 and t3 only what needs no base is asked: x = 1 is q = 0 < p on plus and q = L - 1 >= p + 3C on minus; the other
    #  alleles would land in a codon of theirs, so they go to a copy of the case without the two)
    keep = [r for r in rows if r[0] not in (2, 3)]
    renum = {0: 0, 1: 1, 4: 2, 5: 3}
    small = [(renum[t], q, s, e, k) for t, q, s, e, k in keep]
    classes = _rules(tool, tmp_path, seqs, small, [0, 1, 0, 1], alleles)
    assert {"noncoding_exon", "intron", "splice_donor", "splice_acceptor", "partial_codon", "5_prime_UTR", "3_prime_UTR"} <= classes
    assert D.dropped(seqs, small, [0, 1, 0, 1]) == [0, 0, 1, 0]
    _, _, recs = D.pairs(seqs, rows, flags, [al(0, 1, ord("A"), ord("C"))])
    assert [(r[0], r[1], r[2]) for r in recs] == [(2, "partial_codon", 0), (3, "partial_codon", 3 * BIG - 1)]
    _rules(tool, tmp_path, seqs, rows, flags, [al(0, 1, ord("A"), ord("C"))])


@pytest.mark.parametrize("text,line", [(b"c\t1\t.\tA\n", 1), (b"#h\n\nc\t5\t.\tA\tC\nc\t0\t.\tA\tC\n", 4), (b"c\t7\t.\tA\tC\r\nc\t4294967296\t.\tA\tC\n", 2),
                                       (b"c\t1\t.\tA\tC\n" * 9 + b"c\t1x\t.\tA\tC\n" + b"c\t1\t.\tA\n" * 3, 10)])
def test_the_variants_errors_in_any_number_of_parts(tool, tmp_path, text, line):
    path = tmp_path / "bad.vcf"
    path.write_bytes(text)
    for parts in (1, 2, 3, 7):
        assert _run_tool(tool, ["--vcf", path, parts], ok=(1,)).stdout.startswith(b"error %d " % line), parts


def test_the_variants_file_in_any_number_of_parts(tool, tmp_path):
    rng = random.Random(3)
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT"]
    for i in range(300):
        alt = b",".join(rng.choice([b"A", b"c", b"G", b"t", b"N", b"AT", b"*", b".", b"<DEL>", b""]) for _ in range(rng.randint(1, 4)))
        lines.append(b"chr%d\t%d\t.\t%s\t%s%s" % (rng.randrange(3), rng.randint(1, BIG), rng.choice([b"A", b"C", b"g", b"T", b"n", b"AC", b"."]), alt, rng.choice([b"", b"\tq\tPASS", b"\r"])))
        if rng.random() < 0.1:
            lines.append(rng.choice([b"", b"\r", b"# c"]))
    text = b"\n".join(lines) + rng.choice([b"", b"\n"])
    path = tmp_path / "ok.vcf"
    path.write_bytes(text)
    taken, not_snv = D.parse_vcf(text)
    want = b"".join(b"allele %s %d %s %s\n" % (c, x, r, a) for _, c, x, r, a in taken) + b"not_snv %d\n" % not_snv
    for parts in (1, 2, 5, 64, 1000):
        assert _run_tool(tool, ["--vcf", path, parts]).stdout == want, parts


def run_on_one_core(tool, tmp_path, gff, fasta, vcf, tag="x"):
    g, f, v, o, s = (tmp_path / (tag + ext) for ext in (".gff", ".fa", ".vcf", ".out", ".summary"))
    g.write_bytes(gff), f.write_bytes(fasta), v.write_bytes(vcf)
    r = _run_tool(tool, ["--run", g, f, v, "CDS", "exon", o, s])
    return o.read_bytes(), s.read_bytes(), r.stderr


@pytest.mark.parametrize("seed", range(4))
def test_the_command_on_one_core_gives_the_definitions_bytes(tool, tmp_path, seed):
    gff, fasta, vcf = D.random_files(seed, crlf=seed == 3)
    want, want_summary, cnt = D.render(gff, fasta, vcf)
    out, summary, err = run_on_one_core(tool, tmp_path, gff, fasta, vcf)
    assert out == want and summary == want_summary
    assert len(want.split(b"\n")) > 150 and len({line.split(b"\t")[6] for line in want.split(b"\n")[1:-1]}) >= 10
    for key, text in (("not_snv", b"alleles are not single-base substitutions"), ("no_chrom", b"alleles lie on a seqid the index does not have"),
                      ("orphans", b"features have no Parent"), ("mixed", b"members lie on more than one seqid or strand"),
                      ("unservable", b"a member lies on a seqid the FASTA file lacks or beyond its sequence")):
        assert (b"[WARN] %d " % cnt[key] in err and text in err) if cnt[key] else text not in err, key
    if seed == 0:
        assert all(cnt[k] for k in ("not_snv", "no_chrom", "orphans", "mixed", "unservable"))


def test_the_worked_example_on_one_core(tool, tmp_path):
    out, summary, err = run_on_one_core(tool, tmp_path, D.HAND_GFF, D.HAND_FASTA, D.HAND_VCF)
    assert out == D.HAND_OUT and summary == D.render(D.HAND_GFF, D.HAND_FASTA, D.HAND_VCF)[1] and b"WARN" not in err
