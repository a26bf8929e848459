"""`gffx effect --indels` where no GPU is needed: the definition (tests/_effect_indel_definition.py) on its worked example and
under its laws on random disjoint models; classify_any of device/effect_core.hpp and the --indels side of host/effect_text.hpp
in their host build under AddressSanitizer + UndefinedBehaviorSanitizer (tools/effect_check.cpp, a stand-alone program) on
introns of 0 to 5 bases, one-base exons, every phase against k = 0, 1, 2 and d, m in 0 .. 7, deletions and insertions on, one
before and one past every edge, F equal to the span and a base short of it, coordinates at 2^32 - 1 and an L beyond 2^32,
pieces of 65 535 and 65 536 bytes, the trimming table, the variants file in any number of parts, the command on one core, and
the help and usage bytes with the flag."""
import os
import random
import subprocess

import pytest

import _effect_definition as D
import _effect_indel_definition as X
import _seq_definition as S
from test_effect_cpu import BIG, Virtual, _run_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "effect_check")
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


# ---- the definition -----------------------------------------------------------------------------------------------------

def test_the_worked_example():
    out, summary, cnt = X.render_indels(X.HAND_GFF, D.HAND_FASTA, X.HAND_VCF)
    assert out == X.HAND_OUT and not any(cnt.values())
    classes = {line.split(b"\t")[6].decode() for line in X.HAND_OUT.split(b"\n")[1:-1]}
    assert set(X.CLASSES_ALL[15:]) <= classes and {"partial_codon", "start_lost", "coding_unknown", "stop_gained", "stop_lost", "missense", "synonymous"} <= classes
    assert [line.split("\t")[0] for line in summary.decode().split("\n")[:-1]] == list(X.CLASSES_ALL)


def test_the_trimming_table():
    table = [((7, b"ATG", b"ACG"), (8, 1, 1, b"T", b"C")),          # an SNV inside a longer REF
             ((5, b"A", b"AT"), (6, 0, 1, b"", b"T")),              # a pure insertion
             ((5, b"AT", b"A"), (6, 1, 0, b"T", b"")),              # a pure deletion
             ((5, b"ATT", b"AT"), (7, 1, 0, b"T", b"")),            # the prefix goes first: the LAST T of the run goes (no left-alignment)
             ((5, b"TTA", b"TA"), (6, 1, 0, b"T", b"")),
             ((5, b"acg", b"ACGT"), (8, 0, 1, b"", b"T")),          # case folded
             ((5, b"ACGT", b"acgt"), (9, 0, 0, b"", b"")),          # equal
             ((5, b"CAG", b"TAGAG"), (5, 1, 3, b"C", b"TAG")),      # no prefix, the suffix AG
             ((5, b"GATTACA", b"GCA"), (6, 4, 0, b"ATTA", b"")),
             ((1, b"A", b"GA"), (1, 0, 1, b"", b"G")),              # an insertion in front of base 1
             ((5, b"AC", b"GT"), (5, 2, 2, b"AC", b"GT"))]          # an MNV
    for args, want in table:
        assert X.trim(*args) == want


def _models(seed):
    return X.random_disjoint_case(seed, n_tr=14, n_alleles=1000)


@pytest.mark.parametrize("seed", range(4))
def test_frameshift_only_if_the_length_changes_by_no_multiple_of_three_and_the_protein_law(seed):
    """frameshift is reached only if len(S') - len(S) is no multiple of 3; for a rule-3d result the translation of S' from the
    phase is the translation of S with the reference window's residues replaced by the alternate window's."""
    seqs, rows, flags, alleles = _models(300 + seed)
    trs = D.transcripts(seqs, rows, flags)
    off, _, recs = X.pairs_any(seqs, rows, flags, alleles)
    n_shift = n_window = 0
    for i, (q, x0, ref, ins) in enumerate(alleles):
        d, m = len(ref), len(ins)
        if d == 1 and m == 1:
            continue
        for t, cls, ta, c, k, *_ in recs[off[i]:off[i + 1]]:
            tr = trs[t]
            coords = [b for s, e in tr["D"] for b in range(s + 1, e + 1)]
            gone = [b for b in coords if x0 <= b < x0 + d]
            kept = [b for b in coords if not (x0 <= b < x0 + d)]
            at = sum(1 for b in kept if b < x0)
            S0 = bytes(seqs[q][b - 1] for b in coords)
            S1 = bytes(seqs[q][b - 1] for b in kept[:at]) + ins + bytes(seqs[q][b - 1] for b in kept[at:])
            if cls == "frameshift":
                assert (len(S1) - len(S0)) % 3 != 0
                n_shift += 1
            if cls in D.CODING + ("inframe_insertion", "inframe_deletion"):
                assert len(S1) - len(S0) == m - len(gone) and (m - len(gone)) % 3 == 0
                if tr["minus"]:
                    S0, S1 = S.revcomp(S0), S.revcomp(S1)
                p = tr["p"]
                prot = lambda s: "".join(D.amino(s[j:j + 3]) for j in range(p, len(s) - 2, 3))  # noqa: E731
                n_ref = -(-(k + len(gone)) // 3)
                n_alt = n_ref + (m - len(gone)) // 3
                a, b = prot(S0), prot(S1)
                assert b == a[:c] + b[c:c + n_alt] + a[c + n_ref:] and len(b) == len(a) - n_ref + n_alt
                ra, aa = a[c:c + n_ref], b[c:c + n_alt]
                want = ("coding_unknown" if "X" in ra + aa else ("stop_retained" if "*" in ra else "synonymous") if ra == aa else
                        "stop_gained" if "*" in aa and "*" not in ra else "stop_lost" if "*" in ra and "*" not in aa else
                        "inframe_insertion" if m > len(gone) else "inframe_deletion" if m < len(gone) else "missense")
                assert cls == want
                n_window += 1
    assert n_shift > 20 and n_window > 20


@pytest.mark.parametrize("seed", range(4))
def test_the_mirror_law(seed):
    """Reverse-complement the genome and mirror every coordinate, strand and allele: every pair keeps its class, cds_pos and
    aa_pos.  (On alleles that hit at most one splice window of a transcript: "the smallest first base, the left one on a tie"
    is not symmetric; gaps of four bases or more, as for the SNV's law.)"""
    seqs, rows, flags, alleles = X.random_disjoint_case(400 + seed, n_tr=14, n_alleles=500, gaps=(0, 4, 5, 6, 9), max_len=4)
    n = [len(s) for s in seqs]
    trs = D.transcripts(seqs, rows, flags)
    alleles = [a for a in alleles if all(len(X.windows_hit(tr, a[1], len(a[2]))) <= 1 for tr in trs if tr["seq"] == a[0])]
    m_seqs = [S.revcomp(s) for s in seqs]
    m_rows = [(t, q, n[q] - e, n[q] - s, k) for t, q, s, e, k in rows]
    m_flags = [f ^ 1 for f in flags]
    keep = [a for a in alleles if not (len(a[2]) == 0 and a[1] > n[a[0]])]
    # F mirrors onto itself: a deletion [x0, x0 + d - 1] begins at n + 1 - (x0 + d - 1); an insertion in front of x0 lies in front of n + 2 - x0
    m_alleles = [(q, n[q] + 2 - x0 - len(ref) if ref else n[q] + 2 - x0, S.revcomp(ref), S.revcomp(ins)) for q, x0, ref, ins in keep]
    ok = [i for i, a in enumerate(m_alleles) if not (len(a[2]) == 0 and a[1] < 2)]
    keep, m_alleles = [keep[i] for i in ok], [m_alleles[i] for i in ok]
    off, rm, recs = X.pairs_any(seqs, rows, flags, keep)
    m_off, m_rm, m_recs = X.pairs_any(m_seqs, m_rows, m_flags, m_alleles)
    assert off == m_off and rm == m_rm and len(recs) > 300
    # (a non-SNV's q is where the run BEGINS in transcription order on either strand, so it mirrors as it is)
    assert recs == m_recs
    assert len({r[1] for r in recs}) >= 12


@pytest.mark.parametrize("seed", range(3))
def test_one_base_against_one_base_is_the_snv(seed):
    seqs, rows, flags, snvs = D.random_case(500 + seed, n_tr=20, n_alleles=300)
    assert X.pairs_any(seqs, rows, flags, [(q, x, bytes([ra & 255]), bytes([ra >> 8])) for q, x, ra in snvs]) == D.pairs(seqs, rows, flags, snvs)


# ---- device/effect_core.hpp and host/effect_text.hpp under the sanitizers ----------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "effect_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _indel_rules(tool, tmp_path, seqs, rows, flags, alleles, shift=0, virtual=None):
    """The case through `effect_check --indel-rules`, held to the definition; returns the classes it met.  With `virtual` (the
    sequences' lengths) the tool is given no bases and every coordinate moved up by `shift`: the rules depend on differences
    of coordinates only, so the definition's answers on the small case hold there, with ref_match 0 for every d > 0."""
    tool_seqs = [Virtual(n) for n in virtual] if virtual else seqs
    lines = ["S %d %s" % (len(s), "-" if isinstance(s, Virtual) else s.decode("latin-1")) for s in tool_seqs]
    lines += ["T %d" % f for f in flags] + ["R %d %d %d %d %d" % (t, q, s + shift, e + shift, k) for t, q, s, e, k in rows]
    lines += ["I %d %d %s %s" % (q, x0 + shift, ref.decode() or "-", ins.decode() or "-") for q, x0, ref, ins in alleles]
    path = tmp_path / "case.txt"
    path.write_bytes(("\n".join(lines) + "\n").encode("latin-1"))
    got = _run_tool(tool, ["--indel-rules", path]).stdout.decode("latin-1").split("\n")[:-1]
    trs = D.transcripts(seqs, rows, flags)
    want = ["t %d %d %d" % (0 if t["kept"] else 1, t["lo"] + shift, t["hi"] + shift) for t in trs]
    off, rms, recs = X.pairs_any(seqs, rows, flags, alleles)
    for i, a in enumerate(alleles):
        rm = rms[i] if not virtual or not a[2] else 0
        want.append("a %d %d" % (off[i + 1] - off[i], rm))
        snv = len(a[2]) == 1 and len(a[3]) == 1
        for t, cls, q, c, k, cr, ca, ar, aa, _ in recs[off[i]:off[i + 1]]:
            tail = "" if not snv else " %s %s %s %s" % (cr.decode("latin-1"), ca.decode("latin-1"), ar, aa) if cls in D.CODING else " - - - -"
            want.append("p %d %s %d %d %d%s" % (t, cls, q, c, k, tail))
    assert got == want
    return {r[1] for r in recs}


def test_the_class_names(tool):
    assert _run_tool(tool, ["--all-classes"]).stdout.decode().split() == list(X.CLASSES_ALL)
    assert _run_tool(tool, ["--classes"]).stdout.decode().split() == list(D.CLASSES)  # (the flagless 15 stay)


def test_the_trimming_of_the_tool(tool):
    for pos, ref, alt in ((7, b"ATG", b"ACG"), (5, b"ATT", b"AT"), (5, b"acg", b"ACGT"), (5, b"ACGT", b"acgt"), (5, b"CAG", b"TAGAG"), (BIG, b"GATTACA", b"GCA"), (1, b"A", b"GA")):
        x0, d, m, _, _ = X.trim(pos, ref, alt)
        assert _run_tool(tool, ["--trim", pos, ref.decode(), alt.decode()]).stdout == b"%d %d %d\n" % (x0, d, m)


def test_every_class_on_the_worked_example(tool, tmp_path):
    names, seqs = S.parse_fasta(D.HAND_FASTA)
    rows, flags, tnames, _, _ = D.gff_transcripts(X.HAND_GFF, names, seqs)
    assert tnames == ["tP", "tM", "tN", "tO"]
    alleles = [(0,) + X.trim(pos, ref, alt)[:1] + X.trim(pos, ref, alt)[3:] for _, _, pos, ref, alt in X.parse_vcf_indels(X.HAND_VCF)[0]]
    assert set(X.CLASSES_ALL[15:]) <= _indel_rules(tool, tmp_path, seqs, rows, flags, alleles)


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_the_edge_cases(tool, tmp_path, name):
    """introns: 0 to 5 bases; one_base_exons: windows across three of them; phases: every phase against k and d, m in 0 .. 7;
    edges: on, one before and one past every row's edge, cmin, cmax and the span's edges, F == span and a base short;
    overlapping: unclassified_model between classified transcripts."""
    classes = _indel_rules(tool, tmp_path, *X.CASES[name]())
    want = {"introns": {"splice_donor", "splice_acceptor", "intron", "frameshift", "noncoding_exon"},
            "one_base_exons": {"splice_donor", "splice_acceptor", "frameshift", "inframe_insertion", "inframe_deletion", "partial_codon"},
            "phases": {"start_lost", "frameshift", "inframe_insertion", "inframe_deletion", "missense", "partial_codon", "stop_gained"},
            "edges": {"transcript_ablation", "5_prime_UTR", "3_prime_UTR", "partial_codon", "frameshift", "splice_donor", "intron", "start_lost"},
            "overlapping": {"unclassified_model", "transcript_ablation", "frameshift"}}[name]
    assert want <= classes, want - classes


@pytest.mark.parametrize("seed", range(4))
def test_random_disjoint_models(tool, tmp_path, seed):
    assert len(_indel_rules(tool, tmp_path, *X.random_disjoint_case(600 + seed, n_tr=25, n_alleles=400))) >= 12


NO_BASE = {"partial_codon", "frameshift", "splice_donor", "splice_acceptor", "intron", "5_prime_UTR", "3_prime_UTR", "noncoding_exon", "transcript_ablation",
           "unclassified_model"}


def test_coordinates_at_the_end_of_32_bits_and_a_length_beyond(tool, tmp_path):
    """The edge cases moved up so that the sequence ends at base 2^32 - 1, the tool given no base (a sequence of 4 GB is not
    written): the alleles whose pairs read none are asked (phases 1 and 2 keep rule 3b from reading codon 0).  Then an L
    beyond 2^32, which only rows that overlap can give: unclassified_model."""
    seqs, rows, flags, alleles = X.case_edges()
    flags = [f | 2 if not f & 6 else f for f in flags]
    n = len(seqs[0])
    off, _, recs = X.pairs_any(seqs, rows, flags, alleles)
    ask = [a for i, a in enumerate(alleles) if {r[1] for r in recs[off[i]:off[i + 1]]} <= NO_BASE and not (len(a[2]) == 1 and len(a[3]) == 1)]
    ask += [(0, n - 1, b"AC", b""), (0, n, b"A", b"GG"), (0, n, b"", b"T"), (0, n, b"AC", b"")]  # the last base; beyond it
    assert len(ask) > 300
    classes = _indel_rules(tool, tmp_path, seqs, rows, flags, ask, shift=BIG - n, virtual=[BIG])
    assert {"partial_codon", "frameshift", "splice_donor", "splice_acceptor", "intron", "5_prime_UTR", "3_prime_UTR", "transcript_ablation"} <= classes
    big = [Virtual(BIG)]
    rows = [(0, 0, 0, BIG, 0), (0, 0, 0, BIG, 0), (0, 0, 0, BIG, 0), (1, 0, BIG - 9, BIG - 3, 0)]  # L = 3 (2^32 - 1)
    lines = ["S %d -" % BIG, "T 2", "T 3"] + ["R %d %d %d %d %d" % r for r in rows]
    lines += ["I 0 %d %s %s" % a for a in ((1, "A", "-"), (BIG, "A", "-"), (BIG - 5, "-", "GG"), (BIG - 1, "AC", "T"), (1, "A", "C"))]
    path = tmp_path / "big.txt"
    path.write_text("\n".join(lines) + "\n")
    got = _run_tool(tool, ["--indel-rules", path]).stdout.decode().split("\n")[:-1]
    # (t1: minus, p = 1, rows 2^32 - 9 .. 2^32 - 4, L = 6: the insertion in front of 2^32 - 6 has qa = 3, ta = 3, c = 0, k = 2;
    #  the last allele is an SNV: t0 stays classified as the flagless command classifies it, q = 0 < p)
    assert got == ["t 0 1 %d" % BIG, "t 0 %d %d" % (BIG - 8, BIG - 3),
                   "a 1 0", "p 0 unclassified_model 0 0 0", "a 1 0", "p 0 unclassified_model 0 0 0",
                   "a 2 1", "p 0 unclassified_model 0 0 0", "p 1 frameshift 3 0 2", "a 1 0", "p 0 unclassified_model 0 0 0",
                   "a 1 0", "p 0 partial_codon 0 0 0 - - - -"]
    assert D.dropped(big, rows, [2, 3]) == [0, 0]


def test_pieces_of_65535_and_65536_bytes(tool, tmp_path):
    rng = random.Random(9)
    long_ref = bytes(rng.choice(b"ACGT") for _ in range(65535))
    genome = b"G" * 50 + long_ref + b"T" * 80
    big_ins = bytes(rng.choice(b"ACG") for _ in range(65534)) + b"A"
    text = (b"c\t51\t.\t" + long_ref + b"\tA," + long_ref + b"," + long_ref + b"C\n"       # a deletion of 65534; equal to REF; too long
            b"c\t50\t.\tG\tG" + big_ins[:65534] + b",G" + big_ins + b"\n"                    # an insertion of 65534; too long
            b"c\t51\t.\t" + long_ref + b"A\tC\n" + b"c\t7\t.\tG\t*,.,<DEL>,G]c:5],,GX\n" + b"c\t1\t.\tG\tAG\n")
    path = tmp_path / "long.vcf"
    path.write_bytes(text)
    taken, cnt = X.parse_vcf_indels(text)
    assert [(a[2], len(a[3]), len(a[4])) for a in taken] == [(51, 65535, 1), (50, 1, 65535)] and cnt == dict(other=6, too_long=3, same=1, ins_at_1=1)
    want = b"".join(b"allele %s %d %s %s %d %d %d\n" % ((c, pos, ref, alt) + X.trim(pos, ref, alt)[:3]) for _, c, pos, ref, alt in taken)
    want += b"left_out %d %d %d %d\n" % tuple(cnt[k] for k in X.COUNTS)
    for parts in (1, 3):
        assert _run_tool(tool, ["--vcf-indels", path, parts]).stdout == want
    # ... and through the rules: the longest deletion and the longest insertion over a CDS that holds them
    rows = [(0, 0, 30, 40, 0), (0, 0, 45, 50 + 65535 + 40, 0), (1, 0, 30, 50 + 65535 + 40, 0)]
    alleles = [(0,) + X.trim(a[2], a[3], a[4])[:1] + X.trim(a[2], a[3], a[4])[3:] for a in taken]
    alleles += [(0, 51, long_ref, long_ref[::-1][:65532] if long_ref[-1] != long_ref[0] else b"")]  # in frame: windows of 21845 codons
    classes = _indel_rules(tool, tmp_path, [genome], rows, [0, 1 | 2], alleles)
    assert classes & {"frameshift", "inframe_deletion", "inframe_insertion", "stop_gained", "missense", "stop_lost", "stop_retained", "synonymous"}
    # ... and the case the device is given (test_effect_indel_gpu.py)
    assert {"frameshift", "stop_lost", "inframe_deletion", "inframe_insertion"} <= _indel_rules(tool, tmp_path, *X.case_long_pieces())


def test_the_variants_file_in_any_number_of_parts(tool, tmp_path):
    rng = random.Random(4)
    pieces = [b"A", b"c", b"G", b"t", b"N", b"AT", b"ACG", b"acgt", b"TTTTTT", b"*", b".", b"<DEL>", b"", b"A[chr2:5[", b"AxT"]
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT"]
    for i in range(300):
        alt = b",".join(rng.choice(pieces) for _ in range(rng.randint(1, 4)))
        lines.append(b"chr%d\t%d\t.\t%s\t%s%s" % (rng.randrange(3), rng.choice((1, 1, 2, rng.randint(1, BIG), BIG)), rng.choice(pieces[:10] + [b"AC", b"."]), alt,
                                                   rng.choice([b"", b"\tq\tPASS", b"\r"])))
        if rng.random() < 0.1:
            lines.append(rng.choice([b"", b"\r", b"# c"]))
    text = b"\n".join(lines) + rng.choice([b"", b"\n"])
    path = tmp_path / "ok.vcf"
    path.write_bytes(text)
    taken, cnt = X.parse_vcf_indels(text)
    assert all(cnt[k] for k in ("other", "same", "ins_at_1")) and len(taken) > 100  # (too_long: test_pieces_of_65535_and_65536_bytes)
    want = b"".join(b"allele %s %d %s %s %d %d %d\n" % ((c, pos, ref, alt) + X.trim(pos, ref, alt)[:3]) for _, c, pos, ref, alt in taken)
    want += b"left_out %d %d %d %d\n" % tuple(cnt[k] for k in X.COUNTS)
    for parts in (1, 2, 5, 64, 1000):
        assert _run_tool(tool, ["--vcf-indels", path, parts]).stdout == want, parts
    bad = tmp_path / "bad.vcf"
    bad.write_bytes(b"c\t7\t.\tAC\tA\r\n" * 9 + b"c\t1x\t.\tAC\tA\n" + b"c\t1\t.\tA\n" * 3)
    for parts in (1, 2, 3, 7):
        assert _run_tool(tool, ["--vcf-indels", bad, parts], ok=(1,)).stdout.startswith(b"error 10 "), parts


def run_on_one_core(tool, tmp_path, gff, fasta, vcf, tag="x"):
    g, f, v, o, s = (tmp_path / (tag + ext) for ext in (".gff", ".fa", ".vcf", ".out", ".summary"))
    g.write_bytes(gff), f.write_bytes(fasta), v.write_bytes(vcf)
    r = _run_tool(tool, ["--run", "--indels", g, f, v, "CDS", "exon", o, s])
    return o.read_bytes(), s.read_bytes(), r.stderr


def check_warnings(err, cnt):
    texts = dict(X.WARNINGS, no_chrom=b"alleles lie on a seqid the index does not have", orphans=b"features have no Parent",
                 mixed=b"members lie on more than one seqid or strand", unservable=b"a member lies on a seqid the FASTA file lacks or beyond its sequence")
    for key, text in texts.items():
        assert (b"[WARN] %d " % cnt[key] in err and text in err) if cnt[key] else text not in err, key
    assert b"not single-base substitutions" not in err


@pytest.mark.parametrize("seed", range(4))
def test_the_command_on_one_core_gives_the_definitions_bytes(tool, tmp_path, seed):
    gff, fasta, vcf = X.random_files(seed, crlf=seed == 3)
    want, want_summary, cnt = X.render_indels(gff, fasta, vcf)
    out, summary, err = run_on_one_core(tool, tmp_path, gff, fasta, vcf)
    assert out == want and summary == want_summary
    assert len(want.split(b"\n")) > 150 and len({line.split(b"\t")[6] for line in want.split(b"\n")[1:-1]}) >= 12
    check_warnings(err, cnt)
    if seed == 0:
        assert all(cnt[k] for k in ("other", "same", "ins_at_1", "no_chrom", "orphans", "mixed", "unservable"))


def test_the_worked_example_on_one_core(tool, tmp_path):
    out, summary, err = run_on_one_core(tool, tmp_path, X.HAND_GFF, D.HAND_FASTA, X.HAND_VCF)
    assert out == X.HAND_OUT and summary == X.render_indels(X.HAND_GFF, D.HAND_FASTA, X.HAND_VCF)[1] and b"WARN" not in err


# ---- the command line with the flag --------------------------------------------------------------------------------------------

def test_the_help_and_usage_bytes_with_the_flag():
    plain = subprocess.run([GFFX, "effect", "--help"], capture_output=True)
    for args in (["--indels", "--help"], ["-h", "--indels"], ["-i", "x.gff", "--indels", "--device", "x", "--help"]):
        r = subprocess.run([GFFX, "effect"] + args, capture_output=True)
        assert (r.returncode, r.stderr) == (0, b"") and r.stdout == X.HELP
    assert plain.stdout != X.HELP and b"--indels" not in plain.stdout  # (the flagless help is pinned by test_effect_usage_cpu.py)
    assert all(c.encode() in X.HELP for c in X.CLASSES_ALL) and b"left-aligned" in X.HELP and b"residues an in-frame change replaces are not reported" in X.HELP
    for args, msg in ((["--indels"], "the following required arguments were not provided:\n  --input <FILE>\n  --fasta <FILE>\n  --variants <FILE>"),
                      (["-i", "x.gff", "-f", "g.fa", "-V", "c.vcf", "--indels", "--indels"], "the argument '--indels' cannot be used multiple times"),
                      (["-i", "x.gff", "-f", "g.fa", "-V", "c.vcf", "--indels", "yes"], "unexpected argument 'yes' found")):
        r = subprocess.run([GFFX, "effect"] + args, capture_output=True)
        assert (r.returncode, r.stdout, r.stderr) == (2, b"", b"error: " + msg.encode() + b"\n\n" + X.HELP + b"\nFor more information, try '--help'.\n"), args
    r = subprocess.run([GFFX, "effect", "-i", "/nonexistent/x.gff", "-f", "g.fa", "-V", "c.vcf", "--indels"], capture_output=True)
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and r.stdout == b""


# ---- the new exports without a GPU ---------------------------------------------------------------------------------------------

def test_the_new_exports_report_bad_arguments():
    import ctypes as C

    import numpy as np

    from gffx_amd import _ffi
    L = _ffi.lib()
    assert {"gffx_hip_effect_run_any_start", "gffx_hip_effect_arena_grows"} <= set(_ffi.SIGNATURES)
    grows = C.c_uint64(7)
    assert L.gffx_hip_effect_arena_grows(None, C.byref(grows)) == -1 and b"gffx_hip_effect_arena_grows" in L.gffx_hip_last_error() and grows.value == 7
    rows = np.zeros(6, dtype=np.uint32)
    arena = np.zeros(1, dtype=np.uint8)
    rc = L.gffx_hip_effect_run_any_start(None, 0, rows.ctypes.data_as(_ffi.u32p), 1, arena.ctypes.data_as(_ffi.u8p), 1)
    assert rc != 0 and b"gffx_hip_effect_run_any_start" in L.gffx_hip_last_error()
