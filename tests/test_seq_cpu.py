"""`gffx seq` where no GPU is needed: the definition (tests/_seq_definition.py) on the worked example with its hand-written
answers and under its three laws on random inputs; device/seq_core.hpp and the Parent / phase helpers of feature_rows.hpp in
their host build under AddressSanitizer + UndefinedBehaviorSanitizer (tools/seq_check.cpp): all 256 complement entries, all 64
codons and the X cases, the wrap arithmetic at its edges and beyond 2^32, the FASTA line rules whatever the cut of the text,
Parent lists; the whole command on one core against the definition; without a handle the C-ABI reports an error."""
import os
import random
import subprocess

import pytest

import _seq_definition as sd
from gffx_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "seq_check")


# ---- the definition -----------------------------------------------------------------------------------------------------

def test_the_worked_example():
    names, seqs = sd.parse_fasta(sd.HAND_FASTA)
    assert names == [b"chrA", b"chrB"] and seqs == [sd.HAND_CHRA, b"ttgcaN"]
    assert sd.render(sd.HAND_GFF, sd.HAND_FASTA, join=True, w=60)[0] == sd.HAND_JOIN
    assert sd.render(sd.HAND_GFF, sd.HAND_FASTA)[0] == sd.HAND_PLAIN
    assert sd.render(sd.HAND_GFF, sd.HAND_FASTA, types=("region",))[0] == sd.HAND_REGION
    assert sd.render(sd.HAND_GFF, sd.HAND_FASTA, types=("CDS",), join=True, translated=True)[0] == sd.HAND_CDS_TRANSLATED
    out, cnt = sd.render(sd.HAND_GFF, sd.HAND_FASTA, types=("gene",), w=4)
    assert out == sd.HAND_GENES_W4 and cnt["beyond"] == 1 and cnt["no_seq"] == 0
    assert sd.record_chars(seqs, [(0, 8, 12), (0, 1, 4)], False, 0, False) == sd.HAND_T1_JOINED
    assert sd.record_chars(seqs, [(0, 8, 12), (0, 1, 4)], False, 0, True) == sd.HAND_T1_PHASE0
    assert sd.record_chars(seqs, [(0, 8, 12), (0, 1, 4)], False, 1, True) == sd.HAND_T1_PHASE1
    assert sd.record_chars(seqs, [(0, 14, 17), (0, 18, 20)], True, 0, False) == sd.HAND_T2_JOINED
    assert sd.record_chars(seqs, [(0, 14, 17), (0, 18, 20)], True, 0, True) == sd.HAND_T2_TRANSLATED
    assert sd.record_chars(seqs, [(1, 0, 6)], True, 0, False) == sd.HAND_CHRB_MINUS
    assert sd.record_chars(seqs, [(1, 0, 7)], True, 0, False) is None and sd.record_chars(seqs, [(2, 0, 1)], False, 0, False) is None


def test_the_complement_and_the_codons():
    assert sd.revcomp(b"ACGTUacgtuRYKMBVDHSWNn-*x") == b"x*-nNWSDHBVKMRYaacgtAACGT"
    assert all(sd.COMPLEMENT[sd.COMPLEMENT[b]] == b for b in range(256) if chr(b) not in "Uu")
    assert sd.translate(b"ATGGCCTAAtgauuuNNNACNAC") == b"MA**FXX" and len(sd.CODON) == 64
    assert sd.translate(b"AT") == b"" and sd.translate(b"ATGA", 1) == b"*" and sd.translate(b"ATG", 1) == b""
    assert sd.wrap(b"", 5) == b"" and sd.wrap(b"ABCDE", 5) == b"ABCDE\n" and sd.wrap(b"ABCDEF", 5) == b"ABCDE\nF\n" and sd.wrap(b"ABCDEF", 0) == b"ABCDEF\n"
    for c in (0, 1, 59, 60, 61, 120):
        for w in (0, 1, 60):
            assert len(sd.wrap(b"x" * c, w)) == sd.body_bytes(c, w)


def _random_case(seed, no_u=False):
    rng = random.Random(seed)
    # (no U: it is the one letter whose complement does not lead back, so the mirror law holds without it only)
    fasta, seqs = sd.random_genome(seed, alphabet=b"ACGTacgtNnRYKMBVDHSW" if no_u else b"ACGTacgtNnRYKMBVDHSWUu")
    lines = []
    for t in range(12):
        q = rng.randrange(2)
        strand = rng.choice("+-")
        for k in range(rng.randrange(1, 6)):
            s = rng.randrange(1, len(seqs[q]) - 30)
            e = s + rng.randrange(0, 30)
            lines.append("chr%s\tt\texon\t%d\t%d\t.\t%s\t%s\tID=e%d.%d;Parent=t%d" % ("AB"[q], s, e, strand, rng.choice(".012"), t, k, t))
    rng.shuffle(lines)
    return ("\n".join(lines) + "\n").encode(), fasta, seqs


def _records(text):
    out = []
    for block in text.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        out.append((head, body.replace(b"\n", b"")))
    return out


@pytest.mark.parametrize("seed", range(5))
def test_a_minus_record_is_the_reverse_complement_of_its_plus_twin(seed):
    gff, fasta, _ = _random_case(seed, no_u=True)
    twin = gff.replace(b"\t-\t", b"\t*\t").replace(b"\t+\t", b"\t-\t").replace(b"\t*\t", b"\t+\t")
    for join in (False, True):
        a, b = _records(sd.render(gff, fasta, join=join)[0]), _records(sd.render(twin, fasta, join=join)[0])
        assert len(a) == len(b) > 0
        for (ha, ca), (hb, cb) in zip(a, b):
            assert ha.split(b"(")[0] == hb.split(b"(")[0] and ca == sd.revcomp(cb)


@pytest.mark.parametrize("seed", range(5))
def test_joining_is_concatenating_the_features_in_transcription_order(seed):
    gff, fasta, _ = _random_case(10 + seed)
    feats = sd.features(gff, ("exon",))
    single = dict((h.split(b" ")[0], c) for h, c in _records(sd.render(gff, fasta)[0]))
    for head, chars in _records(sd.render(gff, fasta, join=True)[0]):
        name = head.split(b" ")[0].decode()
        mine = sorted(((f["start"], k, f) for k, f in enumerate(feats) if name in f["parents"]), key=lambda x: x[:2])
        if mine[0][2]["minus"]:
            mine.reverse()
        assert chars == b"".join(single[f["id"].encode()] for _, _, f in mine)


@pytest.mark.parametrize("seed", range(5))
def test_a_translated_body_is_the_translation_of_the_untranslated_one(seed):
    gff, fasta, _ = _random_case(20 + seed)
    feats = sd.features(gff, ("exon",))
    plain, trans = _records(sd.render(gff, fasta, join=True, w=7)[0]), _records(sd.render(gff, fasta, join=True, translated=True, w=7)[0])
    assert [h for h, _ in plain] == [h for h, _ in trans]
    for (head, bases), (_, aa) in zip(plain, trans):
        name = head.split(b" ")[0].decode()
        mine = sorted(((f["start"], k, f) for k, f in enumerate(feats) if name in f["parents"]), key=lambda x: x[:2])
        lead = mine[-1][2] if mine[0][2]["minus"] else mine[0][2]
        assert aa == sd.translate(bases, sd.phase_skip(lead["phase"]))


@pytest.mark.parametrize("text,line,what", [(b"ACGT\n>a\nAC\n", 1, "before"), (b"\n\r\n \n>a\n", 3, "before"), (b">a\nAC\n>\nAC\n", 3, "no name"),
                                            (b">a\n> x\n", 2, "no name"), (b">a\n>b\n\n>a desc\n", 4, "twice")])
def test_the_fasta_errors_name_their_line(text, line, what):
    with pytest.raises(sd.FastaError) as ei:
        sd.parse_fasta(text)
    assert ei.value.line == line and what in ei.value.what


# ---- device/seq_core.hpp and feature_rows.hpp under the sanitizers -----------------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "seq_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, args, ok=(0,)):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, env=env, timeout=600)
    assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode in ok, r.stderr[-3000:]
    return r


def test_all_256_complement_entries(tool):
    assert bytes.fromhex(_run_tool(tool, ["--complement"]).stdout.decode().strip()) == sd.COMPLEMENT


def test_all_64_codons_and_the_x_cases(tool, tmp_path):
    codons = [a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG"]
    text = "".join(codons) + "".join(c.lower() for c in codons) + "".join(c.replace("T", "U") for c in codons) + "uUuNNNANTA-GRTT\xffAAAt\x00gAC"
    path = tmp_path / "codons.txt"
    path.write_bytes(text.encode("latin-1"))
    for p in (0, 1, 2):
        got = _run_tool(tool, ["--translate", p, path]).stdout.rstrip(b"\n")
        assert got == sd.translate(text.encode("latin-1"), p)
    assert _run_tool(tool, ["--translate", 0, path]).stdout.startswith(sd.TABLE1.encode() * 3 + b"FXXXX")


@pytest.mark.parametrize("w", [0, 1, 60, 2 ** 32 - 1])
def test_the_wrap_arithmetic(tool, w):
    big = 2 ** 32 - 1
    for c in sorted({0, 1, 2, max(w, 2) - 1, w, w + 1, 2 * w, 2 * w + 1, 5 * 2 ** 32 + 7}):
        want = sd.body_bytes(c, w)
        line = w + 1 if w else c + 1
        offs = sorted({b for b in (0, 1, w - 1, w, w + 1, line, 2 * line - 1, 2 * line, want - 2, want - 1, big, big + 1, 2 ** 32 + 5, 4 * 2 ** 32 + 3) if 0 <= b < want})
        got = _run_tool(tool, ["--wrap", c, w] + offs).stdout.split()
        assert int(got[0]) == want

        def char_at(b):
            if w == 0:
                return "n" if b == c else str(b)
            ln, col = divmod(b, w + 1)
            return "n" if col == w or ln * w + col >= c else str(ln * w + col)

        assert [g.decode() for g in got[1:]] == [char_at(b) for b in offs], (c, w)
    assert sd.body_bytes(5 * 2 ** 32 + 7, 60) > 2 ** 32 and len(sd.wrap(b"x" * 121, 60)) == sd.body_bytes(121, 60)


FASTA_CASES = {
    "hand": sd.HAND_FASTA,
    "crlf": b">a one\r\nAC\r\nGT\r\n\r\n>b\r\n\r\nTT\r\n",
    "empty_lines_anywhere": b"\n\n>a\n\nAC\n\n\nGT\n>b\n\n",
    "no_final_newline": b">a\nACGT\n>b\nTTG",
    "no_final_newline_cr": b">a\nACGT\r",
    "header_without_newline": b">a\nAC\n>b x",
    "ragged": b">a\tx\nA\nCG\nTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT\nG\n",
    "empty_sequences": b">a\n>b\n\n>c\nA\n>d",
    "greater_inside_a_line": b">a\nAC>GT\n >x\n",
    "cr_inside_a_line": b">a\nAC\rGT\n\r\r\n",
    "a_line_of_1_mib": b">big\n" + b"ACGTN" * (2 ** 20 // 5) + b"\n" + b"T" * (2 ** 20) + b"\nA\n",
}


@pytest.mark.parametrize("name", sorted(FASTA_CASES))
def test_the_fasta_line_rules_whatever_the_cut(tool, tmp_path, name):
    text = FASTA_CASES[name]
    names, seqs = sd.parse_fasta(text)
    want = b"".join(b"%s %d %s\n" % (n, len(s), s) for n, s in zip(names, seqs))
    path = tmp_path / "x.fa"
    path.write_bytes(text)
    pieces = (0, 65536, 1000003) if len(text) > 10000 else (0,) + tuple(range(1, len(text) + 1))
    for piece in pieces:
        assert _run_tool(tool, ["--fasta", path] + ([piece] if piece else [])).stdout == want, piece


@pytest.mark.parametrize("text,line,what", [(b"ACGT\n>a\nAC\n", 1, b"before"), (b"\n\r\n \n>a\n", 3, b"before"), (b">a\nAC\n>\nAC\n", 3, b"no name"),
                                            (b">a\n>\r\n", 2, b"no name"), (b">a\n>b\n\n>a desc\n", 4, b"twice")])
def test_the_fasta_errors_in_the_core(tool, tmp_path, text, line, what):
    path = tmp_path / "bad.fa"
    path.write_bytes(text)
    for piece in (0, 1, 2, 3):
        r = _run_tool(tool, ["--fasta", path] + ([piece] if piece else []), ok=(1,))
        assert r.stdout.startswith(b"error %d " % line) and what in r.stdout, (piece, r.stdout)


def test_parent_phase_and_strand_of_a_line(tool, tmp_path):
    many = ",".join("p%d" % i for i in range(1000))
    gff = ("##gff-version 3\n"
           "c\tt\texon\t1\t2\t.\t+\t0\tID=a;Parent=t1\n"
           "c\tt\texon\t1\t2\t.\t-\t2\tParent=t1,t2;ID=b\r\n"
           "c\tt\texon\t1\t2\t.\t.\t.\tID=c;xParent=no\n"
           "c\tt\texon\t1\t2\t.\t?\t12\tID=d;xParent=no;Parent=,,t3,,t4,\n"
           "c\tt\texon\t1\t2\t.\t+\t1\tParent=\n"
           "c\tt\texon\t1\t2\t.\t+\t1\n"
           "c\tt\texon\t1\t2\t.\t-\t.\tParent=" + many + ";ID=e\n"
           "c\tt\texon\t1\t2\t.\t+\t.\tID=f;Parent=last")
    path = tmp_path / "p.gff"
    path.write_bytes(gff.encode())
    got = _run_tool(tool, ["--fields", path]).stdout.decode().split("\n")[:-1]
    assert got == ["+ 0 a | t1 (1)", "- 2 b | t1 t2 (2)", ". . c | (0)", ". . d | t3 t4 (2)", "+ 1 . | (0)", "+ 1 . | (0)", "- . e | p0 p1 p2 (1000)", "+ . f | last (1)"]


@pytest.mark.parametrize("mode", ["plain", "join", "join_translate", "genes_w4", "w0", "w1"])
def test_the_command_on_one_core_gives_the_definitions_bytes(tool, tmp_path, mode):
    types, join, translated, w = {"plain": ("exon", 0, 0, 60), "join": ("exon", 1, 0, 60), "join_translate": ("CDS,exon", 1, 1, 60),
                                  "genes_w4": ("gene", 0, 0, 4), "w0": ("exon", 1, 0, 0), "w1": ("exon", 1, 1, 1)}[mode]
    cases = [(sd.HAND_GFF, sd.HAND_FASTA)] + [_random_case(30 + s)[:2] for s in range(3)]
    for k, (gff, fasta) in enumerate(cases):
        g, f, o = tmp_path / ("%d.gff" % k), tmp_path / ("%d.fa" % k), tmp_path / ("%d.out" % k)
        g.write_bytes(gff), f.write_bytes(fasta)
        _run_tool(tool, ["--run", g, f, types, join, translated, w, o])
        assert o.read_bytes() == sd.render(gff, fasta, tuple(types.split(",")), bool(join), bool(translated), w)[0], (mode, k)


# ---- the ABI without a handle -------------------------------------------------------------------------------------------

def test_a_null_handle_is_reported_not_crashed_on():
    L = _ffi.lib()
    rcs = [L.gffx_hip_genome_feed(None, None, 0), L.gffx_hip_genome_finish(None), L.gffx_hip_genome_reserve(None, 1), L.gffx_hip_genome_copy_names(None, None, None),
           L.gffx_hip_genome_copy_seqs(None, None, None), L.gffx_hip_genome_copy_bases(None, 0, 0, None)]
    assert rcs == [-1] * len(rcs) and b"genome handle is NULL" in L.gffx_hip_last_error()
    rcs = [L.gffx_hip_seq_copy_offsets(None, None, None), L.gffx_hip_seq_emit_start(None, 0, 0, 1), L.gffx_hip_seq_emit_wait(None, 0, None),
           L.gffx_hip_seq_stage_ms(None, None, None)]
    assert rcs == [-1] * len(rcs) and b"seq handle is NULL" in L.gffx_hip_last_error()
    assert L.gffx_hip_genome_n_seq(None) == 0 and L.gffx_hip_seq_body_bytes(None) == 0 and L.gffx_hip_seq_tile() >= 256
