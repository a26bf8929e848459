"""`gffx effect --indels` end to end: the bytes of the table, the --summary file of 20 lines, the warnings and the exit status.  On
the worked example the table is the hand-written answer of tests/_effect_indel_definition.py; on random small annotations with
variants of every kind it is what the definition renders, by every route of tests/test_effect_cli_gpu.py (the line table parsed
from the text, -t 1 and -t 16, chunks of 3 alleles and of 1, CR LF line ends) -- and the same bytes as the check tool's
`--run --indels` on one host core (its build without the sanitizers).  Without --indels the same variants file gives, byte for
byte, what the commit before this feature wrote: tests/golden/effect_indels_hand_flagless.tsv is that output, recorded."""
import os
import re
import subprocess

import pytest

import _effect_definition as D
import _effect_indel_definition as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "effect_host_baseline")
KNOB = "GFFX_EFFECT_CHUNK_ROWS"
TIMEOUT = 120
WARNINGS = tuple(X.WARNINGS.items()) + (("no_chrom", b"alleles lie on a seqid the index does not have"), ("orphans", b"features have no Parent"),
                                        ("mixed", b"members lie on more than one seqid or strand"),
                                        ("unservable", b"a member lies on a seqid the FASTA file lacks or beyond its sequence"))
# the worked example's variants, then the single-base ones of the flagless worked example
CLI_VCF = X.HAND_VCF + b"".join(line + b"\n" for line in D.HAND_VCF.split(b"\n")[2:-1])


def _effect(files, out, extra=("--indels",), chunk=None, parse=False, threads=None):
    env = {k: v for k, v in os.environ.items() if k not in (KNOB, "GFFX_LINE_TABLE")}
    if chunk:
        env[KNOB] = str(chunk)
    if parse:
        env["GFFX_LINE_TABLE"] = "parse"
    cmd = [GFFX, "effect", "-v", "-i", files["gff"], "-f", files["fa"], "-V", files["vcf"], "-o", out, "--summary", out + ".summary"] + list(extra)
    r = subprocess.run(cmd + (["-t", str(threads)] if threads else []), capture_output=True, env=env, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read(), open(out + ".summary", "rb").read(), r.stderr


def _warned(err, what):
    hits = [ln for ln in err.split(b"\n") if ln.startswith(b"[WARN]") and what in ln]
    assert len(hits) <= 1
    return int(re.match(rb"\[WARN\] (\d+) ", hits[0]).group(1)) if hits else 0


def _files(d, tag, gff, fasta, vcf):
    paths = dict(gff=str(d / (tag + ".gff")), fa=str(d / (tag + ".fa")), vcf=str(d / (tag + ".vcf")), dir=d, texts=(gff, fasta, vcf))
    for key, data in zip(("gff", "fa", "vcf"), (gff, fasta, vcf)):
        open(paths[key], "wb").write(data)
    r = subprocess.run([GFFX, "index", "-i", paths["gff"]], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    return paths


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    return _files(tmp_path_factory.mktemp("effect_indel_hand"), "h", X.HAND_GFF, D.HAND_FASTA, CLI_VCF)


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "effect_host_baseline"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def test_the_worked_example_prints_the_hand_written_answers(hand):
    out, summary, err = _effect(hand, str(hand["dir"] / "a.tsv"))
    snv_lines = b"".join(line + b"\n" for line in D.render(X.HAND_GFF, D.HAND_FASTA, D.HAND_VCF)[0].split(b"\n")[1:-1])
    assert out == X.HAND_OUT + snv_lines and b"[WARN]" not in err  # (a single-base allele's lines are the flagless command's)
    assert summary == X.render_indels(*hand["texts"])[1] and summary.count(b"\n") == 20
    assert b"39 alleles" in err and b" in 1 chunks" in err
    r = subprocess.run([GFFX, "effect", "--indels", "-i", hand["gff"], "-f", hand["fa"], "--variants", hand["vcf"]], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0 and r.stdout == out
    for chunk in (1, 3, 7):
        assert _effect(hand, str(hand["dir"] / "c.tsv"), chunk=chunk)[:2] == (out, summary)


def test_without_the_flag_the_same_file_gives_what_the_commit_before_wrote(hand):
    out, summary, err = _effect(hand, str(hand["dir"] / "f.tsv"), extra=())
    assert out == open(os.path.join(ROOT, "tests", "golden", "effect_indels_hand_flagless.tsv"), "rb").read()
    assert out == D.render(*hand["texts"])[0] and summary == D.render(*hand["texts"])[1] and summary.count(b"\n") == 15
    assert _warned(err, b"alleles are not single-base substitutions and were left out") == 21
    assert sum(ln.startswith(b"[WARN]") for ln in err.split(b"\n")) == 1


ROUTES = (dict(), dict(parse=True), dict(threads=1), dict(threads=16), dict(chunk=3), dict(chunk=3, parse=True, threads=1), dict(chunk=1))


@pytest.mark.parametrize("seed", range(3))
def test_every_route_gives_the_definitions_bytes(tmp_path, tool, seed):
    crlf = seed == 2
    files = _files(tmp_path, "r", *X.random_files(seed, crlf=crlf))
    want, want_summary, cnt = X.render_indels(*files["texts"])
    assert len(want.split(b"\n")) > 150 and (not crlf or all(b"\r\n" in t for t in files["texts"]))
    for kw in ROUTES if seed == 0 else ROUTES[4:6]:
        out, summary, err = _effect(files, str(tmp_path / "o.tsv"), **kw)
        assert out == want and summary == want_summary, kw
        for key, text in WARNINGS:
            assert _warned(err, text) == cnt[key], (key, kw)
        assert b"not single-base substitutions" not in err
        assert (int(re.search(rb" in (\d+) chunks", err).group(1)) > 50) == bool(kw.get("chunk"))
    if seed == 0:
        assert all(cnt[k] for k in ("other", "same", "ins_at_1", "no_chrom", "orphans", "mixed", "unservable"))
    # ... and the same bytes as the command on one host core
    o, s = str(tmp_path / "host.tsv"), str(tmp_path / "host.summary")
    r = subprocess.run([tool, "--run", "--indels", files["gff"], files["fa"], files["vcf"], "CDS", "exon", o, s], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    assert open(o, "rb").read() == want and open(s, "rb").read() == want_summary
    for key, text in WARNINGS:
        assert _warned(r.stderr, text) == cnt[key], key


def test_a_piece_too_long_and_an_allele_beyond_2_32(hand):
    files = dict(hand, vcf=str(hand["dir"] / "long.vcf"))
    open(files["vcf"], "wb").write(b"chrA\t5\t.\tC\t" + b"A" * 65536 + b"," + b"A" * 65535 + b"\nchrA\t4294967295\t.\tAC\tA\nchrA\t60\t.\tA\tAT,T\n")
    out, summary, err = _effect(files, str(hand["dir"] / "l.tsv"))
    lines = out.split(b"\n")[1:-1]
    assert _warned(err, X.WARNINGS["too_long"]) == 1 and len(lines) == 5
    assert lines[0].split(b"\t")[6:] == [b"5_prime_UTR", b".", b".", b".", b".", b"1"] and len(lines[0].split(b"\t")[3]) == 65535
    assert lines[2] == b"chrA\t4294967295\tAC\tA\t.\t.\tintergenic\t.\t.\t.\t.\t0"
    assert lines[3] == b"chrA\t60\tA\tAT\t.\t.\tintergenic\t.\t.\t.\t.\t0"  # (an insertion behind the last base reaches beyond the sequence)
    assert lines[4] == b"chrA\t60\tA\tT\t.\t.\tintergenic\t.\t.\t.\t.\t1"
