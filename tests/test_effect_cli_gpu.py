"""`gffx effect` end to end: the bytes of the table, the --summary file, the warnings and the exit status.  On the worked example the
table is the hand-written answer of tests/_effect_definition.py; on random small annotations (Parent lists, orphans, transcripts on
two strands, on a seqid the FASTA lacks and beyond a sequence's end) with variants of several ALT pieces, indel pieces and an
unknown CHROM it is what the definition renders, by every route: the line table parsed from the text, -t 1 and -t 16, chunks of
3 alleles (a line's ALT pieces fall into different chunks), CR LF line ends in every text input -- and the same bytes as the
check tool's `--run` on one host core (its build without the sanitizers, bin/effect_host_baseline: the sanitizer build runs in
tests/test_effect_cpu.py)."""
import os
import re
import subprocess

import pytest

import _effect_definition as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "effect_host_baseline")
KNOB = "GFFX_EFFECT_CHUNK_ROWS"
TIMEOUT = 120
WARNINGS = (("not_snv", b"alleles are not single-base substitutions"), ("no_chrom", b"alleles lie on a seqid the index does not have"),
            ("orphans", b"features have no Parent"), ("mixed", b"members lie on more than one seqid or strand"),
            ("unservable", b"a member lies on a seqid the FASTA file lacks or beyond its sequence"))


def _effect(files, out, extra=(), chunk=None, parse=False, threads=None):
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
    return _files(tmp_path_factory.mktemp("effect_hand"), "h", D.HAND_GFF, D.HAND_FASTA, D.HAND_VCF)


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "effect_host_baseline"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def test_the_worked_example_prints_the_hand_written_answers(hand):
    out, summary, err = _effect(hand, str(hand["dir"] / "a.tsv"))
    assert out == D.HAND_OUT and summary == D.render(*hand["texts"])[1] and b"[WARN]" not in err
    assert b"18 alleles, 30 pairs in 1 chunks" in err
    # to stdout, without a summary
    r = subprocess.run([GFFX, "effect", "-i", hand["gff"], "-f", hand["fa"], "--variants", hand["vcf"]], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0 and r.stdout == D.HAND_OUT
    # other type names: the CDS lines as exons of transcripts without CDS
    out, _, _ = _effect(hand, str(hand["dir"] / "b.tsv"), ["--cds-type", "none", "--exon-type", "CDS"])
    assert out == D.render(*hand["texts"], cds_type="none", exon_type="CDS")[0] and b"noncoding_exon" in out and b"missense" not in out


ROUTES = (dict(), dict(parse=True), dict(threads=1), dict(threads=16), dict(chunk=3), dict(chunk=3, parse=True, threads=1), dict(chunk=1))


@pytest.mark.parametrize("seed", range(3))
def test_every_route_gives_the_definitions_bytes(tmp_path, tool, seed):
    crlf = seed == 2
    files = _files(tmp_path, "r", *D.random_files(seed, crlf=crlf))
    want, want_summary, cnt = D.render(*files["texts"])
    assert len(want.split(b"\n")) > 150 and (not crlf or all(b"\r\n" in t for t in files["texts"]))
    for kw in ROUTES if seed == 0 else ROUTES[4:6]:
        out, summary, err = _effect(files, str(tmp_path / "o.tsv"), **kw)
        assert out == want and summary == want_summary, kw
        assert (b"parsing the text" in err) == bool(kw.get("parse"))
        for key, text in WARNINGS:
            assert _warned(err, text) == cnt[key], (key, kw)
        assert (int(re.search(rb" in (\d+) chunks", err).group(1)) > 50) == bool(kw.get("chunk"))
    if seed == 0:
        assert all(cnt[k] for k, _ in WARNINGS)
        alts = [line.split(b"\t")[4].split(b",") for line in files["texts"][2].split(b"\n") if line.count(b"\t") >= 4 and not line.startswith(b"#")]
        assert any(len(a) > 1 and b"AT" in a and (b"A" in a or b"C" in a) for a in alts)  # multi-allelic lines with an indel piece
    # ... and the same bytes as the command on one host core
    o, s = str(tmp_path / "host.tsv"), str(tmp_path / "host.summary")
    r = subprocess.run([tool, "--run", files["gff"], files["fa"], files["vcf"], "CDS", "exon", o, s], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    assert open(o, "rb").read() == want and open(s, "rb").read() == want_summary


def test_a_knob_value_that_is_no_positive_number_is_ignored(hand):
    for bad in ("0", "3k", "-3"):
        out, _, err = _effect(hand, str(hand["dir"] / "k.tsv"), chunk=bad)
        assert out == D.HAND_OUT and b" in 1 chunks" in err
    out, _, err = _effect(hand, str(hand["dir"] / "k.tsv"), chunk=7)
    assert out == D.HAND_OUT and b" in 3 chunks" in err


def test_a_variants_file_without_an_allele(hand):
    files = dict(hand, vcf=str(hand["dir"] / "empty.vcf"))
    open(files["vcf"], "wb").write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\nchrA\t5\t.\tAC\tA\n")
    out, summary, err = _effect(files, str(hand["dir"] / "e.tsv"))
    assert out == D.HAND_OUT.split(b"\n")[0] + b"\n" and _warned(err, b"not single-base") == 1
    assert summary == b"".join(c.encode() + b"\t0\t0\n" for c in D.CLASSES)
