"""`gffx seq` end to end: the bytes of the output file, the warnings and the exit status.  On the worked example the file is the
hand-written answer of tests/_seq_definition.py; on a synthetic GFF (multi-parent `Parent=a,b` lines, orphan parents, a
`start > end` line, a gene beyond its sequence's end) over a random genome it is what the definition renders, in every mode
(per line, -j, -j --translate -T CDS, -w 0 / 1 / 60) and by every route: the line table parsed from the text, -t 1 and -t 16,
slices of 64 bytes, a FASTA with CR LF line ends, a FASTA that lacks a seqid.  A gzip-compressed FASTA is refused."""
import gzip
import os
import re
import subprocess

import pytest

import _seq_definition as sd
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
KNOB = "GFFX_SEQ_OUT_BYTES"
TIMEOUT = 120
CHROMS = [("chr1", 60000), ("chr2", 40000), ("chrM", 5000)]


def _seq(gff, fasta, out, extra=(), slice_bytes=None, parse=False, threads=None, ok=True):
    env = {k: v for k, v in os.environ.items() if k not in (KNOB, "GFFX_LINE_TABLE")}
    if slice_bytes:
        env[KNOB] = str(slice_bytes)
    if parse:
        env["GFFX_LINE_TABLE"] = "parse"
    cmd = [GFFX, "seq", "-v", "-i", gff, "-f", fasta, "-o", out] + list(extra) + (["-t", str(threads)] if threads else [])
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read(), r.stderr


def _warned(err, what):
    """the count of the [WARN] line that contains `what`, 0 without one"""
    hits = [ln for ln in err.split(b"\n") if ln.startswith(b"[WARN]") and what in ln]
    assert len(hits) <= 1
    return int(re.match(rb"\[WARN\] (\d+) ", hits[0]).group(1)) if hits else 0


def _check_warnings(err, cnt, join):
    assert _warned(err, b"features lie on a seqid the FASTA file lacks") == cnt["no_seq"]
    assert _warned(err, b"features reach beyond the end") == cnt["beyond"]
    assert _warned(err, b"features have no Parent") == (cnt["orphans"] if join else 0)
    assert _warned(err, b"more than one seqid or strand") == (cnt["mixed"] if join else 0)
    assert _warned(err, b"records were dropped: a member lies") == (cnt["unservable"] if join else 0)


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    d = tmp_path_factory.mktemp("seq_hand")
    gff, fa = str(d / "h.gff"), str(d / "h.fa")
    open(gff, "wb").write(sd.HAND_GFF)
    open(fa, "wb").write(sd.HAND_FASTA)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    return dict(dir=d, gff=gff, fa=fa)


def test_the_worked_example_prints_the_hand_written_answers(hand):
    d = hand["dir"]
    out, err = _seq(hand["gff"], hand["fa"], str(d / "a.fa"), ["-j"])
    assert out == sd.HAND_JOIN and b"[WARN]" not in err
    assert _seq(hand["gff"], hand["fa"], str(d / "b.fa"))[0] == sd.HAND_PLAIN
    assert _seq(hand["gff"], hand["fa"], str(d / "c.fa"), ["-j", "--translate", "-T", "CDS"])[0] == sd.HAND_CDS_TRANSLATED
    out, err = _seq(hand["gff"], hand["fa"], str(d / "d.fa"), ["-T", "gene", "-w", "4"])
    assert out == sd.HAND_GENES_W4 and _warned(err, b"features reach beyond the end") == 1
    assert _seq(hand["gff"], hand["fa"], str(d / "e.fa"), ["-T", "region"])[0] == sd.HAND_REGION
    # to stdout, and a type without lines
    r = subprocess.run([GFFX, "seq", "-i", hand["gff"], "-f", hand["fa"], "-j", "-T", "exon,tRNA"], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0 and r.stdout == sd.HAND_JOIN and b"[WARN] no line of" in r.stderr and b"'tRNA'" in r.stderr


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    d = tmp_path_factory.mktemp("seq_synth")
    roots = synth.gencode_like_roots(40, seed=5, chroms=CHROMS)
    gff = str(d / "s.gff")
    synth.write_gff3(gff, roots, seed=15, quirks=True)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    text = open(gff, "rb").read()
    assert b"Parent=gene" in text and re.search(rb"Parent=[^;\n]*,", text) and b"Parent=nowhere" in text and b"\t900\t850\t" in text
    # (chr2 is 3000 bases short of what the genes were laid out on: some features reach beyond it)
    fasta, _ = sd.random_genome(11, names=[n for n, _ in CHROMS], lengths=[60000, 37000, 5000])
    paths = {}
    for name, data in (("g.fa", fasta), ("crlf.fa", fasta.replace(b"\n", b"\r\n")), ("short.fa", fasta[:fasta.index(b">chrM")])):
        paths[name] = str(d / name)
        open(paths[name], "wb").write(data)
    return dict(dir=d, gff=gff, text=text, fasta=fasta, paths=paths)


MODES = {"per_line": ([], ("exon",), False, False), "join": (["-j"], ("exon",), True, False),
         "join_translate_cds": (["-j", "--translate", "-T", "CDS"], ("CDS",), True, True),
         "join_mrna_multi_parent": (["-j", "-T", "mRNA"], ("mRNA",), True, False), "genes": (["-T", "gene,mRNA"], ("gene", "mRNA"), False, False)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("w", [60, 0, 1])
def test_every_mode_gives_the_definitions_bytes(synthetic, mode, w):
    extra, types, join, translated = MODES[mode]
    want, cnt = sd.render(synthetic["text"], synthetic["fasta"], types, join, translated, w)
    out, err = _seq(synthetic["gff"], synthetic["paths"]["g.fa"], str(synthetic["dir"] / "o.fa"), extra + ["-w", str(w)])
    assert out == want and len(want) > 1000
    _check_warnings(err, cnt, join)


def test_every_warning_is_seen_once(synthetic):
    d, fa = synthetic["dir"], synthetic["paths"]["g.fa"]
    _, cnt = sd.render(synthetic["text"], synthetic["fasta"], ("mRNA",), True, False, 60)
    assert cnt["mixed"] > 0 and cnt["unservable"] > 0 and cnt["beyond"] > 0  # (the multi-parent lines tie genes of two strands together)
    # gene lines have no Parent: with -j every one is counted and nothing is written
    want, cnt = sd.render(synthetic["text"], synthetic["fasta"], ("gene",), True, False, 60)
    out, err = _seq(synthetic["gff"], fa, str(d / "w.fa"), ["-j", "-T", "gene"])
    assert out == want == b"" and cnt["orphans"] >= 40
    _check_warnings(err, cnt, True)


ROUTES = (dict(parse=True), dict(threads=1), dict(threads=16), dict(slice_bytes=64), dict(slice_bytes=64, parse=True, threads=1))


@pytest.mark.parametrize("mode,routes", [("join", ROUTES[:3]), ("join", ROUTES[3:]), ("join_translate_cds", ROUTES[3:]), ("genes", ROUTES[4:])])
def test_every_route_gives_the_same_bytes(synthetic, mode, routes):
    d, fa = synthetic["dir"], synthetic["paths"]["g.fa"]
    extra, types, join, translated = MODES[mode]
    want, _ = sd.render(synthetic["text"], synthetic["fasta"], types, join, translated, 60)
    for kw in routes:
        out, err = _seq(synthetic["gff"], fa, str(d / "r.fa"), extra, **kw)
        assert out == want, (mode, kw)
        assert (b"parsing the text" in err) == bool(kw.get("parse"))
    assert _seq(synthetic["gff"], synthetic["paths"]["crlf.fa"], str(d / "r.fa"), extra)[0] == want, mode


def test_a_knob_value_that_is_no_positive_number_is_ignored(synthetic):
    d, fa = synthetic["dir"], synthetic["paths"]["g.fa"]
    for bad in ("0", "64k"):
        out, err = _seq(synthetic["gff"], fa, str(d / "r.fa"), ["-j"], slice_bytes=bad)
        assert out == sd.render(synthetic["text"], synthetic["fasta"], join=True)[0] and b" in 1 slices" in err


def test_a_fasta_that_lacks_a_seqid(synthetic):
    d = synthetic["dir"]
    short = open(synthetic["paths"]["short.fa"], "rb").read()
    for mode in ("per_line", "join"):
        extra, types, join, translated = MODES[mode]
        want, cnt = sd.render(synthetic["text"], short, types, join, translated, 60)
        out, err = _seq(synthetic["gff"], synthetic["paths"]["short.fa"], str(d / "s.fa"), extra)
        assert out == want and cnt["no_seq"] > 0 and b"chrM" not in out
        _check_warnings(err, cnt, join)


def test_refused_fasta_files(synthetic):
    d = synthetic["dir"]
    gz = str(d / "g.fa.gz")
    open(gz, "wb").write(gzip.compress(synthetic["fasta"][:1000]))
    r = _seq(synthetic["gff"], gz, str(d / "x.fa"), ok=False)
    assert r.returncode == 1 and r.stderr.endswith(b"Error: compressed FASTA is not read: decompress \"" + gz.encode() + b"\" first\n")
    for name, text, line, what in (("early.fa", b"ACGT\n>chr1\nAC\n", 1, b"before the first"), ("noname.fa", b">chr1\nAC\n>\n", 3, b"without a sequence name"),
                                   ("twice.fa", b">chr1\nAC\n\n>chr1 again\n", 4, b"given twice")):
        path = str(d / name)
        open(path, "wb").write(text)
        r = _seq(synthetic["gff"], path, str(d / "x.fa"), ok=False)
        assert r.returncode == 1 and b"Error: FASTA file " + path.encode() + b", line %d: " % line in r.stderr and what in r.stderr, r.stderr
    r = _seq(synthetic["gff"], str(d / "missing.fa"), str(d / "x.fa"), ok=False)
    assert r.returncode == 1 and b"Error: Cannot open FASTA file" in r.stderr
