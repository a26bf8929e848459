"""`gffx closest` end to end on a hand-written GFF and BED: the output bytes are the hand-written text for the six flag
combinations, the same from q.bed, from q.bed.gz (bgzipped: the device reader), with chunks of 200 bytes, with -t 1 and
-t 16, and -- for one region -- with -r; a malformed coordinate ends the run with intersect's Error: line and exit status."""
import os
import subprocess

import pytest

import _closest_definition as cd
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
KNOBS = ("GFFX_BED_DEVICE", "GFFX_BED_CHUNK_BYTES", "GFFX_CHUNK_BYTES", "GFFX_CHUNK_MB")
TIMEOUT = 120

# the four roots of the worked example (GFF is 1-based, closed: [100,200) is 101..200) with children, a second seqid, and a
# third one that the BED never names
GFF = """##gff-version 3
chr1\thand\tgene\t101\t200\t.\t+\t.\tID=geneA;gene_name=A
chr1\thand\tmRNA\t101\t200\t.\t+\t.\tID=mrnaA;Parent=geneA
chr1\thand\texon\t101\t150\t.\t+\t.\tID=exonA1;Parent=mrnaA
chr1\thand\tgene\t151\t160\t.\t-\t.\tID=geneB;gene_name=B
chr1\thand\tmRNA\t151\t160\t.\t-\t.\tID=mrnaB;Parent=geneB
chr1\thand\tgene\t301\t400\t.\t+\t.\tID=geneC;gene_name=C
chr1\thand\tmRNA\t301\t400\t.\t+\t.\tID=mrnaC;Parent=geneC
chr1\thand\tgene\t301\t350\t.\t+\t.\tID=geneD;gene_name=D
chr1\thand\tmRNA\t301\t350\t.\t+\t.\tID=mrnaD;Parent=geneD
chr2\thand\tgene\t1001\t2000\t.\t+\t.\tID=geneE;gene_name=E
chr2\thand\tmRNA\t1001\t2000\t.\t+\t.\tID=mrnaE;Parent=geneE
chr3\thand\tgene\t11\t20\t.\t+\t.\tID=geneF;gene_name=F
chr3\thand\tmRNA\t11\t20\t.\t+\t.\tID=mrnaF;Parent=geneF
"""
# the regions of the table, a row on an unknown seqid (skipped), a comment line, a start > end row (kept: no answer), chr2
BED = b"chr1\t220\t240\nchr1\t165\t170\tpeak2\n# a comment\nchr1\t250\t251\nchrUn\t5\t10\nchr1\t249\t251\nchr1\t200\t300\nchr1\t240\t220\nchr2\t10\t20\n"
HEADER = "chr\tstart\tend\tid\tfeature_start\tfeature_end\tdistance\n"
COORDS = {"A": (100, 200), "B": (150, 160), "C": (300, 400), "D": (300, 350)}

DEFAULT_BY_HAND = HEADER + (
    "chr1\t220\t240\tgeneA\t100\t200\t-21\n"
    "chr1\t165\t170\tgeneA\t100\t200\t0\n"
    "chr1\t250\t251\tgeneC\t300\t400\t50\n"
    "chr1\t250\t251\tgeneD\t300\t350\t50\n"
    "chr1\t249\t251\tgeneA\t100\t200\t-50\n"
    "chr1\t249\t251\tgeneC\t300\t400\t50\n"
    "chr1\t249\t251\tgeneD\t300\t350\t50\n"
    "chr1\t200\t300\tgeneA\t100\t200\t-1\n"
    "chr1\t200\t300\tgeneC\t300\t400\t1\n"
    "chr1\t200\t300\tgeneD\t300\t350\t1\n"
    "chr1\t240\t220\t.\t.\t.\t.\n"
    "chr2\t10\t20\tgeneE\t1000\t2000\t981\n")


def expected(combo):
    """The hand-written answers of the table (tests/_closest_definition.py: TABLE_BY_HAND) as the command prints them, then
    the inverted row and the chr2 row (geneE lies 981 to the right: nothing with --side left)."""
    out = [HEADER]
    for (c, s, e), row in zip(cd.TABLE_REGIONS.tolist(), cd.TABLE_BY_HAND[combo]):
        out += ["chr1\t%d\t%d\tgene%s\t%d\t%d\t%d\n" % (s, e, n, COORDS[n][0], COORDS[n][1], d) for n, d in row]
    out.append("chr1\t240\t220\t.\t.\t.\t.\n")
    out.append("chr2\t10\t20\t.\t.\t.\t.\n" if combo[1] == "left" else "chr2\t10\t20\tgeneE\t1000\t2000\t981\n")
    return "".join(out).encode()


def _flags(combo):
    return (["--ignore-overlaps"] if combo[0] else []) + (["--side", combo[1]] if combo[1] != "both" else [])


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    d = tmp_path_factory.mktemp("closest_cli")
    gff = str(d / "hand.gff")
    open(gff, "w").write(GFF)
    r = subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    bed = str(d / "q.bed")
    open(bed, "wb").write(BED)
    open(bed + ".gz", "wb").write(b"".join(synth.bgzf_member(BED[i:i + 40]) for i in range(0, len(BED), 40)) + synth.BGZF_EOF)
    bad = str(d / "bad.bed")
    open(bad, "wb").write(BED + b"chr1\t12\tx7\tname\nchr1\t1\t2\n")
    return dict(dir=d, gff=gff, bed=bed, bad=bad)


def _run(inp, args, knobs=None, out=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs or {})
    cmd = [GFFX, "closest", "-i", inp["gff"]] + list(args) + (["-o", out] if out else [])
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    return r.returncode, [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")], open(out, "rb").read() if out and os.path.exists(out) else r.stdout


def test_the_default_answers_written_out():
    assert expected((False, "both")) == DEFAULT_BY_HAND.encode()


@pytest.mark.parametrize("combo", cd.COMBOS, ids=lambda c: "%s-%s" % ("ignore" if c[0] else "default", c[1]))
def test_the_bytes_are_the_hand_written_text_on_every_route(inp, combo):
    want = expected(combo)
    f = _flags(combo)
    assert _run(inp, ["-b", inp["bed"]] + f) == (0, [], want)  # stdout
    assert _run(inp, ["-b", inp["bed"] + ".gz"] + f) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"]] + f, {"GFFX_CHUNK_BYTES": "200"}) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"], "-t", "1"] + f) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"], "-t", "16"] + f, out=str(inp["dir"] / "out.tsv")) == (0, [], want)


def test_smaller_chunks_and_the_device_reader_by_knob(inp):
    want = DEFAULT_BY_HAND.encode()
    assert _run(inp, ["-b", inp["bed"]], {"GFFX_BED_DEVICE": "1"}) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"]], {"GFFX_CHUNK_BYTES": "1"}) == (0, [], want)  # a chunk per line
    assert _run(inp, ["-b", inp["bed"] + ".gz"], {"GFFX_CHUNK_BYTES": "12"}) == (0, [], want)  # two rows per slice


@pytest.mark.parametrize("combo", cd.COMBOS, ids=lambda c: "%s-%s" % ("ignore" if c[0] else "default", c[1]))
def test_one_region_with_r(inp, combo):
    rows = cd.TABLE_BY_HAND[combo][1]  # [165,170)
    want = HEADER + "".join("chr1\t165\t170\tgene%s\t%d\t%d\t%d\n" % (n, COORDS[n][0], COORDS[n][1], d) for n, d in rows)
    assert _run(inp, ["-r", "chr1:165-170"] + _flags(combo)) == (0, [], want.encode())


def test_a_region_on_a_seqid_of_its_own_and_stats_json(inp):
    import json
    sj = str(inp["dir"] / "stats.json")
    rc, errors, body = _run(inp, ["-r", "chr3:0-5", "--stats-json", sj])
    assert (rc, errors, body) == (0, [], (HEADER + "chr3\t0\t5\tgeneF\t10\t20\t6\n").encode())
    stats = json.load(open(sj))
    assert stats["counts"]["regions"] == 1 and stats["counts"]["answered_roots"] == 1 and stats["counts"]["end_table_build_ms"] > 0


def test_a_malformed_coordinate_ends_the_run_like_intersect(inp):
    want = (1, [b'Error: lexical parse error: invalid BED coordinate in "chr1\t12\tx7\tname"'])
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([GFFX, "intersect", "-i", inp["gff"], "-b", inp["bad"]], capture_output=True, env=env, timeout=TIMEOUT)
    assert (r.returncode, [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")]) == want
    assert _run(inp, ["-b", inp["bad"]])[:2] == want
    assert _run(inp, ["-b", inp["bad"]], {"GFFX_BED_DEVICE": "1"})[:2] == want
    rc, errors, _ = _run(inp, ["-r", "chr1:170-165"])
    assert rc == 1 and errors == [b"Error: Region start must be less than end (170 >= 165)"]
    rc, errors, _ = _run(inp, ["-r", "chr9:1-2"])
    assert rc == 1 and errors == [b"Error: Sequence ID not found: chr9"]
