"""`gffx annotate` end to end on a hand-written GFF and BED (tests/_annotate_definition.py): the output bytes and the --summary
file are the hand-written text from q.bed, from q.bed.gz (bgzipped: the device reader), with chunks of 200 bytes, with
GFFX_BED_DEVICE=1, with -t 1 and -t 16, with and without the all-line table, and -- for one region -- with -r; a type nobody
carries is a warning and a column of zeros; a malformed coordinate ends the run as it ends `gffx closest`."""
import os
import subprocess

import pytest

import _annotate_definition as ad
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
KNOBS = ("GFFX_BED_DEVICE", "GFFX_BED_CHUNK_BYTES", "GFFX_CHUNK_BYTES", "GFFX_CHUNK_MB", "GFFX_LINE_TABLE")
TIMEOUT = 120
TYPES = ",".join(ad.LAYER_NAMES)


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    d = tmp_path_factory.mktemp("annotate_cli")
    gff = str(d / "hand.gff")
    open(gff, "w").write(ad.GFF)
    r = subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(gff + ".lall")
    bed = str(d / "q.bed")
    open(bed, "wb").write(ad.BED)
    open(bed + ".gz", "wb").write(b"".join(synth.bgzf_member(ad.BED[i:i + 40]) for i in range(0, len(ad.BED), 40)) + synth.BGZF_EOF)
    bad = str(d / "bad.bed")
    open(bad, "wb").write(ad.BED + b"chrA\t12\tx7\tname\nchrA\t1\t2\n")
    return dict(dir=d, gff=gff, bed=bed, bad=bad)


def _run(inp, args, knobs=None, out=None, command="annotate", types=TYPES):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs or {})
    cmd = [GFFX, command, "-i", inp["gff"]] + (["-T", types] if types else []) + list(args) + (["-o", out] if out else [])
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    errors = [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")]
    return r.returncode, errors, open(out, "rb").read() if out and os.path.exists(out) else r.stdout


def test_the_bytes_are_the_hand_written_text_on_every_route(inp):
    want = ad.BY_HAND_TEXT
    assert _run(inp, ["-b", inp["bed"]]) == (0, [], want)  # stdout
    assert _run(inp, ["-b", inp["bed"] + ".gz"]) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"]], {"GFFX_CHUNK_BYTES": "200"}) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"]], {"GFFX_CHUNK_BYTES": "1"}) == (0, [], want)  # a chunk per line
    assert _run(inp, ["-b", inp["bed"]], {"GFFX_BED_DEVICE": "1"}) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"] + ".gz"], {"GFFX_CHUNK_BYTES": "12"}) == (0, [], want)  # the device reader's rows, two per slice
    assert _run(inp, ["-b", inp["bed"], "-t", "1"]) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"], "-t", "16"], out=str(inp["dir"] / "out.tsv")) == (0, [], want)
    assert _run(inp, ["-b", inp["bed"]], {"GFFX_LINE_TABLE": "parse"}) == (0, [], want)  # without the .lall image


def test_the_summary_file_on_every_route(inp):
    for n, (extra, knobs) in enumerate(([[], None], [[], {"GFFX_CHUNK_BYTES": "200"}], [["-t", "1"], {"GFFX_LINE_TABLE": "parse"}])):
        path = str(inp["dir"] / ("summary%d.tsv" % n))
        bed = inp["bed"] + (".gz" if n == 1 else "")
        assert _run(inp, ["-b", bed, "--summary", path] + extra, knobs) == (0, [], ad.BY_HAND_TEXT)
        assert open(path, "rb").read() == ad.BY_HAND_SUMMARY


def test_one_region_with_r(inp):
    head = ad.BY_HAND_TEXT.split(b"\n")[0] + b"\n"
    assert _run(inp, ["-r", "chrA:260-650"]) == (0, [], head + b"chrA\t260\t650\texon\t0\t140\t150\t100\n")
    assert _run(inp, ["-r", "chrB:0-30"]) == (0, [], head + b"chrB\t0\t30\tCDS\t10\t10\t0\t10\n")


def test_the_priority_order_is_the_order_of_the_names(inp):
    # gene first: every base of a gene is "gene"
    rc, errors, body = _run(inp, ["-r", "chrA:100-650"], types="gene,CDS,exon")
    assert (rc, errors, body) == (0, [], b"#chr\tstart\tend\tclass\tgene\tCDS\texon\tnone\nchrA\t100\t650\tgene\t450\t0\t0\t100\n")
    rc, errors, body = _run(inp, ["-r", "chrA:100-650"], types="exon")
    assert (rc, errors, body) == (0, [], b"#chr\tstart\tend\tclass\texon\tnone\nchrA\t100\t650\texon\t250\t300\n")


def test_a_type_nobody_carries_is_a_warning_and_a_zero_column(inp):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([GFFX, "annotate", "-i", inp["gff"], "-b", inp["bed"], "-T", "CDS,pseudogene,exon,gene", "-v"], capture_output=True, env=env,
                       timeout=TIMEOUT)
    assert r.returncode == 0
    warn = [ln for ln in r.stderr.splitlines() if ln.startswith(b"[WARN]")]
    assert len(warn) == 1 and b"'pseudogene'" in warn[0]
    counts = [[row[0], 0] + row[1:] for row in ad.HAND_COUNTS]
    classes = [k + 1 if 0 < k < 3 else 4 if k == 3 else k for k in ad.HAND_CLASS]
    assert r.stdout == ad.expected_text(["CDS", "pseudogene", "exon", "gene"], counts, classes)
    # -v says how many lines each layer got and how many were skipped
    assert b"layer 0 'CDS': 2 lines" in r.stderr and b"layer 2 'exon': 4 lines" in r.stderr and b"layer 3 'gene': 3 lines" in r.stderr
    assert b"0 lines skipped" in r.stderr


def test_a_malformed_coordinate_ends_the_run_like_closest(inp):
    want = (1, [b'Error: lexical parse error: invalid BED coordinate in "chrA\t12\tx7\tname"'])
    assert _run(inp, ["-b", inp["bad"]], command="closest", types=None)[:2] == want
    assert _run(inp, ["-b", inp["bad"]])[:2] == want
    assert _run(inp, ["-b", inp["bad"]], {"GFFX_BED_DEVICE": "1"})[:2] == want
    assert _run(inp, ["-b", inp["bad"]], {"GFFX_BED_DEVICE": "1"}, command="closest", types=None)[:2] == want
    rc, errors, _ = _run(inp, ["-r", "chrA:170-165"])
    assert rc == 1 and errors == [b"Error: Region start must be less than end (170 >= 165)"]
    rc, errors, _ = _run(inp, ["-r", "chr9:1-2"])
    assert rc == 1 and errors == [b"Error: Sequence ID not found: chr9"]
