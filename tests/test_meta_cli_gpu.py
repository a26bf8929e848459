"""`gffx meta` end to end on a hand-written GFF and reads: the summary and the --matrix file are, byte for byte, what
tests/_meta_definition.py renders from the definition; the same bytes from the .bed, .bed.gz, SAM and BAM twins, on two devices,
in batches of 7 rows and with the line table parsed from the text; -g cuts a window at the seqid's end; the unstranded lines are
counted in one warning."""
import os
import subprocess

import numpy as np
import pytest

import _meta_definition as md
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
KNOB = "GFFX_META_BATCH_ROWS"
TIMEOUT = 120

# chrA: the two genes of the hand example (gP [10, 16) on '+', gQ [20, 27) on '-') and their rows; chrB: a `region` line without
# an ID (the index skips that type, so it may have none), one gene without a strand, [3, 9), and a transcript with '?'
GFF = ("##gff-version 3\n"
       "chrA\tt\tgene\t11\t16\t.\t+\t.\tID=gP;gene_name=P\n"
       "chrA\tt\tmRNA\t11\t16\t.\t+\t.\tID=tP;Parent=gP\n"
       "chrA\tt\tgene\t21\t27\t.\t-\t.\tgene_name=Q;ID=gQ\n"
       "chrA\tt\tmRNA\t21\t27\t.\t-\t.\tID=tQ;Parent=gQ\n"
       "chrB\tt\tregion\t1\t10\t.\t.\t.\tName=whole\n"
       "chrB\tt\tgene\t4\t9\t.\t.\t.\tgene_name=R;ID=gR\n"
       "chrB\tt\tmRNA\t4\t9\t.\t?\t.\tID=tR\n")
NAMES = ["chrA", "chrB"]
GENES = np.array([(0, 10, 16, 0), (0, 20, 27, 1), (1, 3, 9, 0)], np.uint32)
GENE_IDS = ["gP", "gQ", "gR"]
MRNAS = np.array([(0, 10, 16, 0), (0, 20, 27, 1), (1, 3, 9, 0)], np.uint32)
ROWS = np.concatenate([md.HAND_ROWS, np.array([(1, 0, 5), (1, 4, 12), (1, 8, 9)], np.uint32)])
REFS = [("chrA", 100000), ("chrZ", 1000), ("chrB", 100000)]  # (BAM / SAM twins: chrZ is not in the index)
GENOME = b"chrA\t30\nchrB\t10\n"


def _bgzip(text, block=60):
    return b"".join(synth.bgzf_member(text[i:i + block]) for i in range(0, len(text), block)) + synth.BGZF_EOF


def _meta(gff, source, out, extra=(), matrix=None, gpus=1, batch_rows=None, parse=False):
    env = {k: v for k, v in os.environ.items() if k not in (KNOB, "GFFX_LINE_TABLE")}
    if batch_rows:
        env[KNOB] = str(batch_rows)
    if parse:
        env["GFFX_LINE_TABLE"] = "parse"
    cmd = [GFFX, "meta", "-v", "--gpus", str(gpus), "-i", gff, "-s", source, "-o", out] + list(extra) + (["--matrix", matrix] if matrix else [])
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read(), (open(matrix, "rb").read() if matrix else None), r.stderr


def _want(feats, ids, lay, seq_len=None):
    m = md.sparse(len(NAMES), ROWS, feats, lay, seq_len)
    return md.summary_text(lay, *md.totals(m, md.lens(feats, lay, seq_len))), md.matrix_text(NAMES, feats, ids, m)


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    d = tmp_path_factory.mktemp("meta")
    gff = str(d / "h.gff")
    open(gff, "w").write(GFF)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    text = b"# reads\nchrZ\t1\t2\n" + b"".join(b"%s\t%d\t%d\n" % (NAMES[c].encode(), s, e) for c, s, e in ROWS.tolist())
    open(str(d / "q.bed"), "wb").write(text)
    open(str(d / "q.bed.gz"), "wb").write(_bgzip(text))
    tid = {0: 0, 1: 2}
    order = sorted([tuple(r) for r in ROWS.tolist()] + [(9, 1, 2)], key=lambda r: (tid.get(r[0], 1), r[1]))  # coordinate-sorted, chrZ's read between
    recs = [(tid.get(c, 1), s, ((0, e - s),)) for c, s, e in order]
    synth.write_bam(str(d / "q.bam"), synth.bam_header(REFS), [synth.bam_record(t, p, cigar=cg) for t, p, cg in recs])
    synth.write_sam(str(d / "q.sam"), synth.sam_header(REFS), [synth.sam_line(REFS[t][0], p, cigar=cg) for t, p, cg in recs])
    open(str(d / "genome.txt"), "wb").write(GENOME)
    return dict(dir=d, gff=gff, bed=str(d / "q.bed"), genome=str(d / "genome.txt"))


POINT = ["-u", "4", "-d", "4", "-w", "2"]
SCALED = POINT + ["--scale", "3"]


def test_the_hand_example_in_both_modes(hand):
    d = hand["dir"]
    # chrA alone is the example whose numbers are written out in the definition
    only_a = str(d / "a.gff")
    open(only_a, "w").write("".join(ln + "\n" for ln in GFF.split("\n") if ln.startswith(("#", "chrA"))))
    assert subprocess.run([GFFX, "index", "-i", only_a], capture_output=True, timeout=TIMEOUT).returncode == 0
    summary, _, err = _meta(only_a, hand["bed"], str(d / "a.tsv"), POINT)
    assert summary == md.HAND_POINT_SUMMARY and b"[WARN]" not in err
    summary, _, _ = _meta(only_a, hand["bed"], str(d / "a.tsv"), SCALED)
    assert summary == md.HAND_SCALED_SUMMARY


@pytest.mark.parametrize("extra,lay", [(POINT, md.HAND_POINT), (SCALED, md.HAND_SCALED), (POINT + ["--anchor", "tes"], md.point(4, 4, 2, md.TES)),
                                       (["-u", "6", "-d", "3", "-w", "3", "--anchor", "center"], md.point(6, 3, 3, md.CENTER))])
def test_summary_and_matrix_are_the_definitions_bytes(hand, extra, lay):
    d = hand["dir"]
    summary, matrix, err = _meta(hand["gff"], hand["bed"], str(d / "s.tsv"), extra, matrix=str(d / "m.tsv"))
    want_summary, want_matrix = _want(GENES, GENE_IDS, lay)
    assert summary == want_summary and matrix == want_matrix
    warns = [ln for ln in err.split(b"\n") if ln.startswith(b"[WARN]")]
    assert len(warns) == 1 and warns[0].startswith(b"[WARN] 1 features have neither '+' nor '-'")
    # without --matrix the same summary
    assert _meta(hand["gff"], hand["bed"], str(d / "s2.tsv"), extra)[0] == summary


def test_other_types_and_a_type_without_lines(hand):
    d = hand["dir"]
    summary, matrix, err = _meta(hand["gff"], hand["bed"], str(d / "t.tsv"), POINT + ["-T", "mRNA,tRNA"], matrix=str(d / "tm.tsv"))
    assert (summary, matrix) == _want(MRNAS, ["tP", "tQ", "tR"], md.HAND_POINT)
    assert b"[WARN] no line of" in err and b"'tRNA'" in err and b"[WARN] 1 features have neither" in err
    both, matrix, _ = _meta(hand["gff"], hand["bed"], str(d / "t.tsv"), POINT + ["-T", "gene,mRNA"], matrix=str(d / "tm.tsv"))
    feats = np.stack([GENES[0], MRNAS[0], GENES[1], MRNAS[1], GENES[2], MRNAS[2]])  # file order
    assert (both, matrix) == _want(feats, ["gP", "tP", "gQ", "tQ", "gR", "tR"], md.HAND_POINT)
    # a line without ID= is named '.'
    _, matrix, err = _meta(hand["gff"], hand["bed"], str(d / "t.tsv"), POINT + ["-T", "region"], matrix=str(d / "tm.tsv"))
    assert matrix == _want(np.array([(1, 0, 10, 0)], np.uint32), ["."], md.HAND_POINT)[1] and b"[WARN] 1 features have neither" in err


def test_the_same_bytes_from_every_source_device_count_batch_size_and_line_table(hand):
    d = hand["dir"]
    first = _meta(hand["gff"], hand["bed"], str(d / "f.tsv"), SCALED, matrix=str(d / "fm.tsv"))[:2]
    assert first == _want(GENES, GENE_IDS, md.HAND_SCALED)
    for ext in (".bed.gz", ".sam", ".bam"):
        assert _meta(hand["gff"], str(d / ("q" + ext)), str(d / "x.tsv"), SCALED, matrix=str(d / "xm.tsv"))[:2] == first, ext
    for gpus, batch_rows, parse in ((2, None, False), (1, 7, False), (2, 7, False), (3, 2, False), (1, None, True), (2, 7, True)):
        got = _meta(hand["gff"], hand["bed"], str(d / "x.tsv"), SCALED, matrix=str(d / "xm.tsv"), gpus=gpus, batch_rows=batch_rows, parse=parse)
        assert got[:2] == first, (gpus, batch_rows, parse)
        assert (b"parsing the text" in got[2]) == parse


def test_a_genome_file_cuts_the_window_at_the_seqids_end(hand):
    d = hand["dir"]
    seq_len = [30, 10]
    free = _meta(hand["gff"], hand["bed"], str(d / "g0.tsv"), POINT, matrix=str(d / "g0m.tsv"))
    cut = _meta(hand["gff"], hand["bed"], str(d / "g1.tsv"), POINT + ["-g", hand["genome"]], matrix=str(d / "g1m.tsv"))
    assert cut[:2] == _want(GENES, GENE_IDS, md.HAND_POINT, seq_len) and free[:2] == _want(GENES, GENE_IDS, md.HAND_POINT)
    # gQ's first column [29, 31) loses the base beyond chrA's end, chrB's gene [3, 9) its columns beyond 10: less length, the same
    # bases wherever no row lies beyond the end (the row chrB [4, 12) does)
    assert cut[0] != free[0] and md.lens(GENES, md.HAND_POINT, seq_len).sum() < md.lens(GENES, md.HAND_POINT).sum()
    assert b"no -g" in free[2] and b"no -g" not in cut[2]
