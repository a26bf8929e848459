"""`gffx coverage --thresholds T1,T2,... / --bedgraph FILE`: two columns per threshold -- bases_ge<T>, fraction_ge<T> -- behind
every column the command prints, and the depth profile itself as a bedGraph.  A hand-written GFF with the answers worked out
below and re-derived from tests/_profile_definition.py; the columns before the new ones byte for byte those of the run without
the flags; the same bytes whatever the source format, the device count or the batch size; and without the flags nothing new
anywhere."""
import json
import os
import subprocess

import numpy as np
import pytest

import _profile_definition as pf
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
HEAD6 = b"id\tchr\tstart\tend\tbreadth\tfraction"
HEAD9 = HEAD6 + b"\tbases\tlength\tmean_depth"
KNOB = "GFFX_COVERAGE_BATCH_ROWS"
TIMEOUT = 120
THRESHOLDS = (1, 2, 42, 43)

# 1-based closed in the text; below as 0-based half-open.
#   chr1  g1 [100,200)  t1 [100,200)  e1 [100,130)  e2 [150,200)  c1 on two lines [110,120) + [160,170)
#         g2 [300,400)  t2 [300,400)  e3 [280,320): sticks out of its gene
#   chr2  g3 [10,60)    t3, e4 the same
#   chr3  g4 [0,100)    t4, e5 the same: no row of the source is on chr3
GFF = ("##gff-version 3\n"
       "chr1\tt\tgene\t101\t200\t.\t+\t.\tID=g1;gene_name=G1\n"
       "chr1\tt\tmRNA\t101\t200\t.\t+\t.\tID=t1;Parent=g1\n"
       "chr1\tt\texon\t101\t130\t.\t+\t.\tID=e1;Parent=t1\n"
       "chr1\tt\texon\t151\t200\t.\t+\t.\tID=e2;Parent=t1\n"
       "chr1\tt\tCDS\t111\t120\t.\t+\t0\tID=c1;Parent=t1\n"
       "chr1\tt\tCDS\t161\t170\t.\t+\t0\tID=c1;Parent=t1\n"
       "chr1\tt\tgene\t301\t400\t.\t+\t.\tID=g2;gene_name=G2\n"
       "chr1\tt\tmRNA\t301\t400\t.\t+\t.\tID=t2;Parent=g2\n"
       "chr1\tt\texon\t281\t320\t.\t+\t.\tID=e3;Parent=t2\n"
       "chr2\tt\tgene\t11\t60\t.\t+\t.\tID=g3;gene_name=G3\n"
       "chr2\tt\tmRNA\t11\t60\t.\t+\t.\tID=t3;Parent=g3\n"
       "chr2\tt\texon\t11\t60\t.\t+\t.\tID=e4;Parent=t3\n"
       "chr3\tt\tgene\t1\t100\t.\t+\t.\tID=g4;gene_name=G4\n"
       "chr3\tt\tmRNA\t1\t100\t.\t+\t.\tID=t4;Parent=g4\n"
       "chr3\tt\texon\t1\t100\t.\t+\t.\tID=e5;Parent=t4\n")
NAMES = ["chr1", "chr2", "chr3"]
# rows (seqid, start, end): one deep on e1, two deep on e2, forty more on c1's second line (42 deep there), tiled end to end over
# g2 (a depth of exactly 1: the five tiles are ONE run), one row over the part of e3 outside its gene, two on chr2
ROWS = ([(0, 100, 130)] + [(0, 150, 200)] * 2 + [(0, 160, 170)] * 40 + [(0, 300 + 20 * k, 320 + 20 * k) for k in range(5)] +
        [(0, 270, 290)] + [(1, 0, 30), (1, 20, 80)])
# the depth, by hand:  chr1  [100,130) 1   [150,160) 2   [160,170) 42   [170,200) 2   [270,290) 1   [300,400) 1
#                      chr2  [0,20) 1      [20,30) 2     [30,80) 1
BEDGRAPH = (b"chr1\t100\t130\t1\nchr1\t150\t160\t2\nchr1\t160\t170\t42\nchr1\t170\t200\t2\nchr1\t270\t290\t1\nchr1\t300\t400\t1\n"
            b"chr2\t0\t20\t1\nchr2\t20\t30\t2\nchr2\t30\t80\t1\n")
# id -> (the ID's lines, bases at depth >= 1, 2, 42, 43, the lines' bases), by hand:
#   e1  all 30 at 1x            e2  all 50 at 2x, [160,170) at 42x       c1  [110,120) at 1x, [160,170) at 42x
#   g1 = t1  30 + 50 at 1x (nothing on [130,150)), 50 at 2x, 10 at 42x   g2 = t2  100 at 1x
#   e3 [280,320)  [280,290) of the row at [270,290) + [300,320) = 30 at 1x -- its breadth is 20: the row at [270,290) hits no root
#   g3 = t3 = e4 [10,60)  all 50 at 1x, [20,30) at 2x
WANT = {
    b"e1": ([(0, 100, 130)], (30, 0, 0, 0), 30), b"e2": ([(0, 150, 200)], (50, 50, 10, 0), 50),
    b"c1": ([(0, 110, 120), (0, 160, 170)], (20, 10, 10, 0), 20),
    b"g1": ([(0, 100, 200)], (80, 50, 10, 0), 100), b"t1": ([(0, 100, 200)], (80, 50, 10, 0), 100),
    b"g2": ([(0, 300, 400)], (100, 0, 0, 0), 100), b"t2": ([(0, 300, 400)], (100, 0, 0, 0), 100),
    b"e3": ([(0, 280, 320)], (30, 0, 0, 0), 40),
    b"g3": ([(1, 10, 60)], (50, 10, 0, 0), 50), b"t3": ([(1, 10, 60)], (50, 10, 0, 0), 50), b"e4": ([(1, 10, 60)], (50, 10, 0, 0), 50),
}
REFS = [("chr1", 100000), ("chrZ", 1000), ("chr2", 100000)]  # (BAM / SAM twins: chrZ is not in the index)
NEW_KEYS = ("profile_points", "profile_folds", "profile_kernels_ms", "profile_events_ms", "profile_sort_ms", "profile_scan_ms", "profile_points_ms")


def _head(thresholds, mean_depth=False):
    return (HEAD9 if mean_depth else HEAD6) + b"".join(b"\tbases_ge%d\tfraction_ge%d" % (t, t) for t in thresholds)


def _bgzip(text, block=300):
    return b"".join(synth.bgzf_member(text[i:i + block]) for i in range(0, len(text), block)) + synth.BGZF_EOF


def _coverage(gff, source, out, thresholds=THRESHOLDS, bedgraph=None, mean_depth=False, gpus=1, batch_rows=None, stats=None):
    env = {k: v for k, v in os.environ.items() if k != KNOB}
    if batch_rows:
        env[KNOB] = str(batch_rows)
    cmd = [GFFX, "coverage", "-v", "--gpus", str(gpus), "-i", gff, "-s", source, "-o", out] + (["--mean-depth"] if mean_depth else [])
    if thresholds:
        cmd += ["--thresholds", ",".join(map(str, thresholds))]
    if bedgraph:
        if os.path.exists(bedgraph):
            os.remove(bedgraph)
        cmd += ["--bedgraph", bedgraph]
    if stats:
        if os.path.exists(stats):
            os.remove(stats)
        cmd += ["--stats-json", stats]
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read(), r.stderr


def _split(data, head):
    lines = data.split(b"\n")
    assert lines[0] == head and lines[-1] == b""
    return [ln.split(b"\t") for ln in lines[1:-1]]


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    d = tmp_path_factory.mktemp("thresholds")
    gff = str(d / "h.gff")
    open(gff, "w").write(GFF)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    text = b"# reads\nchrZ\t1\t2\n" + b"".join(b"%s\t%d\t%d\n" % (NAMES[c].encode(), s, e) for c, s, e in ROWS)
    open(str(d / "q.bed"), "wb").write(text)
    open(str(d / "q.bed.gz"), "wb").write(_bgzip(text))
    open(str(d / "empty.bed"), "wb").write(b"# nothing\nchrZ\t1\t2\n")
    tid = {0: 0, 1: 2}
    order = sorted(ROWS + [(9, 1, 2)], key=lambda r: (tid.get(r[0], 1), r[1]))  # coordinate-sorted, chrZ's one read between
    recs = [(tid.get(c, 1), s, ((0, e - s),)) for c, s, e in order]
    synth.write_bam(str(d / "q.bam"), synth.bam_header(REFS), [synth.bam_record(t, p, cigar=cg) for t, p, cg in recs])
    synth.write_sam(str(d / "q.sam"), synth.sam_header(REFS), [synth.sam_line(REFS[t][0], p, cigar=cg) for t, p, cg in recs])
    return dict(dir=d, gff=gff, bed=str(d / "q.bed"))


def test_the_hand_tables_are_the_definition():
    rows = np.array(ROWS, np.uint32)
    points = pf.sweep(rows, 3)
    assert pf.same(points, pf.brute(rows, 3))
    lines = [b"%s\t%d\t%d\t%d\n" % (NAMES[c].encode(), s, e, d) for c, s, e, d in pf.runs(points) if d > 0]
    assert b"".join(lines) == BEDGRAPH
    assert pf.max_depth(points) == 42 and int(points[0][3]) == int(points[0][2])  # nothing on chr3
    for name, (segs, ge, length) in WANT.items():
        q, a, b = (np.array(x, np.uint32) for x in zip(*segs))
        assert int((b - a).sum()) == length, name
        for T, want in zip(THRESHOLDS, ge):
            assert int(pf.covered_at_least(points, T, q, a, b).sum()) == want, (name, T)


def test_hand_written_gff(hand):
    d = hand["dir"]
    plain, _ = _coverage(hand["gff"], hand["bed"], str(d / "plain.tsv"), thresholds=None)
    stats, bg = str(d / "stats.json"), str(d / "depth.bedgraph")
    data, err = _coverage(hand["gff"], hand["bed"], str(d / "th.tsv"), bedgraph=bg, stats=stats)
    got = _split(data, _head(THRESHOLDS))
    # the columns before the new ones: the bytes of the run without the flags
    assert b"\n".join(b"\t".join(f[:6]) for f in got) == b"\n".join(b"\t".join(f) for f in _split(plain, HEAD6))
    assert all(len(f) == 6 + 2 * len(THRESHOLDS) for f in got)
    assert sorted(f[0] for f in got) == sorted(WANT)  # (which rows are printed does not change: nothing of chr3)
    for f in got:
        _, ge, length = WANT[f[0]]
        for k, want in enumerate(ge):
            assert (f[6 + 2 * k], f[7 + 2 * k]) == (b"%d" % want, ("%.6f" % (want / length)).encode()), (f, k)
    e3 = [f for f in got if f[0] == b"e3"][0]
    assert e3[4] == b"20" and e3[6] == b"30"  # breadth counts the rows that hit e3's root; bases_ge1 all rows of the seqid
    assert open(bg, "rb").read() == BEDGRAPH
    st = json.load(open(stats))
    assert all(k in st["counts"] for k in NEW_KEYS), st["counts"]
    assert st["counts"]["profile_points"] == 14 and st["counts"]["profile_folds"] == 1 and st["counts"]["profile_kernels_ms"] > 0
    assert "Depth profile (device)" in json.dumps(st) and b"Depth profile (device) took" in err and b"depth profile of 14 points" in err
    # with --mean-depth: its three columns stay where they are, the new ones come behind them
    md_plain, _ = _coverage(hand["gff"], hand["bed"], str(d / "md.tsv"), thresholds=None, mean_depth=True)
    both = _split(_coverage(hand["gff"], hand["bed"], str(d / "both.tsv"), mean_depth=True)[0], _head(THRESHOLDS, True))
    assert b"\n".join(b"\t".join(f[:9]) for f in both) == b"\n".join(b"\t".join(f) for f in _split(md_plain, HEAD9))
    assert [f[9:] for f in both] == [f[6:] for f in got]
    assert all(f[7] == b"%d" % WANT[f[0]][2] for f in both)  # --mean-depth's length is the fractions' denominator
    # the thresholds in the order given
    swapped = _split(_coverage(hand["gff"], hand["bed"], str(d / "swapped.tsv"), thresholds=(42, 1))[0], _head((42, 1)))
    assert [f[6:] for f in swapped] == [[f[10], f[11], f[6], f[7]] for f in got]
    # --bedgraph alone: the six columns and the file
    alone, _ = _coverage(hand["gff"], hand["bed"], str(d / "alone.tsv"), thresholds=None, bedgraph=bg)
    assert alone == plain and open(bg, "rb").read() == BEDGRAPH


def test_without_the_flags_nothing_new(hand):
    d = hand["dir"]
    stats = str(d / "plain_stats.json")
    plain, err = _coverage(hand["gff"], hand["bed"], str(d / "plain2.tsv"), thresholds=None, stats=stats)
    assert plain.startswith(HEAD6 + b"\n")
    text = open(stats).read()
    assert "profile" not in text.lower() and not any(k in text for k in NEW_KEYS) and b"rofile" not in err


def test_the_same_bytes_from_every_source_device_count_and_batch_size(hand):
    d = hand["dir"]
    bg = str(d / "twin.bedgraph")
    first, _ = _coverage(hand["gff"], hand["bed"], str(d / "first.tsv"), bedgraph=bg)
    assert open(bg, "rb").read() == BEDGRAPH
    for ext in (".bed.gz", ".sam", ".bam"):
        data, _ = _coverage(hand["gff"], str(d / ("q" + ext)), str(d / "twin.tsv"), bedgraph=bg)
        assert data == first and open(bg, "rb").read() == BEDGRAPH, ext
    stats = str(d / "folds.json")
    for gpus, batch_rows in ((2, None), (1, 7), (2, 7)):  # 7 rows a batch: many folds, carried points on every one
        data, _ = _coverage(hand["gff"], hand["bed"], str(d / "knob.tsv"), bedgraph=bg, gpus=gpus, batch_rows=batch_rows, stats=stats)
        assert data == first and open(bg, "rb").read() == BEDGRAPH, (gpus, batch_rows)
        if (gpus, batch_rows) == (1, 7):
            assert json.load(open(stats))["counts"]["profile_folds"] == (len(ROWS) + 6) // 7


def test_an_empty_source(hand):
    d = hand["dir"]
    bg = str(d / "empty.bedgraph")
    data, _ = _coverage(hand["gff"], str(d / "empty.bed"), str(d / "empty.tsv"), bedgraph=bg)
    assert data == _head(THRESHOLDS) + b"\n" and open(bg, "rb").read() == b""
