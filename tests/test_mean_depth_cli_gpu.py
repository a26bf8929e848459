"""`gffx coverage --mean-depth`: three more columns -- bases, length, mean_depth -- beside the six the command prints.  A hand-written
GFF with the answers worked out below; the first six columns byte for byte those of the run without the flag; the same bytes
whatever the source format, the device count or the batch size; and without the flag nothing new anywhere."""
import json
import os
import subprocess

import numpy as np
import pytest

import _pileup_definition as pd
from gffx_amd import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
HEAD6 = b"id\tchr\tstart\tend\tbreadth\tfraction"
HEAD9 = HEAD6 + b"\tbases\tlength\tmean_depth"
KNOB = "GFFX_COVERAGE_BATCH_ROWS"
TIMEOUT = 120

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
# rows (seqid, start, end): one deep on e1, two deep on e2, forty deep on c1's second line, tiled end to end over g2 (the same
# breadth as a pile, a depth of exactly 1), one row over the part of e3 outside its gene (it hits no root at all), two on chr2
ROWS = ([(0, 100, 130)] + [(0, 150, 200)] * 2 + [(0, 160, 170)] * 40 + [(0, 300 + 20 * k, 320 + 20 * k) for k in range(5)] +
        [(0, 270, 290)] + [(1, 0, 30), (1, 20, 80)])
# id -> (the ID's lines, bases, length, mean_depth), by hand:
#   e1  30 / 30            e2  2 * 50 + 40 * 10 = 500 / 50         c1  (10) + (2 * 10 + 40 * 10) = 430 / 20
#   g1 = t1  30 + 100 + 400 = 530 / 100                             g2 = t2  5 * 20 = 100 / 100
#   e3  20 of the first tile + 10 of the row at [270, 290) = 30 / 40
#   g3 = t3 = e4  20 of [0, 30) + 40 of [20, 80) = 60 / 50
WANT = {
    b"g1": ([(0, 100, 200)], 530, 100, b"5.300000"), b"t1": ([(0, 100, 200)], 530, 100, b"5.300000"),
    b"e1": ([(0, 100, 130)], 30, 30, b"1.000000"), b"e2": ([(0, 150, 200)], 500, 50, b"10.000000"),
    b"c1": ([(0, 110, 120), (0, 160, 170)], 430, 20, b"21.500000"),
    b"g2": ([(0, 300, 400)], 100, 100, b"1.000000"), b"t2": ([(0, 300, 400)], 100, 100, b"1.000000"),
    b"e3": ([(0, 280, 320)], 30, 40, b"0.750000"),
    b"g3": ([(1, 10, 60)], 60, 50, b"1.200000"), b"t3": ([(1, 10, 60)], 60, 50, b"1.200000"), b"e4": ([(1, 10, 60)], 60, 50, b"1.200000"),
}
REFS = [("chr1", 100000), ("chrZ", 1000), ("chr2", 100000)]  # (BAM / SAM twins: chrZ is not in the index)


def _bgzip(text, block=300):
    return b"".join(synth.bgzf_member(text[i:i + block]) for i in range(0, len(text), block)) + synth.BGZF_EOF


def _coverage(gff, source, out, flag=True, gpus=1, batch_rows=None, stats=None):
    env = {k: v for k, v in os.environ.items() if k != KNOB}
    if batch_rows:
        env[KNOB] = str(batch_rows)
    cmd = [GFFX, "coverage", "-v", "--gpus", str(gpus), "-i", gff, "-s", source, "-o", out] + (["--mean-depth"] if flag else [])
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
    d = tmp_path_factory.mktemp("mean_depth")
    gff = str(d / "h.gff")
    open(gff, "w").write(GFF)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    text = b"# reads\nchrZ\t1\t2\n" + b"".join(b"%s\t%d\t%d\n" % (NAMES[c].encode(), s, e) for c, s, e in ROWS)
    open(str(d / "q.bed"), "wb").write(text)
    open(str(d / "q.bed.gz"), "wb").write(_bgzip(text))
    tid = {0: 0, 1: 2}
    order = sorted(ROWS + [(9, 1, 2)], key=lambda r: (tid.get(r[0], 1), r[1]))  # coordinate-sorted, chrZ's one read between
    recs = [(tid.get(c, 1), s, ((0, e - s),)) for c, s, e in order]
    synth.write_bam(str(d / "q.bam"), synth.bam_header(REFS), [synth.bam_record(t, p, cigar=cg) for t, p, cg in recs])
    synth.write_sam(str(d / "q.sam"), synth.sam_header(REFS), [synth.sam_line(REFS[t][0], p, cigar=cg) for t, p, cg in recs])
    return dict(dir=d, gff=gff, bed=str(d / "q.bed"))


def test_the_hand_table_is_the_definition():
    rows = np.array(ROWS, np.uint32)
    for name, (lines, bases, length, mean) in WANT.items():
        q, a, b = (np.array(x, np.uint32) for x in zip(*lines))
        assert int(pd.brute(rows, q, a, b).sum()) == bases and int((b - a).sum()) == length, name
        assert bases < 2 ** 53 and ("%.6f" % (bases / length)).encode() == mean, name


def test_hand_written_gff(hand):
    d = hand["dir"]
    plain, _ = _coverage(hand["gff"], hand["bed"], str(d / "plain.tsv"), flag=False)
    stats = str(d / "stats.json")
    data, err = _coverage(hand["gff"], hand["bed"], str(d / "md.tsv"), stats=stats)
    got = _split(data, HEAD9)
    # the first six columns: the bytes of the run without the flag
    assert b"\n".join(b"\t".join(f[:6]) for f in got) == b"\n".join(b"\t".join(f) for f in _split(plain, HEAD6))
    assert all(len(f) == 9 for f in got)
    assert sorted(f[0] for f in got) == sorted(WANT)  # (nothing of chr3: no row hits g4)
    for f in got:
        _, bases, length, mean = WANT[f[0]]
        assert (f[6], f[7], f[8]) == (b"%d" % bases, b"%d" % length, mean), f
    st = json.load(open(stats))
    assert st["counts"]["pileup_segments"] == 15  # the segments of ALL blocks, chr3's too (g4's block is never hit): 6 + 3 + 3 + 3
    assert st["counts"]["pileup_kernels_ms"] > 0 and "Pileup (device)" in json.dumps(st)
    assert b"Pileup (device) took" in err and b"pileup of 15 segments" in err


def test_the_same_bytes_from_every_source_device_count_and_batch_size(hand):
    d = hand["dir"]
    first, _ = _coverage(hand["gff"], hand["bed"], str(d / "first.tsv"))
    for ext in (".bed.gz", ".sam", ".bam"):
        data, _ = _coverage(hand["gff"], str(d / ("q" + ext)), str(d / "twin.tsv"))
        assert data == first, ext
    for gpus, batch_rows in ((2, None), (1, 7), (1, 1000), (2, 7), (3, 7)):
        data, _ = _coverage(hand["gff"], hand["bed"], str(d / "knob.tsv"), gpus=gpus, batch_rows=batch_rows)
        assert data == first, (gpus, batch_rows)


def _id_lines(gff_path, names):
    """ID -> (seqid number of its first line, its lines as (start, end), 0-based half-open), in file order."""
    ids = {}
    for ln in open(gff_path):
        f = ln.rstrip("\n").split("\t")
        if ln.startswith("#") or len(f) < 9:
            continue
        for kv in f[8].split(";"):
            if kv.startswith("ID="):
                ids.setdefault(kv[3:], (names.index(f[0]), []))[1].append((int(f[3]) - 1, int(f[4])))
    return ids


def _merge(lines):  # merge_intervals: sort by start, merge while s <= current end
    out = []
    for s, e in sorted(lines):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def test_seeded_gff_with_and_without_the_flag(tmp_path):
    names = [n for n, _ in synth.SMALL2]
    roots = synth.gencode_like_roots(300, seed=4, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=4)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0
    regions = synth.synth_bed(4000, seed=14, chroms=synth.SMALL2, width=(1, 3000), edge_frac=0.1, roots=roots)
    regions = regions[regions[:, 1] < regions[:, 2]]
    bed = str(tmp_path / "q.bed")
    synth.write_bed(bed, regions, names)
    # flag off: the rows of the reference's restatement, six columns, no pileup anywhere
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.coverage_run(gff, bed, want)
    assert rc == 0, msg
    stats = str(tmp_path / "stats.json")
    plain, err = _coverage(gff, bed, str(tmp_path / "plain.tsv"), flag=False, stats=stats)
    assert sorted(plain.split(b"\n")[1:-1]) == sorted(open(want, "rb").read().split(b"\n")[1:-1]) and plain.startswith(HEAD6 + b"\n")
    assert "pileup" not in open(stats).read().lower() and b"ileup" not in err
    # flag on: the same six columns, the three new ones by the definition over the ID's lines
    got = _split(_coverage(gff, bed, str(tmp_path / "md.tsv"), batch_rows=900)[0], HEAD9)
    assert b"\n".join(b"\t".join(f[:6]) for f in got) + b"\n" == plain[len(HEAD6) + 1:] and len(got) > 50
    ids = _id_lines(gff, names)
    q, a, b, owner = [], [], [], []
    for k, f in enumerate(got):
        c, lines = ids[f[0].decode()]
        for s, e in _merge(lines):
            q.append(c), a.append(s), b.append(e), owner.append(k)
    q, a, b, owner = (np.array(x, np.uint32) for x in (q, a, b, owner))
    bases = np.zeros(len(got), np.uint64)
    np.add.at(bases, owner, pd.brute(regions, q, a, b))
    length = np.zeros(len(got), np.uint64)
    np.add.at(length, owner, (b - a).astype(np.uint64))
    assert np.any(bases > length) and np.any((bases > 0) & (bases < length))  # (features more and less than one deep)
    for k, f in enumerate(got):
        mean = "%.6f" % (int(bases[k]) / int(length[k])) if length[k] else "0.000000"
        assert (f[6], f[7], f[8]) == (b"%d" % bases[k], b"%d" % length[k], mean.encode()), f
