"""`gffx coverage --gpus N` on the batched, device-side union path: rows == the oracle's restatement of
commands/coverage.rs for every N and batch size, bytes == the `--gpus 1` output.  Logical devices beyond the visible
ones wrap onto the same GPU (as in test_depth_gpu.py), so a one-GPU machine runs every case."""
import json
import os
import subprocess

import pytest

from gffx_amd import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
HEAD = b"id\tchr\tstart\tend\tbreadth\tfraction"
KNOB = "GFFX_COVERAGE_BATCH_ROWS"


def _rows(data):
    lines = data.split(b"\n")
    assert lines[0] == HEAD and lines[-1] == b""
    return sorted(lines[1:-1])


def _coverage(gff, source, out, gpus, batch_rows=None, stats=None):
    env = dict(os.environ)
    env.pop(KNOB, None)
    if batch_rows:
        env[KNOB] = str(batch_rows)
    cmd = [GFFX, "coverage", "-v", "--gpus", str(gpus), "-i", gff, "-s", source, "-o", out]
    if stats:
        cmd += ["--stats-json", stats]
    r = subprocess.run(cmd, capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    return r.stderr


def _host_segments(stderr):
    for line in stderr.split(b"\n"):
        if b"evaluated on the host)" in line:
            return int(line.split(b"(")[1].split()[0])
    raise AssertionError("no segment line in: %r" % stderr)


@pytest.mark.parametrize("seed", [2, 3])
def test_cli_equals_the_oracle_for_every_device_count_and_batch_size(tmp_path, seed):
    roots = synth.gencode_like_roots(300, seed=seed, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=seed, quirks=True)  # `region` lines sit in the previous gene's block and stick out of its root
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    n_rows = 4000
    regions = synth.synth_bed(n_rows, seed=seed + 10, chroms=synth.SMALL2, width=(1, 3000), edge_frac=0.1, roots=roots)
    bed = str(tmp_path / "q.bed")
    synth.write_bed(bed, regions, [n for n, _ in synth.SMALL2], extra_lines=["# header\n", "chrZ\t1\t2\n", "chr1\t7\n"])
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.coverage_run(gff, bed, want)
    assert rc == 0, msg
    want_rows = _rows(open(want, "rb").read())
    assert len(want_rows) > 50
    first = None
    for gpus in (1, 2, 3):
        for batch_rows in (None, 200):  # 200: >= 6 batches for each of three devices
            out = str(tmp_path / ("got_%d_%s.tsv" % (gpus, batch_rows)))
            stats = str(tmp_path / "stats.json")
            err = _coverage(gff, bed, out, gpus, batch_rows, stats)
            assert _host_segments(err) > 0  # the exact path for segments outside their root ran
            data = open(out, "rb").read()
            assert _rows(data) == want_rows, (gpus, batch_rows)
            first = data if first is None else first
            assert data == first, (gpus, batch_rows)  # bytes, not only rows: the order is the block order
            st = json.load(open(stats))
            dev = st["devices"]
            assert st["counts"]["gpus"] == gpus and len(dev) == gpus and st["counts"]["union_spans"] > 0
            kept = int(st["counts"]["rows"])
            assert sum(d["rows"] for d in dev) == kept and 0 < kept <= n_rows
            if batch_rows:
                assert all(d["rows"] >= 5 * batch_rows for d in dev)  # at least 5 batches on every device
            # the rows are uploaded once
            assert st["counts"]["upload_bytes"] == 12 * kept and (b"rows uploaded once: %d bytes" % (12 * kept)) in err


def test_a_child_beyond_its_gene_is_measured_against_the_roots_own_rows(tmp_path):
    """Rows A = [0, 10) and B = [5, 20); a root at [15, 30) that only B hits; its child e1 covers [2, 8).  Under the union
    of all rows, [0, 20), e1 would have 6 covered bases; the root's own list holds only B and gives 3 (coverage.rs:401)."""
    gff = str(tmp_path / "h.gff")
    open(gff, "w").write("##gff-version 3\n"
                         "chr1\tt\tgene\t16\t30\t.\t+\t.\tID=g1;gene_name=G1\n"
                         "chr1\tt\tmRNA\t16\t30\t.\t+\t.\tID=t1;Parent=g1\n"
                         "chr1\tt\texon\t3\t8\t.\t+\t.\tID=e1;Parent=t1\n"
                         "chr1\tt\texon\t20\t25\t.\t+\t.\tID=e2;Parent=t1\n"
                         "chr1\tt\tgene\t101\t200\t.\t+\t.\tID=g2;gene_name=G2\n"
                         "chr1\tt\tmRNA\t101\t200\t.\t+\t.\tID=t2;Parent=g2\n"
                         "chr1\tt\texon\t101\t150\t.\t+\t.\tID=e3;Parent=t2\n")
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    bed = str(tmp_path / "h.bed")
    open(bed, "w").write("chr1\t0\t10\nchr1\t5\t20\n")
    literal = sorted([b"e1\tchr1\t2\t8\t3\t0.500000", b"e2\tchr1\t19\t25\t1\t0.166667", b"g1\tchr1\t15\t30\t5\t0.333333",
                      b"t1\tchr1\t15\t30\t5\t0.333333"])
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.coverage_run(gff, bed, want)
    assert rc == 0, msg
    assert _rows(open(want, "rb").read()) == literal
    for gpus, batch_rows in ((1, None), (2, None), (2, 1)):
        out = str(tmp_path / "got.tsv")
        err = _coverage(gff, bed, out, gpus, batch_rows)
        assert _host_segments(err) == 1
        assert _rows(open(out, "rb").read()) == literal, (gpus, batch_rows)


REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]


def test_bam_source_on_two_devices_equals_the_oracle_on_the_same_bed(tmp_path):
    roots = synth.gencode_like_roots(300, seed=1, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=1)
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    recs = synth.bam_test_records(3000, seed=5, refs=REFS, big=True)
    bam = str(tmp_path / "x.bam")
    synth.write_bam(bam, synth.bam_header(REFS), [r[0] for r in recs], layout="spanning")
    rows = synth.bam_rows_definition(recs, [0, 0xFFFFFFFF, 1])  # chrU is not in the index
    bed = str(tmp_path / "same.bed")
    synth.write_bed(bed, rows, [n for n, _ in synth.SMALL2])
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.coverage_run(gff, bed, want)
    assert rc == 0, msg
    want_rows = _rows(open(want, "rb").read())
    assert len(want_rows) > 10
    for batch_rows in (None, 300):
        out = str(tmp_path / "got.tsv")
        err = _coverage(gff, bam, out, 2, batch_rows)
        assert b"BAM inflate (device)" in err
        assert _rows(open(out, "rb").read()) == want_rows, batch_rows


def test_three_million_rows_on_two_devices(tmp_path):
    """Scale: 3 000 000 BED rows (width U[100, 10 000], GRCh38-shaped) against a 5 000-gene GENCODE-shaped GFF (280 000 output
    rows), --gpus 2 with the default batch size.  At this size the one-thread host sort of 3 M keys that the union used to
    need is the dominant device-side stage of the command.  Sized on the CPU: the oracle's coverage_run, which is
    one-threaded, takes 5.7 s for this input (66 s with 20 000 genes: its cost grows with the GFF, not the rows); writing and
    indexing the inputs takes about 2 s more."""
    n = 3_000_000
    roots = synth.gencode_like_roots(5000, seed=21)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3_fast(gff, roots, seed=21)
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    regions = synth.synth_bed(n, seed=22)
    bed = str(tmp_path / "q.bed")
    synth.write_bed_fast(bed, regions, roots["names"])
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.coverage_run(gff, bed, want)
    assert rc == 0, msg
    want_rows = _rows(open(want, "rb").read())
    assert len(want_rows) > 100000
    out, stats = str(tmp_path / "got.tsv"), str(tmp_path / "stats.json")
    _coverage(gff, bed, out, 2, 1 << 19, stats)
    assert _rows(open(out, "rb").read()) == want_rows
    st = json.load(open(stats))
    assert st["counts"]["union_spans"] > 0 and st["counts"]["gpus"] == 2 and len(st["devices"]) == 2
    assert sum(d["rows"] for d in st["devices"]) == n == st["counts"]["rows"]
    assert all(d["rows"] > 0 and d["spans"] > 0 for d in st["devices"])
    assert st["counts"]["upload_bytes"] == 12 * n
