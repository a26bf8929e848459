"""BAM files of shapes that tests/test_bam_gpu.py does not have, through the staging code, the framing kernels and k_bam_rows of
device/bgzf.hip: more members in one feed than a sub-batch may hold (65536), sub-batches of thousands of members (k_scan with
several elements per thread, k_frame_guess / k_frame_list with many blocks, frame_fix over thousands of segments that do not
begin with a record), and long reads of 64 KiB - 1 MB back to back in the middle of the file, whose carry grows over many
sub-batches.  Expected rows and counters come from synth.bam_rows_definition and the record list; the end-to-end runs are
compared with the oracle on a BED of the same rows."""
import os
import subprocess

import numpy as np
import pytest

from gffx_amd import engine, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]
REF_SEQ = [0, 0xFFFFFFFF, 1]  # chrU is not in the index
HEADER = synth.bam_header(REFS)


def _file(blocks, level=1):
    return b"".join(synth.bgzf_member(b, level) for b in blocks) + synth.BGZF_EOF


@pytest.fixture(scope="module")
def small_recs():
    return synth.bam_test_records(70000, seed=8, refs=REFS, big=False)


@pytest.fixture(scope="module")
def small_members(small_recs):
    """One record per member, the header in a member of its own."""
    return _file([HEADER] + [r[0] for r in small_recs])


@pytest.fixture(scope="module")
def long_recs():
    return synth.bam_long_read_records(400, seed=3, refs=REFS)


@pytest.fixture(scope="module")
def long_files(long_recs):
    return {layout: _file(synth.bgzf_blocks(HEADER, [r[0] for r in long_recs], layout)) for layout in ("aligned", "spanning")}


def _read(data, recs, chunk_bytes=0, feed_members=0):
    """The whole file through a BamReader: rows and counters against the definition."""
    want = synth.bam_rows_definition(recs, REF_SEQ)
    r = engine.BamReader(REF_SEQ, len(HEADER), chunk_bytes)
    try:
        if feed_members:
            off = engine.bgzf_members(data)
            for i in range(0, len(off) - 1, feed_members):
                r.feed(data[off[i]:off[min(i + feed_members, len(off) - 1)]])
        else:
            r.feed(data)
        r.finish()
        got, c = r.rows(), r.counts()
    finally:
        r.close()
    assert c["records"] == len(recs)
    assert c["kept"] == len(want) and c["unmapped"] == sum(1 for x in recs if x[3] & 4)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_more_members_in_one_feed_than_a_sub_batch_holds(small_members, small_recs):
    n_members = len(engine.bgzf_members(small_members)) - 1
    assert n_members == len(small_recs) + 2 and n_members > 65536  # gffx_hip_bam_feed cuts at 65536 members: a second sub-batch
    _read(small_members, small_recs)


@pytest.mark.parametrize("per_batch", [1500, 5000])
def test_sub_batches_of_thousands_of_members(small_members, small_recs, per_batch):
    n_members = len(engine.bgzf_members(small_members)) - 1
    chunk_bytes = len(small_members) * per_batch // n_members
    _read(small_members, small_recs, chunk_bytes)
    _read(small_members, small_recs, chunk_bytes, feed_members=1000)


def test_thousands_of_segments_that_do_not_begin_with_a_record(small_recs):
    records = [r[0] for r in small_recs]
    spanning = _file(synth.bgzf_blocks(HEADER, records, "spanning", block=4096))
    n = len(engine.bgzf_members(spanning)) - 1
    assert n > 2500
    _read(spanning, small_recs)  # one sub-batch: frame_fix walks the chain through all of them
    _read(spanning, small_recs, len(spanning) // 3 + 4096)
    aligned = _file(synth.bgzf_blocks(HEADER, records, "aligned", block=256))  # most records are cut into several blocks
    n = len(engine.bgzf_members(aligned)) - 1
    assert n > 30000
    _read(aligned, small_recs, len(aligned) * 3000 // n)
    _read(aligned, small_recs)


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
@pytest.mark.parametrize("chunk", ["1", "3", "default"])
def test_long_reads_in_the_middle_of_the_file(long_files, long_recs, layout, chunk):
    data = long_files[layout]
    sizes = np.diff(engine.bgzf_members(data))
    assert max(len(r[0]) for r in long_recs) == 1_000_000 and len(sizes) > 80
    chunk_bytes = {"1": 1, "3": int(max(sizes[i:i + 3].sum() for i in range(len(sizes)))), "default": 0}[chunk]
    _read(data, long_recs, chunk_bytes)
    _read(data, long_recs, chunk_bytes, feed_members=5)


@pytest.mark.parametrize("chunk_bytes", [1, 0])
def test_a_file_ending_inside_a_long_read(long_recs, chunk_bytes):
    sizes = [len(r[0]) for r in long_recs]
    second = next(i for i in range(1, len(sizes)) if sizes[i] == sizes[i - 1] == 1_000_000)  # of two 1 MB records in a row
    stream = HEADER + b"".join(r[0] for r in long_recs[:second + 1])
    cut = stream[:-400_000]
    data = _file([cut[i:i + synth.BGZF_BLOCK] for i in range(0, len(cut), synth.BGZF_BLOCK)])
    r = engine.BamReader(REF_SEQ, len(HEADER), chunk_bytes)
    try:
        r.feed(data)
        with pytest.raises(engine._ffi.GffxHipError) as ei:
            r.finish()
        assert "ends inside a record (600000 bytes" in str(ei.value)
        assert r.counts()["records"] == second
    finally:
        r.close()
    _read(_file(synth.bgzf_blocks(HEADER, [x[0] for x in long_recs[:second + 1]], "spanning")), long_recs[:second + 1], chunk_bytes)


def _table(data, head):
    lines = data.split(b"\n")
    assert lines[0] == head and lines[-1] == b""
    return sorted(lines[1:-1])


@pytest.mark.parametrize("shape", ["small members", "long reads"])
def test_depth_and_coverage_equal_the_oracle_on_the_same_bed(tmp_path, request, shape):
    if shape == "small members":
        recs, data = request.getfixturevalue("small_recs"), request.getfixturevalue("small_members")
    else:
        recs, data = request.getfixturevalue("long_recs"), request.getfixturevalue("long_files")["spanning"]
    roots = synth.gencode_like_roots(300, seed=1, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=1)
    assert subprocess.run([GFFX, "index", "-i", gff], timeout=300).returncode == 0
    path = str(tmp_path / "x.bam")
    open(path, "wb").write(data)
    bed = str(tmp_path / "same.bed")
    synth.write_bed(bed, synth.bam_rows_definition(recs, REF_SEQ), [n for n, _ in synth.SMALL2])
    for cmd, run, head in (("depth", ob.depth_run, b"id\tchr\tstart\tend\tdepth"),
                           ("coverage", ob.coverage_run, b"id\tchr\tstart\tend\tbreadth\tfraction")):
        want = str(tmp_path / ("want_%s.tsv" % cmd))
        rc, msg = run(gff, bed, want)
        assert rc == 0, msg
        want_rows = _table(open(want, "rb").read(), head)
        assert len(want_rows) > 10
        for chunk in (None, "1"):
            env = dict(os.environ)
            if chunk:
                env["GFFX_BAM_CHUNK_BYTES"] = chunk
            out = str(tmp_path / ("got_%s.tsv" % cmd))
            r = subprocess.run([GFFX, cmd, "-v", "-i", gff, "-s", path, "-o", out], capture_output=True, env=env, timeout=600)
            assert r.returncode == 0, r.stderr
            assert b"BAM inflate (device)" in r.stderr and b"rows kept" in r.stderr
            assert _table(open(out, "rb").read(), head) == want_rows, (cmd, chunk)
