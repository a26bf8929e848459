"""BAM sources on the GPU: k_bgzf_inflate == zlib, the rows of k_bam_rows == the Python restatement of depth.rs:335-364, and
`gffx depth|coverage -s x.bam` == the oracle's answer for a BED of the same rows (the reference joins both sources the same
way: depth.rs:462-498 against :335-372, coverage.rs:245-262 against :157-190).  Every file here is written through zlib;
tests/test_deflate_streams_gpu.py adds streams of another encoder, tests/test_bam_shapes_gpu.py files of many members and long reads."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from gffx_amd import engine, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


def _corpora():
    rng = np.random.default_rng(3)
    words = [b"gene", b"exon", b"chr1", b"\t", b"ID=", b"Parent=", b"transcript", b";", b"\n"] + [b"%d" % i for i in range(50)]
    text = b"".join(words[i] for i in rng.integers(0, len(words), 40000))
    runs = b"".join(bytes([int(rng.integers(0, 4))]) * int(rng.integers(1, 400)) for _ in range(600))
    return {"random": rng.integers(0, 256, 200000, dtype=np.uint8).tobytes(), "text": text, "runs": runs}


@pytest.mark.parametrize("level,strategy", [(0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FILTERED), (6, zlib.Z_HUFFMAN_ONLY),
                                            (6, zlib.Z_RLE), (6, zlib.Z_FIXED)])
def test_inflate_equals_zlib(level, strategy):
    for name, data in _corpora().items():
        pieces = [data[i:i + synth.BGZF_BLOCK] for i in range(0, len(data), synth.BGZF_BLOCK)]
        stream = b"".join(synth.bgzf_member(p, level, strategy) for p in pieces) + synth.BGZF_EOF
        assert engine.bgzf_inflate(stream) == data, name
    # an empty member alone, and a member of exactly 65536 bytes
    assert engine.bgzf_inflate(synth.BGZF_EOF) == b""
    full = b"ACGT" * 16384
    assert engine.bgzf_inflate(synth.bgzf_member(full, max(level, 1), strategy)) == full  # (stored: too large for one member)


def test_inflate_reports_a_bad_member_by_offset():
    good = synth.bgzf_member(b"hello world" * 100)
    bad = bytearray(synth.bgzf_member(b"x" * 1000))
    bad[-8] ^= 1  # CRC
    with pytest.raises(engine._ffi.GffxHipError) as ei:
        engine.bgzf_inflate(good + bytes(bad))
    assert "CRC32" in str(ei.value) and ("offset %d" % len(good)) in str(ei.value)


REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]


def _bam(tmp_path, layout, big=True, flush_header=True, text=b""):
    recs = synth.bam_test_records(3000, seed=5, refs=REFS, big=big)
    path = str(tmp_path / ("x_%s.bam" % layout))
    hb = synth.write_bam(path, synth.bam_header(REFS, text), [r[0] for r in recs], layout=layout, flush_header=flush_header)
    return path, hb, recs


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
@pytest.mark.parametrize("chunk", ["all", "1", "3"])
def test_bam_rows_equal_the_definition(tmp_path, layout, chunk):
    path, hb, recs = _bam(tmp_path, layout)
    data = open(path, "rb").read()
    ref_seq = [0, 0xFFFFFFFF, 1]  # chrU is not in the index
    want = synth.bam_rows_definition(recs, ref_seq)
    off = engine.bgzf_members(data)
    sizes = np.diff(off)
    chunk_bytes = {"all": 0, "1": 1, "3": int(max(sizes[i:i + 3].sum() for i in range(len(sizes))))}[chunk]
    r = engine.BamReader(ref_seq, hb, chunk_bytes)
    for i in range(0, len(off) - 1, 2):  # fed two members at a time
        r.feed(data[off[i]:off[min(i + 2, len(off) - 1)]])
    r.finish()
    got = r.rows()
    c = r.counts()
    r.close()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert c["kept"] == len(want) and c["records"] == len(recs)
    assert c["unmapped"] == sum(1 for x in recs if x[3] & 4)


def test_bam_multi_block_header_with_records_in_its_last_block(tmp_path):
    text = bytes(np.random.default_rng(1).integers(65, 90, 150000, dtype=np.uint8))  # @CO lines: 3 blocks of header
    for layout in ("aligned", "spanning"):
        path, hb, recs = _bam(tmp_path, layout, big=False, flush_header=False, text=text)
        data = open(path, "rb").read()
        want = synth.bam_rows_definition(recs, [0, 0xFFFFFFFF, 1])
        for chunk in (0, 1):
            assert np.array_equal(engine.bam_rows(data, [0, 0xFFFFFFFF, 1], hb, chunk), want), (layout, chunk)


def _index(tmp_path, seed=1):
    roots = synth.gencode_like_roots(300, seed=seed, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=seed)
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    return gff


def _table(data, head):
    lines = data.split(b"\n")
    assert lines[0] == head and lines[-1] == b""
    return sorted(lines[1:-1])


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
def test_depth_and_coverage_from_bam_equal_the_oracle_on_the_same_bed(tmp_path, layout):
    gff = _index(tmp_path)
    path, hb, recs = _bam(tmp_path, layout)
    rows = synth.bam_rows_definition(recs, [0, 0xFFFFFFFF, 1])
    bed = str(tmp_path / "same.bed")
    synth.write_bed(bed, rows, [n for n, _ in synth.SMALL2])
    for cmd, run, head in (("depth", ob.depth_run, b"id\tchr\tstart\tend\tdepth"),
                           ("coverage", ob.coverage_run, b"id\tchr\tstart\tend\tbreadth\tfraction")):
        want = str(tmp_path / ("want_%s.tsv" % cmd))
        rc, msg = run(gff, bed, want)
        assert rc == 0, msg
        want_rows = _table(open(want, "rb").read(), head)
        assert len(want_rows) > 10
        for chunk in (None, "1", "60000"):
            env = dict(os.environ)
            if chunk:
                env["GFFX_BAM_CHUNK_BYTES"] = chunk
            out = str(tmp_path / ("got_%s.tsv" % cmd))
            r = subprocess.run([GFFX, cmd, "-v", "-i", gff, "-s", path, "-o", out], capture_output=True, env=env)
            assert r.returncode == 0, r.stderr
            assert b"BAM inflate (device)" in r.stderr and b"rows kept" in r.stderr
            assert _table(open(out, "rb").read(), head) == want_rows, (cmd, chunk)
    out = str(tmp_path / "got2.tsv")
    r = subprocess.run([GFFX, "depth", "--gpus", "2", "-i", gff, "-s", path, "-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert _table(open(out, "rb").read(), b"id\tchr\tstart\tend\tdepth") == \
        _table(open(str(tmp_path / "want_depth.tsv"), "rb").read(), b"id\tchr\tstart\tend\tdepth")


def test_bad_bam_files_fail_with_a_message(tmp_path):
    gff = _index(tmp_path)
    path, hb, recs = _bam(tmp_path, "aligned", big=False)
    data = open(path, "rb").read()
    off = engine.bgzf_members(data)
    cases = {"truncated": data[:off[len(off) // 2] + 100],
             "crc": data[:off[3] - 8] + bytes([data[off[3] - 8] ^ 0xFF]) + data[off[3] - 7:]}
    # a record cut short: the last record's final bytes dropped, the stream re-blocked
    stream = synth.bam_header(REFS) + b"".join(r[0] for r in recs)
    cut = stream[:-10]
    cases["record cut"] = b"".join(synth.bgzf_member(cut[i:i + synth.BGZF_BLOCK]) for i in range(0, len(cut), synth.BGZF_BLOCK)) + synth.BGZF_EOF
    for name, blob in cases.items():
        bad = str(tmp_path / ("bad_%s.bam" % name.replace(" ", "_")))
        open(bad, "wb").write(blob)
        r = subprocess.run([GFFX, "depth", "-i", gff, "-s", bad], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stderr.startswith(b"Error: "), (name, r.returncode, r.stderr)
    assert b"offset %d" % off[2] in subprocess.run([GFFX, "depth", "-i", gff, "-s", str(tmp_path / "bad_crc.bam")],
                                                   capture_output=True).stderr
    r = subprocess.run([GFFX, "depth", "-i", gff, "-s", path], capture_output=True)  # a valid run afterwards
    assert r.returncode == 0, r.stderr


def test_missing_eof_marker_warns_and_reads(tmp_path):
    gff = _index(tmp_path)
    path, hb, recs = _bam(tmp_path, "aligned", big=False)
    noeof = str(tmp_path / "noeof.bam")
    open(noeof, "wb").write(open(path, "rb").read()[:-28])
    a = subprocess.run([GFFX, "depth", "-i", gff, "-s", path], capture_output=True)
    b = subprocess.run([GFFX, "depth", "-i", gff, "-s", noeof], capture_output=True)
    assert a.returncode == 0 and b.returncode == 0 and b"EOF marker" in b.stderr
    assert a.stdout == b.stdout


def test_sam_and_cram_are_still_refused_and_a_missing_bam_names_htslib(tmp_path):
    gff = _index(tmp_path)
    for ext in ("sam", "cram"):
        p = tmp_path / ("reads." + ext)
        p.write_bytes(b"x")
        for cmd in ("depth", "coverage"):
            r = subprocess.run([GFFX, cmd, "-i", gff, "-s", str(p)], capture_output=True)
            assert r.returncode == 1 and b"htslib" in r.stderr
    for cmd in ("depth", "coverage"):
        r = subprocess.run([GFFX, cmd, "-i", gff, "-s", str(tmp_path / "missing.bam")], capture_output=True)
        assert r.returncode == 1 and b"htslib" in r.stderr


@pytest.mark.parametrize("bad", ["no_name", "tid", "cigar_beyond"])
def test_malformed_record_fails_and_names_the_block_it_begins_in(tmp_path, bad):
    """A record that k_bam_rows rejects (l_read_name == 0, refID >= n_ref, CIGAR beyond block_size) fails the run, and the
    message names the member in which the record begins -- also when the record spans members and is checked in a later
    chunk, from the carry (1-member chunks)."""
    import struct
    gff = _index(tmp_path)
    recs = [r[0] for r in synth.bam_test_records(300, seed=4, refs=REFS, big=False)]
    big = bytearray(synth.bam_record(0, 500, 0, [(0, 100)], b"big", 100, b"XXZ" + b"B" * 12000 + b"\x00"))
    if bad == "no_name":
        big[12] = 0
    elif bad == "tid":
        big[4:8] = struct.pack("<i", len(REFS))
    else:
        big[16:18] = struct.pack("<H", 60000)
    header = synth.bam_header(REFS)
    at = len(header) + sum(len(r) for r in recs[:150])  # where the bad record begins in the decompressed stream
    path = str(tmp_path / "bad.bam")
    synth.write_bam(path, header, recs[:150] + [bytes(big)] + recs[150:], layout="spanning", block=4096)
    off = engine.bgzf_members(open(path, "rb").read())
    assert (at + len(big)) // 4096 > at // 4096  # it spans members
    want = b"file offset %d" % off[at // 4096]
    for chunk in (None, "1"):
        env = dict(os.environ)
        if chunk:
            env["GFFX_BAM_CHUNK_BYTES"] = chunk
        r = subprocess.run([GFFX, "depth", "-i", gff, "-s", path], capture_output=True, env=env, timeout=120)
        assert r.returncode == 1 and b"malformed BAM record" in r.stderr and want in r.stderr, (chunk, r.stderr)
    good = str(tmp_path / "good.bam")
    synth.write_bam(good, header, recs, layout="spanning", block=4096)
    r = subprocess.run([GFFX, "depth", "-i", gff, "-s", good], capture_output=True)
    assert r.returncode == 0, r.stderr
