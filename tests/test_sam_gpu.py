"""SAM sources on the GPU: the rows of k_sam_line_* / k_sam_rows == the Python restatement (synth.sam_rows_definition) on plain
and BGZF-compressed text, whatever the chunk size and however the text is fed; the same records give the same rows as BAM and
as SAM; and `gffx depth|coverage -s x.sam` == the oracle's answer for a BED of the same rows.  The failure cases are error
returns of well-formed launches: a malformed line is read inside its bounds and reported by its line number."""
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
NAMES = [n for n, _ in REFS]
REF_SEQ = [0, 0xFFFFFFFF, 1]  # chrU is not in the index


@pytest.fixture(scope="module")
def big():
    """3000 records (and the three special ones, the 150 KB-tag record among them), their lines and their rows."""
    recs = synth.bam_test_records(3000, seed=5, refs=REFS, big=True)
    return recs, synth.sam_records_from(recs, REFS), synth.sam_rows_definition(recs, REF_SEQ), synth.sam_counts_definition(recs, REF_SEQ)


@pytest.fixture(scope="module")
def small():
    recs = synth.bam_test_records(60, seed=6, refs=REFS, big=False)
    return recs, synth.sam_records_from(recs, REFS), synth.sam_rows_definition(recs, REF_SEQ), synth.sam_counts_definition(recs, REF_SEQ)


def _text(tmp_path, lines, header=None, **kw):
    path = str(tmp_path / "x.sam")
    hb = synth.write_sam(path, synth.sam_header(REFS) if header is None else header, lines, **kw)
    return open(path, "rb").read(), hb


def _check(data, hb, want, counts, **kw):
    c = {}
    got = engine.sam_rows(data, NAMES, REF_SEQ, hb, counts=c, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), kw
    assert c == counts, (kw, c, counts)


@pytest.mark.parametrize("chunk,feed", [(0, 0), (4096, 0), (0, 1000), (4096, 1000)])
@pytest.mark.parametrize("final_newline", [True, False])
def test_plain_rows_equal_the_definition(tmp_path, big, chunk, feed, final_newline):
    """chunk 4096: most chunks end inside a line, and the 150 KB-tag record (36.6 chunks long) lies across 37 chunks or more."""
    recs, lines, want, counts = big
    assert max(len(ln) for ln in lines) > 36 * 4096
    data, hb = _text(tmp_path, lines, final_newline=final_newline)
    _check(data, hb, want, counts, chunk_bytes=chunk, feed_bytes=feed)


@pytest.mark.parametrize("chunk,feed", [(257, 0), (0, 1), (257, 1)])
def test_plain_rows_of_a_small_file_in_tiny_chunks_and_pieces(tmp_path, small, chunk, feed):
    recs, lines, want, counts = small
    data, hb = _text(tmp_path, lines)
    assert len(want) > 20
    _check(data, hb, want, counts, chunk_bytes=chunk, feed_bytes=feed)
    crlf, hb2 = _text(tmp_path, lines, newline=b"\r\n")
    _check(crlf, hb2, want, counts, chunk_bytes=chunk, feed_bytes=feed)


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
@pytest.mark.parametrize("chunk", ["all", "1"])
def test_bgzf_rows_equal_the_definition(tmp_path, big, layout, chunk):
    recs, lines, want, counts = big
    data, hb = _text(tmp_path, lines, bgzf=True, layout=layout)
    assert len(engine.bgzf_members(data)) > 8
    _check(data, hb, want, counts, bgzf=True, chunk_bytes={"all": 0, "1": 1}[chunk], feed_members=2)


def test_a_file_without_header_and_a_file_that_is_all_header(tmp_path, small):
    recs, lines, want, counts = small
    data, hb = _text(tmp_path, lines, header=b"")
    assert hb == 0
    _check(data, 0, want, counts)
    only = synth.sam_header(REFS)
    for text in (only, only[:-1]):  # (the last header line with and without its newline)
        c = {}
        got = engine.sam_rows(text, NAMES, REF_SEQ, len(text), counts=c)
        assert len(got) == 0 and c == {"lines": 0, "unmapped": 0, "no_seq": 0, "kept": 0}


@pytest.mark.parametrize("name,line_bytes", [(b"", 15), (b"c", 16)])
def test_a_chunk_of_nothing_but_the_shortest_kept_lines(name, line_bytes):
    """The densest text there is: 1 MiB of lines of 14 (the empty reference name) or 15 bytes and their newlines, every one
    kept -- 12 bytes of rows per 15 bytes of text, what sam::max_kept_lines sizes k_sam_rows' output buffer for.  In one chunk,
    in 4096-byte chunks, and with the last line's newline missing (the bound is exact there)."""
    n = (1 << 20) // line_bytes
    pos = 1 + np.arange(n) % 9
    text = b"".join(b"\t0\t%s\t%d\t\t1M\t\t\t\t\t\n" % (name, p) for p in pos.tolist())
    assert len(text) == n * line_bytes
    want = np.stack([np.zeros(n, np.uint32), (pos - 1).astype(np.uint32), pos.astype(np.uint32)], axis=1)
    for data, chunk in ((text, 0), (text[:-1], 0), (text, 4096)):
        c = {}
        got = engine.sam_rows(data, [name], [0], 0, chunk_bytes=chunk, counts=c)
        assert got.shape == want.shape and np.array_equal(got, want), (chunk, len(data))
        assert c == {"lines": n, "unmapped": 0, "no_seq": 0, "kept": n}


def test_same_records_as_bam_and_as_sam(tmp_path, big):
    """Records with a CIGAR give the same rows from a BAM file and from a SAM file.  A record without flag 0x4 whose CIGAR is
    `*` is kept by the BAM reader (end = pos + 1) and dropped by the SAM reader: the ASSUMED behaviour of htslib's SAM parser
    ("mapped query must have a CIGAR; treated as unmapped"), device/sam_core.hpp."""
    recs = [r for r in big[0] if r[4]]
    bam = str(tmp_path / "x.bam")
    hb = synth.write_bam(bam, synth.bam_header(REFS), [r[0] for r in recs])
    from_bam = engine.bam_rows(open(bam, "rb").read(), REF_SEQ, hb)
    data, shb = _text(tmp_path, synth.sam_records_from(recs, REFS))
    from_sam = engine.sam_rows(data, NAMES, REF_SEQ, shb)
    assert len(from_bam) > 1000 and np.array_equal(from_bam, from_sam)
    star = [(synth.bam_record(0, 100, 0, [], b"a"), 0, 100, 0, []), (synth.bam_record(0, 200, 0, [(0, 10)], b"b"), 0, 200, 0, [(0, 10)])]
    hb = synth.write_bam(bam, synth.bam_header(REFS), [r[0] for r in star])
    assert engine.bam_rows(open(bam, "rb").read(), REF_SEQ, hb).tolist() == [[0, 100, 101], [0, 200, 210]]
    data, shb = _text(tmp_path, synth.sam_records_from(star, REFS))
    c = {}
    assert engine.sam_rows(data, NAMES, REF_SEQ, shb, counts=c).tolist() == [[0, 200, 210]]
    assert c == {"lines": 2, "unmapped": 1, "no_seq": 0, "kept": 1}


LONG_GROUPS = ((synth.BGZF_BLOCK, 1), (synth.BGZF_BLOCK + 1, 2), (2 * synth.BGZF_BLOCK, 2), (300_000, 2), (1_000_000, 2))


@pytest.fixture(scope="module")
def long_reads():
    """Lines longer than a BGZF block and up to 1 MB, back to back; a CIGAR of 70,000 operations; a line whose sixth field
    ends beyond byte 256 (a 300-byte QNAME)."""
    recs = synth.bam_long_read_records(300, seed=8, refs=REFS, groups=LONG_GROUPS)
    lines = synth.sam_records_from(recs, REFS)
    many = [(0, 3), (1, 2)] * 34_999 + [(2, 5), (0, 1)]
    extra = [((None, 2, 5000, 0, many), synth.sam_line("chr2", 5000, 0, many, b"manyops", 100)),
             ((None, 0, 777, 16, [(0, 90)]), synth.sam_line("chr1", 777, 16, [(0, 90)], b"n" * 300, 90))]
    assert len(many) == 70_000 and extra[1][1].index(b"\t90M\t") > 256
    for at, (rec, line) in zip((40, 200), extra):
        recs.insert(at, rec)
        lines.insert(at, line)
    assert sum(len(x) for x in lines) < 8_000_000 and max(len(x) for x in lines) > 900_000
    return recs, lines, synth.sam_rows_definition(recs, REF_SEQ), synth.sam_counts_definition(recs, REF_SEQ)


@pytest.mark.parametrize("kind", ["plain", "plain 64 KiB chunks", "aligned", "spanning", "spanning 1-member chunks"])
def test_long_lines(tmp_path, long_reads, kind):
    recs, lines, want, counts = long_reads
    if kind.startswith("plain"):
        data, hb = _text(tmp_path, lines)
        _check(data, hb, want, counts, chunk_bytes=65536 if "64" in kind else 0)
    else:
        data, hb = _text(tmp_path, lines, bgzf=True, layout=kind.split()[0])
        _check(data, hb, want, counts, bgzf=True, chunk_bytes=1 if "1-member" in kind else 0)


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
def test_bgzf_header_of_three_members_with_lines_in_its_last_member(tmp_path, small, layout):
    recs, lines, want, counts = small
    text = b"".join(b"@CO\t" + bytes([65 + i % 26]) * 1000 + b"\n" for i in range(150))
    header = synth.sam_header(REFS, text)
    data, hb = _text(tmp_path, lines, header=header, bgzf=True, layout=layout, flush_header=False)
    off = engine.bgzf_members(data)
    assert 2 * synth.BGZF_BLOCK < hb < 3 * synth.BGZF_BLOCK and len(off) - 1 <= 5  # header and lines share the third member
    for chunk in (0, 1):
        _check(data, hb, want, counts, bgzf=True, chunk_bytes=chunk)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gff(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_index")
    roots = synth.gencode_like_roots(300, seed=1, chroms=synth.SMALL2)
    path = str(d / "s.gff")
    synth.write_gff3(path, roots, seed=1)
    assert subprocess.run([GFFX, "index", "-i", path]).returncode == 0
    return path


def _table(data, head):
    lines = data.split(b"\n")
    assert lines[0] == head and lines[-1] == b""
    return sorted(lines[1:-1])


HEADS = {"depth": b"id\tchr\tstart\tend\tdepth", "coverage": b"id\tchr\tstart\tend\tbreadth\tfraction"}


@pytest.mark.parametrize("source", ["plain", "aligned", "spanning"])
def test_depth_and_coverage_from_sam_equal_the_oracle_on_the_same_bed(tmp_path, gff, big, source):
    recs, lines, rows, counts = big
    path = str(tmp_path / "reads.sam")
    synth.write_sam(path, synth.sam_header(REFS), lines, bgzf=source != "plain", layout=source if source != "plain" else "aligned")
    bed = str(tmp_path / "same.bed")
    synth.write_bed(bed, rows, [n for n, _ in synth.SMALL2])
    for cmd, run in (("depth", ob.depth_run), ("coverage", ob.coverage_run)):
        head = HEADS[cmd]
        want = str(tmp_path / ("want_%s.tsv" % cmd))
        rc, msg = run(gff, bed, want)
        assert rc == 0, msg
        want_rows = _table(open(want, "rb").read(), head)
        assert len(want_rows) > 10
        for chunk in (None, "5000"):
            env = dict(os.environ)
            if chunk:
                env["GFFX_SAM_CHUNK_BYTES"] = chunk
            out = str(tmp_path / ("got_%s.tsv" % cmd))
            r = subprocess.run([GFFX, cmd, "-v", "-i", gff, "-s", path, "-o", out], capture_output=True, env=env)
            assert r.returncode == 0, r.stderr
            assert b"SAM rows (device)" in r.stderr and b"SAM line scan (device)" in r.stderr and b"rows kept" in r.stderr
            assert b"%d rows kept" % len(rows) in r.stderr
            assert _table(open(out, "rb").read(), head) == want_rows, (cmd, chunk)
    if source != "plain":
        return
    out = str(tmp_path / "got2.tsv")
    r = subprocess.run([GFFX, "depth", "--gpus", "2", "-i", gff, "-s", path, "-o", out], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert _table(open(out, "rb").read(), HEADS["depth"]) == _table(open(str(tmp_path / "want_depth.tsv"), "rb").read(), HEADS["depth"])


def test_dispatch_by_content_and_extension(tmp_path, gff, big):
    recs, lines, rows, counts = big
    good = str(tmp_path / "good.sam")
    synth.write_sam(good, synth.sam_header(REFS), lines)
    ref = subprocess.run([GFFX, "depth", "-i", gff, "-s", good], capture_output=True)
    assert ref.returncode == 0 and ref.stdout.startswith(HEADS["depth"] + b"\n") and ref.stdout.count(b"\n") > 1, ref.stderr
    # an upper-case extension
    upper = str(tmp_path / "UPPER.SAM")
    synth.write_sam(upper, synth.sam_header(REFS), lines)
    r = subprocess.run([GFFX, "depth", "-i", gff, "-s", upper], capture_output=True)
    assert r.returncode == 0 and r.stdout == ref.stdout, r.stderr
    # a BAM file under a .sam name is read as BAM (records with a CIGAR: the same rows either way)
    with_cigar = [x for x in recs if x[4]]
    bam_as_sam, as_sam = str(tmp_path / "really_bam.sam"), str(tmp_path / "with_cigar.sam")
    synth.write_bam(bam_as_sam, synth.bam_header(REFS), [x[0] for x in with_cigar])
    synth.write_sam(as_sam, synth.sam_header(REFS), synth.sam_records_from(with_cigar, REFS))
    a = subprocess.run([GFFX, "depth", "-v", "-i", gff, "-s", bam_as_sam], capture_output=True)
    b = subprocess.run([GFFX, "depth", "-i", gff, "-s", as_sam], capture_output=True)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and b"BAM inflate (device)" in a.stderr, a.stderr
    # no @SQ line: a warning, no rows, the header-only table
    bare = str(tmp_path / "bare.sam")
    synth.write_sam(bare, b"@HD\tVN:1.6\n", lines)
    for cmd in ("depth", "coverage"):
        r = subprocess.run([GFFX, cmd, "-i", gff, "-s", bare], capture_output=True)
        assert r.returncode == 0 and r.stdout == HEADS[cmd] + b"\n", r.stderr
        assert sum(1 for ln in r.stderr.splitlines() if b"[WARN]" in ln and b"@SQ" in ln) == 1, r.stderr
    # an empty file, gzip that is not BGZF, a duplicate @SQ name
    import gzip
    bad = {"empty.sam": (b"", b"is empty"), "plain_gzip.sam": (gzip.compress(b"@HD\tVN:1.6\n"), b"not BGZF"),
           "dup.sam": (synth.sam_header(REFS + [("chr1", 5)]) + lines[0] + b"\n", b"duplicate")}
    for name, (blob, msg) in bad.items():
        p = tmp_path / name
        p.write_bytes(blob)
        r = subprocess.run([GFFX, "depth", "-i", gff, "-s", str(p)], capture_output=True)
        assert r.returncode == 1 and msg in r.stderr and r.stderr.rstrip().endswith(b"(read without htslib)"), (name, r.stderr)


MALFORMED = {
    "10 fields": (b"q\t0\tchr1\t5\t60\t10M\t*\t0\t0\tACGT", b"fewer than 11 fields"),
    "empty line": (b"", b"fewer than 11 fields"),
    "flag 0x10": (b"q\t0x10\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", b"FLAG"),
    "flag 016": (b"q\t016\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", b"FLAG"),
    "flag 70000": (b"q\t70000\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", b"FLAG"),
    "empty pos": (b"q\t0\tchr1\t\t60\t10M\t*\t0\t0\t*\t*", b"POS"),
    "19-digit pos": (b"q\t0\tchr1\t1234567890123456789\t60\t10M\t*\t0\t0\t*\t*", b"POS"),
    "cigar 10": (b"q\t0\tchr1\t5\t60\t10\t*\t0\t0\t*\t*", b"CIGAR"),
    "cigar M": (b"q\t0\tchr1\t5\t60\tM\t*\t0\t0\t*\t*", b"CIGAR"),
    "cigar 5Q": (b"q\t0\tchr1\t5\t60\t5Q\t*\t0\t0\t*\t*", b"CIGAR"),
    "cigar 268435456M": (b"q\t0\tchr1\t5\t60\t268435456M\t*\t0\t0\t*\t*", b"CIGAR"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_line_fails_and_names_its_line(tmp_path, gff, big, name):
    """On line 1 (a file without header), on a middle line, on the last line, and on a line that straddles a chunk boundary
    (4096-byte chunks); with a second malformed line further down, which must not be the one reported."""
    bad, reason = MALFORMED[name]
    lines = [ln for ln in big[1][:400] if len(ln) < 2000]
    header = synth.sam_header(REFS)
    n_head = header.count(b"\n")
    # `bad` begins `half` bytes before offset 8192, so it lies across the boundary of the second and third 4096-byte chunk (the
    # empty line: its newline is the third chunk's first byte); a good filler line of the right length ends just before it
    half = len(bad) // 2
    good_tail = b"\t0\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*"
    at_cut, size = 0, len(header)
    while size + len(lines[at_cut]) + 1 <= 8192 - half - len(good_tail) - 2:
        size += len(lines[at_cut]) + 1
        at_cut += 1
    filler = b"p" * (8192 - half - size - len(good_tail) - 1) + good_tail
    cases = [("line 1", b"", [bad] + lines, 1, None),
             ("middle", header, lines[:150] + [bad] + lines[150:], n_head + 151, None),
             ("last", header, lines + [bad], n_head + len(lines) + 1, None),
             ("straddling", header, lines[:at_cut] + [filler, bad] + lines[at_cut:] + [MALFORMED["cigar M"][0]], n_head + at_cut + 2, "4096")]
    for what, head, body, line_no, chunk in cases:
        path = str(tmp_path / "bad.sam")
        synth.write_sam(path, head, body)
        if what == "straddling":
            begin = len(head) + sum(len(x) + 1 for x in body[:at_cut + 1])
            assert begin == 8192 - half and begin + len(bad) >= 8192, (begin, len(bad))
        env = dict(os.environ)
        if chunk:
            env["GFFX_SAM_CHUNK_BYTES"] = chunk
        r = subprocess.run([GFFX, "depth", "-i", gff, "-s", path], capture_output=True, env=env, timeout=120)
        assert r.returncode == 1 and b"Error: " in r.stderr, (what, r.returncode, r.stderr)
        assert b"bad.sam\": line %d: " % line_no in r.stderr and reason in r.stderr, (what, r.stderr)
        assert r.stderr.rstrip().endswith(b"(read without htslib)"), (what, r.stderr)


def test_corrupt_bgzf_member_names_its_file_offset_and_a_valid_run_follows(tmp_path, gff, big):
    recs, lines, rows, counts = big
    path = str(tmp_path / "x.sam")
    synth.write_sam(path, synth.sam_header(REFS), lines, bgzf=True)
    data = open(path, "rb").read()
    off = engine.bgzf_members(data)
    bad = str(tmp_path / "bad_crc.sam")
    open(bad, "wb").write(data[:off[3] - 8] + bytes([data[off[3] - 8] ^ 0xFF]) + data[off[3] - 7:])
    r = subprocess.run([GFFX, "depth", "-i", gff, "-s", bad], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"offset %d" % off[2] in r.stderr and b"CRC32" in r.stderr, r.stderr
    assert r.stderr.rstrip().endswith(b"(read without htslib)")
    cut = str(tmp_path / "cut.sam")
    open(cut, "wb").write(data[:off[len(off) // 2] + 100])
    r = subprocess.run([GFFX, "depth", "-i", gff, "-s", cut], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"offset %d" % off[len(off) // 2] in r.stderr, r.stderr
    r = subprocess.run([GFFX, "depth", "-i", gff, "-s", path], capture_output=True)
    assert r.returncode == 0, r.stderr


def test_engine_reports_the_first_malformed_line_and_stays_failed(tmp_path, small):
    recs, lines, want, counts = small
    bad1, bad2 = MALFORMED["cigar 5Q"][0], MALFORMED["flag 016"][0]
    body = lines[:10] + [bad1] + lines[10:] + [bad2]
    data, hb = _text(tmp_path, body)
    n_head = synth.sam_header(REFS).count(b"\n")
    for chunk in (0, 300):
        r = engine.SamReader(NAMES, REF_SEQ, hb, chunk)
        with pytest.raises(engine._ffi.GffxHipError) as ei:
            r.feed(data)
            r.finish()
        assert ("line %d: CIGAR" % (n_head + 11)) in str(ei.value), str(ei.value)
        with pytest.raises(engine._ffi.GffxHipError) as again:  # sticky
            r.finish()
        assert ("line %d: CIGAR" % (n_head + 11)) in str(again.value)
        r.close()
    with pytest.raises(engine._ffi.GffxHipError) as ei:
        engine.SamReader(["chr1", "chr2", "chr1"], [0, 1, 0], 0)
    assert "duplicate" in str(ei.value)
