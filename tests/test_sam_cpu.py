"""The SAM text front end shared by the host and k_sam_rows (device/sam_core.hpp: header scan, the rules of one alignment
line, the names table), built for the host under AddressSanitizer + UndefinedBehaviorSanitizer (tools/sam_check.cpp): rows
equal to the Python restatement, the header's size on long, missing and cut headers, every malformed class rejected with its
reason and no sanitizer report, RNAME lookup on tables of 1, 2 and 5000 names.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from gffx_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "sam_check")
REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]
REF_SEQ = [0, 0xFFFFFFFF, 2]  # sam_check: the @SQ rank, UINT32_MAX for the names given as missing


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "sam_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def records():
    recs = synth.bam_test_records(3000, seed=5, refs=REFS, big=True)
    return recs, synth.sam_records_from(recs, REFS)


def _kept(stdout):
    """(header line, kept rows, tallies) of a `sam_check rows` run."""
    lines = stdout.splitlines()
    rows = [tuple(int(x) for x in ln.split()[1:4]) for ln in lines[1:] if ln.startswith("keep ")]
    tally = {k: sum(1 for ln in lines[1:] if ln.startswith("skip " + k + " ")) for k in ("unmapped", "noseq", "nointerval")}
    return lines[0], np.array(rows, dtype=np.uint32).reshape(-1, 3), tally, len(lines) - 1


def test_rows_equal_the_definition(tool, tmp_path, records):
    recs, lines = records
    want = synth.sam_rows_definition(recs, REF_SEQ)
    counts = synth.sam_counts_definition(recs, REF_SEQ)
    assert len(want) > 1000 and any(not r[4] and not r[3] & 4 for r in recs)  # a `*` CIGAR on a mapped read is among them
    header = synth.sam_header(REFS)
    outs = {}
    for name, kw in (("plain", {}), ("no_final_newline", {"final_newline": False}), ("crlf", {"newline": b"\r\n"})):
        path = tmp_path / (name + ".sam")
        hb = synth.write_sam(str(path), header, lines, **kw)
        r = _run(tool, "rows", path, "chrU")
        assert r.returncode == 0, r.stdout[-500:]
        head, got, tally, n = _kept(r.stdout)
        assert head == "header %d %d" % (hb, len(REFS)), name
        assert n == len(recs), name
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert tally["unmapped"] == counts["unmapped"] and tally["noseq"] == counts["no_seq"], name
        outs[name] = r.stdout.splitlines()[1:]
    assert outs["plain"] == outs["no_final_newline"] == outs["crlf"]


def test_header_size_on_a_long_header_no_header_and_every_cut(tool, tmp_path, records):
    _, lines = records
    long_text = b"".join(b"@CO\t" + bytes([65 + i % 26]) * 1000 + b"\n" for i in range(150))  # 150 KB of @CO lines
    header = synth.sam_header(REFS, long_text)
    assert len(header) > 150_000
    path = tmp_path / "long.sam"
    synth.write_sam(str(path), header, lines[:50])
    r = _run(tool, "rows", path)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "header %d %d" % (len(header), len(REFS))
    # no header at all: the first line is an alignment
    path = tmp_path / "bare.sam"
    synth.write_sam(str(path), b"", lines[:50])
    r = _run(tool, "rows", path)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "header 0 0" and len(r.stdout.splitlines()) == 51
    # a small header cut at every length: truncated (status 1), never a size; with the first byte of an alignment: its size
    small = synth.sam_header(REFS, b"@CO\tx\n@PG\tID:p\n")
    path = tmp_path / "cut.sam"
    path.write_bytes(small + lines[0][:1])
    out = [ln.split() for ln in _run(tool, "header", path).stdout.splitlines()]
    assert len(out) == len(small) + 2
    for length, st, hb in out[:-1]:
        assert (int(st), int(hb)) == (1, 0), length
    assert out[-1] == [str(len(small) + 1), "0", str(len(small))]


MALFORMED = {
    "10 fields": (b"q\t0\tchr1\t5\t60\t10M\t*\t0\t0\tACGT", "fewer than 11 fields"),
    "empty line": (b"", "fewer than 11 fields"),
    "flag 0x10": (b"q\t0x10\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", "FLAG"),
    "flag 016": (b"q\t016\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", "FLAG"),
    "flag 70000": (b"q\t70000\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", "FLAG"),
    "empty pos": (b"q\t0\tchr1\t\t60\t10M\t*\t0\t0\t*\t*", "POS"),
    "19-digit pos": (b"q\t0\tchr1\t1234567890123456789\t60\t10M\t*\t0\t0\t*\t*", "POS"),
    "cigar 10": (b"q\t0\tchr1\t5\t60\t10\t*\t0\t0\t*\t*", "CIGAR"),
    "cigar M": (b"q\t0\tchr1\t5\t60\tM\t*\t0\t0\t*\t*", "CIGAR"),
    "cigar 5Q": (b"q\t0\tchr1\t5\t60\t5Q\t*\t0\t0\t*\t*", "CIGAR"),
    "cigar 268435456M": (b"q\t0\tchr1\t5\t60\t268435456M\t*\t0\t0\t*\t*", "CIGAR"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_every_malformed_class_yields_its_status(tool, tmp_path, records, name):
    _, lines = records
    bad, reason = MALFORMED[name]
    header = synth.sam_header(REFS)
    n_head = header.count(b"\n")
    for at in (0, 7, 20):  # first, a middle and the last line (the last one without a newline too)
        for final_newline in (True, False):
            body = lines[:20]
            body = body[:at] + [bad] + body[at:]
            if not final_newline and not body[-1]:
                continue  # (an empty rest after the last newline is no line)
            path = tmp_path / "bad.sam"
            synth.write_sam(str(path), header, body, final_newline=final_newline)
            r = _run(tool, "rows", path)
            assert r.returncode == 3, (name, at, r.stdout[-300:])
            last = r.stdout.splitlines()[-1]
            assert last.startswith("malformed %d " % (n_head + at + 1)) and reason in last, (name, at, last)
    # its neighbours at the limit are read: 18 digits, 2^28 - 1, flag 65535 (unmapped among its bits), a lone 0
    ok = [b"q\t65535\tchr1\t5\t60\t10M\t*\t0\t0\t*\t*", b"q\t0\tchr1\t123456789012345678\t60\t10M\t*\t0\t0\t*\t*",
          b"q\t0\tchr1\t5\t60\t268435455M\t*\t0\t0\t*\t*", b"q\t0\tchr1\t0\t60\t10M\t*\t0\t0\t*\t*", b"q\t0\tchr1\t5\t60\t3B7M\t*\t0\t0\t*\t*"]
    path = tmp_path / "ok.sam"
    synth.write_sam(str(path), header, ok)
    r = _run(tool, "rows", path)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[1:] == ["skip unmapped 65535", "keep 0 4294967295 4294967295 0", "keep 0 4 268435459 0",
                                         "skip nointerval 0", "keep 0 4 11 0"]


def _fnv1a(name: bytes) -> int:
    h = 2166136261
    for b in name:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


@pytest.mark.parametrize("n", [1, 2, 5000])
def test_rname_lookup(tool, tmp_path, n):
    """Names that are prefixes of each other (chr1, chr10, chr100 ...), names that share a bucket of the table, names the
    table does not have -- among them ones that hash into an occupied bucket."""
    names = [b"chr%d" % (i + 1) for i in range(n)]
    slots = 2
    while slots < 2 * n:
        slots *= 2
    buckets = {}
    for nm in names:
        buckets.setdefault(_fnv1a(nm) & (slots - 1), []).append(nm)
    if n == 5000:
        assert any(len(v) > 1 for v in buckets.values())  # (some names do share a bucket)
    absent = [b"chr0", b"chr", b"chr1x", b"", b"*", b"CHR1"] + [b"scaffold%d" % i for i in range(300)]
    if n == 5000:
        assert any(_fnv1a(a) & (slots - 1) in buckets for a in absent)
    queries = names + absent + names[::-1]
    want = list(range(n)) + [-1] * len(absent) + list(range(n))[::-1]
    (tmp_path / "names.txt").write_bytes(b"\n".join(names) + b"\n")
    (tmp_path / "queries.txt").write_bytes(b"\n".join(queries) + b"\n")
    r = _run(tool, "lookup", tmp_path / "names.txt", tmp_path / "queries.txt")
    assert r.returncode == 0, r.stdout[-300:]
    out = r.stdout.splitlines()
    assert out[0] == "slots %d" % slots
    # (the empty query line in the middle is a line of its own for the tool as well)
    assert [int(x) for x in out[1:]] == want


def test_duplicate_reference_name_is_refused(tool, tmp_path):
    (tmp_path / "names.txt").write_bytes(b"chr1\nchr2\nchr1\n")
    (tmp_path / "queries.txt").write_bytes(b"chr1\n")
    r = _run(tool, "lookup", tmp_path / "names.txt", tmp_path / "queries.txt")
    assert r.returncode == 3 and r.stdout.strip() == "duplicate 2"


MINIMAL = b"\t0\t\t1\t\t1M\t\t\t\t\t"  # ten TABs, FLAG 0, the empty RNAME (an @SQ line may have the empty name), POS 1, CIGAR 1M


def test_the_shortest_kept_line_and_the_bound_that_sizes_the_rows_buffer(tool, tmp_path):
    """k_sam_rows' output buffer holds max_kept_lines(text bytes) rows, so no text may keep more lines than that.  A kept line
    needs ten TABs, a digit of FLAG, a digit of POS and a digit and an op of CIGAR: 14 bytes, and MINIMAL is such a line.  The
    bound is exact on a text of nothing but such lines (the last one without its newline) and nothing shorter is kept."""
    n = 70
    path = tmp_path / "min.sam"
    hb = synth.write_sam(str(path), b"@SQ\tSN:\tLN:9\n", [MINIMAL] * n, final_newline=False)
    r = _run(tool, "rows", path)
    assert r.returncode == 0 and r.stdout.splitlines() == ["header %d 1" % hb] + ["keep 0 0 1 0"] * n, r.stdout[-300:]
    sizes = [k * (len(MINIMAL) + 1) - 1 for k in range(1, n + 1)]
    out = _run(tool, "bound", 0, 13, *sizes, *[x - 1 for x in sizes]).stdout.split()
    assert int(out[0]) == len(MINIMAL) == 14
    bound = dict(zip(map(int, out[1::2]), map(int, out[2::2])))
    assert bound[0] == 0 and bound[13] == 0
    for k, size in enumerate(sizes, 1):
        assert bound[size] == k and bound[size - 1] == k - 1, (k, size)
    # the line of a reference with a one-letter name is kept as well; MINIMAL less any one byte is not
    synth.write_sam(str(path), b"@SQ\tSN:c\tLN:9\n", [b"\t0\tc\t1\t\t1M\t\t\t\t\t"])
    assert _run(tool, "rows", path).stdout.splitlines()[1:] == ["keep 0 0 1 0"]
    for i in range(len(MINIMAL)):
        synth.write_sam(str(path), b"@SQ\tSN:\tLN:9\n", [MINIMAL[:i] + MINIMAL[i + 1:]])
        r = _run(tool, "rows", path)
        assert r.returncode == 3 and "keep" not in r.stdout, (i, r.stdout)


def test_cli_refusals_that_need_no_device(tmp_path):
    """What `gffx depth -s x.sam` decides on the host, before any device is asked for: an empty file, gzip that is not BGZF, a
    duplicate @SQ name, a missing file -- each with a message that ends in "(read without htslib)"; CRAM keeps its refusal."""
    import gzip
    gffx = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, synth.gencode_like_roots(50, seed=1, chroms=synth.SMALL2), seed=1)
    assert subprocess.run([gffx, "index", "-i", gff], capture_output=True).returncode == 0
    line = synth.sam_line("chr1", 10, 0, [(0, 5)], b"q")
    cases = {"empty.sam": (b"", b"is empty"), "plain_gzip.sam": (gzip.compress(b"@HD\tVN:1.6\n"), b"not BGZF"),
             "dup.SAM": (synth.sam_header(REFS + [("chr1", 5)]) + line + b"\n", b"duplicate @SQ SN:chr1"), "missing.sam": (None, b"cannot open")}
    for name, (blob, msg) in cases.items():
        p = tmp_path / name
        if blob is not None:
            p.write_bytes(blob)
        for cmd in ("depth", "coverage"):
            r = subprocess.run([gffx, cmd, "-i", gff, "-s", str(p)], capture_output=True)
            assert r.returncode == 1 and msg in r.stderr and r.stderr.rstrip().endswith(b"(read without htslib)"), (name, r.stderr)
    (tmp_path / "r.cram").write_bytes(b"x")
    r = subprocess.run([gffx, "depth", "-i", gff, "-s", str(tmp_path / "r.cram")], capture_output=True)
    assert r.returncode == 1 and b"SAM/CRAM sources need htslib" in r.stderr
