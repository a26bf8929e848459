"""BED sources on the GPU (device/bed.hip through engine.bed_rows): rows, tallies and errors equal the Python restatement
(tests/_bed_oracle.py) in both dialects, on plain and BGZF-compressed text, at the shapes where the kernels can go wrong --
line ends around the 1024-byte step and the 4096-byte tile of the line kernels, 63 to 129 lines in one tile of the rows
kernel, chunk and feed boundaries inside a name, inside a number, between CR and LF and right after LF, member boundaries
inside a line -- and no larger.  The failure cases are error returns of well-formed launches."""
import numpy as np
import pytest

import _bed_cases as cases
import _bed_oracle as bo
from gffx_amd import _ffi, engine, synth

pytestmark = pytest.mark.gpu

DIALECTS = [bo.INTERSECT, bo.DEPTH]
NAMES = cases.NAMES


def _bgzf(payloads, eof=True):
    return b"".join(synth.bgzf_member(p) for p in payloads) + (synth.BGZF_EOF if eof else b"")


def _cut(text, n):
    return [text[i:i + n] for i in range(0, len(text), n)]


def _check(text, dialect, names=NAMES, data=None, **kw):
    """engine.bed_rows on `data` (default: the text itself) against the oracle on `text`: rows and tallies, or the error."""
    want, counts, err, _ = bo.run(text, dialect, names)
    if err is not None:
        with pytest.raises(_ffi.GffxHipError) as ei:
            engine.bed_rows(text if data is None else data, names, dialect, **kw)
        assert ei.value.code == -1 and str(ei.value) == "gffx_hip error -1: " + err, kw
        return
    c = {}
    got = engine.bed_rows(text if data is None else data, names, dialect, counts=c, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), kw
    assert c == counts and c["lines"] == c["skipped"] + c["no_seq"] + c["kept"], (kw, c, counts)


ROWS = b"chr1\t5\t9\nchr10\t7\t7\n#c\nchrX\t1\t2"  # (kept, a start == end row, a comment, a last line without newline)


@pytest.mark.parametrize("dialect", DIALECTS)
@pytest.mark.parametrize("at", [1023, 1024, 1025, 4095, 4096, 4097])
def test_a_line_end_at_the_step_and_tile_edges(dialect, at):
    """The newline of the first line is byte `at` of the text: the last lane's last byte of a 1024-byte step, the first of the
    next, and the same at the tile's edge."""
    head = b"chr1\t1\t2\t"
    text = head + b"x" * (at - len(head)) + b"\n" + ROWS
    assert text[at:at + 1] == b"\n" and text.index(b"\n") == at
    _check(text, dialect)
    _check(b"chrX\t3\t4\n" + text[10:], dialect)  # the same with a line end in front of it


@pytest.mark.parametrize("dialect", DIALECTS)
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_lane_groups_of_the_rows_kernel(dialect, n):
    """n lines end in one tile: one lane group short of a lane, full, one over, and two groups and one; every fifth line is
    skipped, so the compaction's ballot has holes."""
    lines = [b"#skip" if i % 5 == 3 else b"chr10\t%d\t%d" % (i, i + 2) for i in range(n)]
    text = b"".join(ln + b"\n" for ln in lines)
    assert len(text) < 4096 and text.count(b"\n") == n
    _check(text, dialect)
    _check(text[:-1], dialect)  # ... the last of them without its newline


@pytest.mark.parametrize("dialect", DIALECTS)
def test_a_tile_without_a_line_end_then_a_tile_that_begins_with_one(dialect):
    first = b"chr1\t1\t2\t" + b"y" * (4096 - 9)
    assert len(first) == 4096
    _check(first + b"\n" + ROWS, dialect)  # tile 0 has no newline, tile 1 begins with it
    lead = b"chrX\t8\t9\n"
    mid = b"chr1\t3\t4\t" + b"y" * (8192 - len(lead) - 9)
    text = lead + mid + b"\n" + ROWS
    assert text[8192:8193] == b"\n" and b"\n" not in text[4096:8192]
    _check(text, dialect)  # a line end in tile 0, none in tile 1, tile 2 begins with one


def _placed_text():
    """CRLF lines, laid out so that byte 4096 falls inside a name, 8192 inside a number, 12288 between CR and LF and 16384
    right after LF.  Returns the text and a label per byte: N name, D digit, other bytes themselves."""
    rng = np.random.Generator(np.random.PCG64(3))
    out, label = bytearray(), bytearray()

    def add(name, s, e, tail=b""):
        a, b = b"%d" % s, b"%d" % e
        out.extend(name + b"\t" + a + b"\t" + b + tail + b"\r\n")
        label.extend(b"N" * len(name) + b"\t" + b"D" * len(a) + b"\t" + b"D" * len(b) + tail + b"\r\n")

    def row():
        s = int(rng.integers(100000, 900000))
        add(NAMES[int(rng.integers(0, 3))], s, s + int(rng.integers(1, 5000)), (b"", b"\tn\t0")[int(rng.integers(0, 2))])

    for k, lead in ((1, 2), (2, 7), (3, 20), (4, 0)):  # the line that starts `lead` bytes before 4096 * k
        edge = 4096 * k
        while edge - lead - len(out) > 100:
            row()
        fill = edge - lead - len(out) - 3
        out.extend(b"#" + b"f" * fill + b"\r\n")
        label.extend(b"#" + b"f" * fill + b"\r\n")
        assert len(out) == edge - lead
        add(b"chr10", 123456, 234567, b"")  # 21 bytes with CR LF: byte 19 is the CR, byte 20 the LF
    for _ in range(40):
        row()
    return bytes(out), bytes(label)


def _placements(label, step):
    seen = set()
    for b in range(step, len(label), step):
        p, q = label[b - 1:b], label[b:b + 1]
        if p == q == b"N":
            seen.add("name")
        if p == q == b"D":
            seen.add("number")
        if p == b"\r" and q == b"\n":
            seen.add("crlf")
        if p == b"\n":
            seen.add("after")
    return seen


@pytest.mark.parametrize("dialect", DIALECTS)
@pytest.mark.parametrize("feed", [1, 7, 4096])
@pytest.mark.parametrize("chunk", [64, 100, 4096])
def test_chunk_and_feed_boundaries_anywhere(dialect, chunk, feed):
    text, label = _placed_text()
    assert len(text) == len(label) and len(text) > 4 * 4096
    for step in (chunk, feed):  # each placement occurs among the sub-batch boundaries and among the feed boundaries
        assert _placements(label, step) == {"name", "number", "crlf", "after"}, step
    _check(text, dialect, chunk_bytes=chunk, feed_bytes=feed)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_small_files(dialect):
    for text in (b"", b"\n", b"#a\n#b\n# c", b"#a\n", b"chr1\t1\t2", b"chr1\t1\t2\n\n", b"chr1\t1", b"\n\nchrX\t0\t1"):
        for kw in ({}, {"chunk_bytes": 1}, {"chunk_bytes": 5, "feed_bytes": 2}):
            _check(text, dialect, **kw)
        _check(text, dialect, data=_bgzf([text] if text else []), bgzf=True)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_bgzf_member_shapes(dialect):
    lines = [ln for ln, want in cases.expected(dialect) if want[0] != "error"]
    text = b"".join(ln + b"\n" for ln in lines)
    shapes = {
        "boundary inside a line": _cut(text, 37),
        "one line per member": [ln + b"\n" for ln in lines],
        "an empty member in the middle": _cut(text, 500)[:3] + [b""] + _cut(text, 500)[3:],
        "one member": [text] if len(text) < 60000 else _cut(text, 60000),
    }
    for tag, payloads in shapes.items():
        assert b"".join(payloads) == text
        for kw in ({}, {"chunk_bytes": 1}, {"feed_bytes": 1}):  # all at once; a member per sub-batch; a member per feed call
            _check(text, dialect, data=_bgzf(payloads), bgzf=True, **kw)
    _check(b"", dialect, data=synth.BGZF_EOF, bgzf=True)  # the EOF member only
    _check(text, dialect, data=_bgzf(_cut(text, 37), eof=False), bgzf=True)
    few = b"".join(b"chr10\t%d\t%d\n" % (i, i + 3) for i in range(180))[:2100]  # (the last line cut short, without newline)
    members = _cut(few, 7)
    assert len(members) == 300
    _check(few, dialect, data=_bgzf(members), bgzf=True)
    _check(few, dialect, data=_bgzf(members), bgzf=True, chunk_bytes=100)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_a_mib_line_then_a_good_row(dialect):
    text = b"chr1\t1\t2\t" + b"z" * (1 << 20) + b"\nchrX\t5\t6\n"
    _check(text, dialect)
    _check(text, dialect, chunk_bytes=65536, feed_bytes=50000)
    _check(text, dialect, data=_bgzf(_cut(text, 65000)), bgzf=True, chunk_bytes=1 << 16)
    _check(b"chr1\t1\t2\t" + b"z" * (1 << 20) + b"\xe2\x82\nchrX\t5\t6\n", dialect)  # ... invalid at its very end


def test_the_first_error_in_file_order_is_reported():
    good = b"".join(b"chr1\t%d\t%d\n" % (i, i + 1) for i in range(40))
    bad_c, bad_c2, bad_u = b"chr1\tx\t5\n", b"chr1\t5\t-7\n", b"chr1\t1\t2\t\xff\n"
    # two bad lines in one sub-batch, 70 lines (two lane groups) and several tiles apart: the first is the one reported
    far = b"".join(b"chr1\t1\t2\t" + b"p" * 200 + b"\n" for _ in range(70))
    for text in (good + bad_c + far + bad_c2 + good, good + bad_c2 + far + bad_c, good + bad_c + bad_c2, good + bad_u + far + bad_c):
        _check(text, bo.INTERSECT)
        _check(text, bo.INTERSECT, data=_bgzf(_cut(text, 1000)), bgzf=True)
    # a bad line in the third sub-batch after two good ones; one in each of the three: the first
    assert len(good) > 300
    for text in (good[:200] + bad_c + good, bad_c2 + good[:200] + bad_c + good):
        _check(text, bo.INTERSECT, chunk_bytes=100)
        _check(text, bo.INTERSECT, chunk_bytes=100, feed_bytes=7)
    # a UTF-8 error and a coordinate error on neighbouring lines, in either order
    for text in (good + bad_u + bad_c + good, good + bad_c + bad_u + good, bad_u + bad_c, bad_c + bad_u):
        for kw in ({}, {"chunk_bytes": 64}):
            _check(text, bo.INTERSECT, **kw)
    # the depth dialect calls none of these an error
    _check(good + bad_u + bad_c + bad_c2 + good, bo.DEPTH)


def test_an_error_is_sticky_and_the_rows_are_refused():
    text = b"chr1\t1\t2\n" * 30 + b"chr1\t+\t5\tname\n" + b"chr1\t3\t4\n" * 30
    want = 'gffx_hip error -1: lexical parse error: invalid BED coordinate in "chr1\t+\t5\tname"'
    r = engine.BedReader(NAMES, bo.INTERSECT, chunk_bytes=128)
    try:
        with pytest.raises(_ffi.GffxHipError) as ei:
            r.feed(text)
        assert str(ei.value) == want
        for call in (lambda: r.feed(b"chr1\t1\t2\n"), r.finish, r.rows, lambda: r.feed(b""), r.finish):
            with pytest.raises(_ffi.GffxHipError) as ei:
                call()
            assert ei.value.code == -1 and str(ei.value) == want
    finally:
        r.close()
    # a long line is quoted whole, the first time and every later time
    long_line = b"chr1\tx\t5\t" + b"q" * 5000
    r = engine.BedReader(NAMES, bo.INTERSECT)
    try:
        r.feed(long_line + b"\n")
        for call in (r.finish, r.finish, r.rows):
            with pytest.raises(_ffi.GffxHipError) as ei:
                call()
            assert str(ei.value) == 'gffx_hip error -1: lexical parse error: invalid BED coordinate in "%s"' % long_line.decode()
    finally:
        r.close()


@pytest.fixture(scope="module")
def generated():
    out = {}
    for dialect in DIALECTS:
        lines = bo.generate(20000, 11, dialect)
        bo.check_generated(lines, dialect)
        out[dialect] = b"".join(ln + b"\n" for ln in lines)
    return out


@pytest.mark.parametrize("dialect", DIALECTS)
@pytest.mark.parametrize("form", ["plain", "plain chunks", "bgzf", "bgzf chunks"])
def test_generated_lines_equal_the_oracle(generated, dialect, form):
    text = generated[dialect]
    if form == "plain":
        _check(text, dialect, names=bo.GEN_NAMES)
    elif form == "plain chunks":
        _check(text, dialect, names=bo.GEN_NAMES, chunk_bytes=10007, feed_bytes=4099)
    else:
        data = _bgzf(_cut(text, 0xFF00))
        _check(text, dialect, names=bo.GEN_NAMES, data=data, bgzf=True, chunk_bytes=0 if form == "bgzf" else 20000)
    # ... and the error-bearing set ends at the oracle's first error
    if dialect == bo.INTERSECT and form in ("plain", "bgzf"):
        bad = b"".join(ln + b"\n" for ln in bo.generate(2000, 12, bo.INTERSECT, errors=True))
        _check(bad, dialect, names=bo.GEN_NAMES, data=_bgzf(_cut(bad, 3000)) if form == "bgzf" else None, bgzf=form == "bgzf")
