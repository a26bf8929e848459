"""The streaming pipeline the BAM and the SAM reader share (device/source_stream.hpp), pinned for both readers on streams of
about a hundred records in members of a few hundred bytes: a failure stays a failure with its first message, rows are
refused while a sub-batch is in flight (or text is pending) and handed out after finish(), and a pinned staging buffer that
has to grow between two feeds of one handle still carries the right bytes."""
import numpy as np
import pytest

from gffx_amd import engine, synth

pytestmark = pytest.mark.gpu

REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]
NAMES = [n for n, _ in REFS]
REF_SEQ = [0, 0xFFFFFFFF, 1]  # chrU is not in the index
BLOCK = 512  # uncompressed bytes per member
Error = engine._ffi.GffxHipError


@pytest.fixture(scope="module")
def recs():
    return synth.bam_test_records(100, seed=7, refs=REFS, big=False)


def _members(payloads):
    return [synth.bgzf_member(p) for p in payloads]


def _bam_members(records, layout="aligned"):
    """The members of a BAM stream of `records` (bytes each) and the header's size."""
    header = synth.bam_header(REFS)
    return _members(synth.bgzf_blocks(header, records, layout, True, BLOCK)), len(header)


def _sam_members(lines, layout="aligned"):
    header = synth.sam_header(REFS)
    return _members(synth.bgzf_blocks(header, [ln + b"\n" for ln in lines], layout, True, BLOCK)), len(header)


def _bam_counts(recs):
    unmapped = sum(1 for r in recs if r[3] & 4)
    no_seq = sum(1 for r in recs if not r[3] & 4 and (r[1] < 0 or REF_SEQ[r[1]] == 0xFFFFFFFF))
    return {"records": len(recs), "unmapped": unmapped, "no_seq": no_seq, "kept": len(synth.bam_rows_definition(recs, REF_SEQ))}


def _reader(kind, hb, chunk_bytes):
    if kind == "bam":
        return engine.BamReader(REF_SEQ, hb, chunk_bytes)
    return engine.SamReader(NAMES, REF_SEQ, hb, chunk_bytes, bgzf=True)


@pytest.mark.parametrize("chunk", [0, 1])
@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_a_failed_reader_stays_failed_with_its_first_message(recs, kind, chunk):
    """40 records with a malformed one in the middle (BAM: l_read_name 0; SAM: a CIGAR operation that does not exist), in one
    sub-batch (chunk 0: found at finish) and one member per sub-batch (chunk 1: found inside feed)."""
    good = recs[:40]
    if kind == "bam":
        bad = bytearray(synth.bam_record(0, 500, 0, [(0, 100)], b"bad", 100))
        bad[12] = 0
        body = [r[0] for r in good[:20]] + [bytes(bad)] + [r[0] for r in good[20:]]
        members, hb = _bam_members(body)
        want = "malformed BAM record"
    else:
        lines = synth.sam_records_from(good, REFS)
        body = lines[:20] + [b"q\t0\tchr1\t5\t60\t5Q\t*\t0\t0\t*\t*"] + lines[20:]
        members, hb = _sam_members(body)
        want = "line %d: CIGAR" % (synth.sam_header(REFS).count(b"\n") + 21)
    assert len(members) >= 3
    r = _reader(kind, hb, chunk)
    with pytest.raises(Error) as first:
        r.feed(b"".join(members))
        r.finish()
    assert want in str(first.value), str(first.value)
    with pytest.raises(Error) as again:
        r.finish()
    assert str(again.value) == str(first.value)
    with pytest.raises(Error) as fed:
        r.feed(b"")
    assert str(fed.value) == str(first.value)
    r.close()


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_rows_are_refused_before_finish_and_handed_out_after(recs, kind):
    """A 3-member stream (the header, then two members of six records): fed, its one sub-batch is in flight."""
    some = recs[:12]
    if kind == "bam":
        header, body = synth.bam_header(REFS), [r[0] for r in some]
        want = synth.bam_rows_definition(some, REF_SEQ)
    else:
        header, body = synth.sam_header(REFS), [ln + b"\n" for ln in synth.sam_records_from(some, REFS)]
        want = synth.sam_rows_definition(some, REF_SEQ)
    members = _members([header, b"".join(body[:6]), b"".join(body[6:])])
    r = _reader(kind, len(header), 0)
    r.feed(b"".join(members))
    with pytest.raises(Error) as ei:
        r.rows()
    assert "finish first" in str(ei.value)
    r.finish()  # (the refusal is not sticky)
    got = r.rows()
    r.close()
    assert len(want) > 0 and got.shape == want.shape and np.array_equal(got, want)


def test_rows_of_plain_sam_are_refused_while_text_is_pending(recs):
    """Fewer bytes than a chunk: nothing is in flight, the pending text alone refuses."""
    some = recs[:12]
    header = synth.sam_header(REFS)
    text = header + b"".join(ln + b"\n" for ln in synth.sam_records_from(some, REFS))
    want = synth.sam_rows_definition(some, REF_SEQ)
    r = engine.SamReader(NAMES, REF_SEQ, len(header), 0)
    r.feed(text)
    with pytest.raises(Error) as ei:
        r.rows()
    assert "finish first" in str(ei.value)
    r.finish()
    got = r.rows()
    r.close()
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("single", [1, 2])
@pytest.mark.parametrize("kind,layout", [("bam", "aligned"), ("bam", "spanning"), ("sam", "aligned")])
def test_staging_that_grows_between_feeds(recs, kind, layout, single):
    """One handle, default chunk size: `single` feeds of one member each, then all the remaining members in one call, a
    sub-batch that needs a far larger pinned buffer than those before it (single 2: the very buffer the first feed sized)."""
    if kind == "bam":
        members, hb = _bam_members([r[0] for r in recs], layout)
        want, counts = synth.bam_rows_definition(recs, REF_SEQ), _bam_counts(recs)
    else:
        members, hb = _sam_members(synth.sam_records_from(recs, REFS), layout)
        want, counts = synth.sam_rows_definition(recs, REF_SEQ), synth.sam_counts_definition(recs, REF_SEQ)
    assert len(members) - single >= 20 and max(len(m) for m in members) < 1024
    r = _reader(kind, hb, 0)
    for m in members[:single]:
        r.feed(m)
    r.feed(b"".join(members[single:]))
    r.finish()
    got, c = r.rows(), r.counts()
    r.close()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert c == counts, (c, counts)
