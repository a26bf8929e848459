"""The device side of `gffx seq` against the definition (tests/_seq_definition.py), bit for bit.  The genome object: feeds cut at
every byte position, chunk edges inside headers and CR LF pairs, line counts at the line kernels' tile and wave edges, ragged
lines, an empty sequence, 300 sequences, the three FASTA errors with their lines.  The plan and the emit: record lengths around
the line width and the output tile, tile edges on and behind a newline, one-base segments, codons across two and three
segments, every phase with 0 .. 3 bases left, minus twins of all of them, segments at a sequence's first and last base, a member
one base beyond the end, 1 / 63 / 64 / 65 records, one record of 5000 segments, duplicate and overlapping segments, a lower-case
IUPAC genome, and slices of 1, 7 and SEQ_TILE + 1 bytes against one slice."""
import random

import numpy as np
import pytest

import _seq_definition as sd
from gffx_amd import _ffi, engine

pytestmark = pytest.mark.gpu


# ---- the genome object ----------------------------------------------------------------------------------------------------

def _check_genome(g, text):
    names, seqs = sd.parse_fasta(text)
    assert g.names == names and g.lengths.tolist() == [len(s) for s in seqs]
    assert g.offsets.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).tolist()
    assert g.bases() == b"".join(seqs)


SMALL = b">chrA x\r\nACGTACGTAC\r\n\r\nGTTTGACCAT\n>b\n\n>chrB\tdesc\nttgcaN\r\n>c\nA\nC\n>GT\r"


def test_feeds_cut_at_every_byte_position():
    for cut in range(len(SMALL) + 1):
        g = engine.Genome()
        g.feed(SMALL[:cut])
        g.feed(SMALL[cut:])
        g.finish()
        _check_genome(g, SMALL)
        g.close()


@pytest.mark.parametrize("piece,chunk", [(1, 0), (2, 0), (3, 0), (5, 0), (0, 1), (0, 2), (0, 7), (1000, 16), (0, 0)])
def test_pieces_and_chunk_edges_inside_headers_and_crlf_pairs(piece, chunk):
    for text in (SMALL, sd.HAND_FASTA, b">a\nAC\n>bb long header here\r\nGG", b"\n\n>a\n", b""):
        g = engine.genome_from_fasta(text, feed_bytes=piece, chunk_bytes=chunk)
        _check_genome(g, text)
        g.close()


@pytest.mark.parametrize("width", [1, 3, 15, 16, 63])
def test_line_counts_at_the_tile_and_wave_edges(width):
    # lines of `width` bases: the line ends fall on every phase of the 16-byte loads, the 1024-byte steps and the 4 KiB tiles
    rng = random.Random(width)
    for n_lines in (63, 64, 65, 4096 // (width + 1) - 1, 4096 // (width + 1), 4096 // (width + 1) + 1, 2 * 4096 // (width + 1) + 1):
        body = b"".join(bytes(rng.choice(b"ACGT") for _ in range(width)) + b"\n" for _ in range(n_lines))
        for head in (b">s\n", b">s" + b"x" * 13 + b"\n"):
            text = head + body
            g = engine.genome_from_fasta(text)
            _check_genome(g, text)
            g.close()


def test_ragged_lines_an_empty_sequence_and_300_sequences():
    rng = random.Random(5)
    parts = []
    for i in range(300):
        parts.append(b">s%d d\n" % i)
        if i % 7 == 3:
            continue  # an empty sequence
        for _ in range(rng.randrange(1, 9)):
            parts.append(bytes(rng.choice(b"ACGTNacgtn") for _ in range(rng.choice((1, 1, 2, 5, 17, 60, 61, 200)))) + rng.choice((b"\n", b"\r\n", b"\n\n")))
    text = b"".join(parts)
    for piece, chunk in ((0, 0), (4097, 0), (0, 1000), (0, 4096), (0, 4097)):
        g = engine.genome_from_fasta(text, feed_bytes=piece, chunk_bytes=chunk)
        _check_genome(g, text)
        assert g.stage_ms()["pack_ms"] > 0
        g.close()
    text, _ = sd.random_genome(9, names=("a", "b", "c"), lengths=(70001, 1, 33333))
    g = engine.genome_from_fasta(text, chunk_bytes=30011)
    _check_genome(g, text)
    g.close()


@pytest.mark.parametrize("text,line,what", [(b"ACGT\n>a\nAC\n", 1, b"before the first"), (b"\n\r\n \n>a\n", 3, b"before the first"),
                                            (b">a\nAC\n>\nAC\n", 3, b"without a sequence name"), (b">a\n>\r\n", 2, b"without a sequence name"),
                                            (b">a\n>b\n\n>a desc\n", 4, b"given twice"), (b">a\nAC\n" * 2, 3, b"given twice")])
def test_the_fasta_errors_name_the_line_and_stick(text, line, what):
    for piece in (0, 1, 4):
        g = engine.Genome()
        with pytest.raises(_ffi.GffxHipError) as ei:
            for i in range(0, len(text), piece or len(text)):
                g.feed(text[i:i + (piece or len(text))])
            g.finish()
        msg = str(ei.value).encode()
        assert ei.value.code == -1 and b"line %d:" % line in msg and what in msg, msg
        with pytest.raises(_ffi.GffxHipError) as again:  # sticky
            g.finish()
        assert b"failed earlier" in str(again.value).encode()
        g.close()


# ---- the plan and the emit ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def genome():
    text, seqs = sd.random_genome(3, names=("s0", "s1", "s2"), lengths=(30000, 997, 64), alphabet=b"ACGTacgtNnRYKMBVDHSWUu")
    g = engine.genome_from_fasta(text)
    yield g, seqs
    g.close()


def _check(genome, rows, flags, translated, w, slices=()):
    g, seqs = genome
    want, off, dropped = sd.bodies(seqs, rows, flags, translated, w)
    p = engine.SeqPlan(g, np.array(rows, np.uint32).reshape(-1, 4), np.array(flags, np.uint8), translated, w)
    assert p.body_off.tolist() == off and p.dropped.tolist() == dropped and p.body_bytes == len(want)
    assert p.emit() == want
    for s in slices:
        assert p.emit_sliced(s) == want, s
    p.close()
    return want


def _with_minus_twins(rows, flags):
    """every record once more on minus, behind the plus ones"""
    n = len(flags)
    return rows + [(r + n, q, s, e) for r, q, s, e in rows], flags + [f | 1 for f in flags]


def test_record_lengths_around_the_width_and_the_tile(genome):
    tile = engine.SEQ_TILE
    for w in (60, 7, 0):
        lens = sorted({1, 2, max(w, 2) - 1, max(w, 2), w + 1, 2 * w + 1, tile - 1, tile, tile + 1, 2 * tile + 1})
        rows, flags = [], []
        for k, n in enumerate(lens):
            rows.append((k, 0, 10 + k, 10 + k + n))
            flags.append(0)
        rows, flags = _with_minus_twins(rows, flags)
        _check(genome, rows, flags, False, w, slices=(tile + 1,))


def test_a_tile_edge_on_a_newline_and_right_after_one(genome):
    tile, w = engine.SEQ_TILE, 60
    # a first record whose body ends d bytes before the tile edge, then a long one: its newlines shift over the edge
    ends = {tile - d for d in range(4)}
    for n in range(tile - 80, tile):
        if sd.body_bytes(n, w) in ends:
            rows = [(0, 0, 5, 5 + n), (1, 0, 100, 100 + 3 * tile), (2, 0, 7, 7 + 61)]
            _check(genome, rows, [0, 1, 0], False, w, slices=(tile, 61))
    for n in (tile - tile // 61 - 1, tile - tile // 61, tile - tile // 61 + 1, 60 * 67, 60 * 67 + 1):  # one record across the edge
        _check(genome, [(0, 0, 0, n), (1, 0, 3, 3 + n)], [0, 1], False, w)


def test_one_base_segments_and_codons_across_segments(genome):
    # segments of one base; a codon in one, two and three segments; every phase with L - p in 0 .. 3
    rows, flags = [], []

    def rec(segments, phase=0):
        for s, e in segments:
            rows.append((len(flags), 0, s, e))
        flags.append(phase << 1)

    rec([(100, 101), (200, 201), (300, 301)])                      # three one-base segments: one codon across three
    rec([(100, 102), (200, 201), (300, 306)])                      # across two
    rec([(i * 10, i * 10 + 1) for i in range(50, 91)])             # 41 one-base segments
    for p in (0, 1, 2):
        for left in (0, 1, 2, 3):
            n = p + left
            if n:
                rec([(400, 400 + n)], p)
                rec([(500 + 2 * i, 500 + 2 * i + 1) for i in range(n)], p)
    rec([(0, 1)]), rec([(29999, 30000)]), rec([(0, 30000)])        # a sequence's first and last base, all of it
    rows, flags = _with_minus_twins(rows, flags)
    for translated in (False, True):
        for w in (60, 1, 0):
            _check(genome, rows, flags, translated, w, slices=(7,))


def test_a_member_beyond_the_end_drops_its_record_only(genome):
    rows = [(0, 1, 0, 997), (1, 1, 990, 998), (2, 1, 5, 50), (3, 2, 0, 64), (3, 2, 63, 65), (4, 2, 0, 64), (5, 3, 0, 1), (6, 0xFFFFFFFF, 0, 1), (7, 1, 996, 997)]
    flags = [0, 0, 1, 1, 0, 3, 0, 0]
    want = _check(genome, rows, flags, False, 60)
    g, seqs = genome
    keep = [r for r in rows if r[0] in (0, 2, 4, 7)]
    renum = {0: 0, 2: 1, 4: 2, 7: 3}
    alone, _, _ = sd.bodies(seqs, [(renum[r], q, s, e) for r, q, s, e in keep], [0, 1, 0, 0], False, 60)
    assert want == alone  # the neighbours' bytes as without the dropped records
    _check(genome, rows, flags, True, 60)
    # dropped by the caller
    _check(genome, [(0, 1, 0, 10), (1, 1, 0, 10), (2, 1, 0, 10)], [0, 8, 1], False, 60)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_record_counts(genome, n):
    rng = random.Random(n)
    rows, flags = [], []
    for r in range(n):
        q = rng.choice((0, 0, 1))
        top = (30000, 997)[q]
        for _ in range(rng.randrange(1, 5)):
            s = rng.randrange(0, top - 1)
            rows.append((r, q, s, min(top, s + rng.randrange(1, 300))))
        flags.append(rng.randrange(2) | rng.randrange(3) << 1)
    rng.shuffle(rows)
    for translated in (False, True):
        _check(genome, rows, flags, translated, 60, slices=(engine.SEQ_TILE + 1,) if n == 65 else ())


def test_one_record_of_5000_segments_duplicates_and_overlaps(genome):
    rng = random.Random(77)
    rows = [(0, 0, s, s + rng.randrange(1, 40)) for s in (rng.randrange(0, 29900) for _ in range(5000))]
    rows += [(1, 0, 50, 80), (1, 0, 50, 80), (1, 0, 60, 100), (1, 0, 50, 51), (1, 0, 40, 120)]  # duplicates, overlaps, the same start
    rows += [(2, 0, s, e) for _, _, s, e in rows[:5000]]
    for translated in (False, True):
        _check(genome, rows, [0, 1, 5], translated, 60, slices=(7,) if not translated else ())


def test_slices_of_1_7_and_a_tile_plus_1_against_one_slice(genome):
    rng = random.Random(8)
    rows, flags = [], []
    for r in range(40):
        for _ in range(rng.randrange(1, 4)):
            s = rng.randrange(0, 29000)
            rows.append((r, 0, s, s + rng.randrange(1, 400)))
        flags.append(rng.randrange(2) | rng.randrange(3) << 1)
    for translated, w in ((False, 60), (True, 60), (False, 0), (True, 1)):
        _check(genome, rows, flags, translated, w, slices=(7, engine.SEQ_TILE + 1))
        few = [r for r in rows if r[0] < 5]  # (a slice per byte: a launch per byte)
        _check(genome, few, flags[:5], translated, w, slices=(1,))


def test_refused_arguments_leave_an_error_not_a_crash(genome):
    g, _ = genome
    ok = np.array([(0, 0, 0, 5)], np.uint32)
    for rows, flags, what in (([(1, 0, 0, 5)], [0], b"record >= n_records"), ([(0, 0, 5, 5)], [0], b"start >= end"), ([(0, 0, 0, 5)], [6], b"rec_flags"),
                              ([(0, 0, 0, 5)], [0, 0], b"record")):
        with pytest.raises(_ffi.GffxHipError) as ei:
            engine.SeqPlan(g, np.array(rows, np.uint32), np.array(flags, np.uint8))
        assert what in str(ei.value).encode(), str(ei.value)
    p = engine.SeqPlan(g, ok, np.array([0], np.uint8))
    with pytest.raises(_ffi.GffxHipError):
        p.emit(0, p.body_bytes + 1)
    assert p.emit() == sd.bodies(genome[1], [(0, 0, 0, 5)], [0], False, 60)[0]  # still usable
    p.close()
    empty = engine.SeqPlan(g, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint8))
    assert empty.body_bytes == 0 and empty.emit() == b""
    empty.close()
    unfinished = engine.Genome()
    with pytest.raises(_ffi.GffxHipError):
        engine.SeqPlan(unfinished, ok, np.array([0], np.uint8))
    unfinished.close()
