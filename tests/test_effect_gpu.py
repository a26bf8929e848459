"""engine.Effect (device/effect.hip) against tests/_effect_definition.py, bit for bit, at the smallest shapes where its kernels can
go wrong: pair counts around a wave and a block, alleles with 0, 1 and 300 transcripts, transcripts of 1 and of 5000 segments, a
codon across three one-base segments, dropped transcripts between kept ones, a pair buffer that grows, chunks that cut a line's
ALT pieces apart, more sequences than the engine's direct pass stages in LDS, two objects on one genome, the sticky failure."""
import numpy as np
import pytest

import _effect_definition as D
from gffx_amd import _ffi, engine

pytestmark = pytest.mark.gpu

if engine.device_count() < 1:
    pytest.skip("needs an MI355X", allow_module_level=True)

Effect = engine.Effect  # (the parent commit has none: the module fails to import there)


def fasta_of(seqs):
    return b"".join(b">s%d\n" % i + s + b"\n" for i, s in enumerate(seqs))


def device_tuples(rec):
    return [(int(r["q"]), int(r["c"]), int(r["transcript"]), int(r["cls"]), int(r["k"]), int(r["ref_match"]), int(r["aa_ref"]), int(r["aa_alt"]),
             tuple(int(x) for x in r["codon_ref"]), tuple(int(x) for x in r["codon_alt"])) for r in rec]


def check(seqs, rows, flags, alleles, genome=None, chunk=None, max_alleles=None):
    """Build the object, run the alleles (in chunks of `chunk`), hold everything to the definition; returns the object's stats."""
    own = genome is None
    g = engine.genome_from_fasta(fasta_of(seqs)) if own else genome
    try:
        e = Effect(g, np.array(rows, dtype=np.uint32).reshape(-1, 5), flags, max_alleles or max(len(alleles), 1))
        try:
            assert list(e.dropped) == D.dropped(seqs, rows, flags)
            trs = D.transcripts(seqs, rows, flags)
            assert [tuple(int(v) for v in s) for s in e.span] == [(t["lo"], t["hi"]) for t in trs]
            a = np.array(alleles, dtype=np.uint32).reshape(-1, 3)
            off, rm, rec = e.run_chunked(a, chunk) if chunk else e.run(a)
            want_off, want_rm, want = D.pairs(seqs, rows, flags, alleles)
            assert list(off) == want_off
            assert list(rm) == want_rm
            assert device_tuples(rec) == D.device_records(want)
            assert all(int(r["pad"]) == 0 for r in rec)
            return e.stats(), len(want)
        finally:
            e.close()
    finally:
        if own:
            g.close()


def al(q, x, ref, alt):
    return (q, x, ref | alt << 8)


SEQ0 = bytes(b"ACGTTGCAAGCTNACGGTCA"[i % 20] for i in range(400))
SEQ1 = bytes(b"TTGACCATGGNCATCGA"[i % 17] for i in range(90))
SEQ2 = bytes(b"GATTACA"[i % 7] for i in range(50))
# t0 on s0: four CDS segments and UTR exons, phase 1; t1 its minus twin, phase 2; t2 on s1 with no allele near; s2 has none
WORLD_ROWS = ([(0, 0, 19, 40, 0), (0, 0, 44, 47, 0), (0, 0, 60, 130, 0), (0, 0, 140, 300, 0), (0, 0, 9, 40, 1), (0, 0, 44, 47, 1), (0, 0, 60, 130, 1), (0, 0, 140, 320, 1)] +
              [(1, 0, 19, 40, 0), (1, 0, 44, 47, 0), (1, 0, 60, 130, 0), (1, 0, 140, 300, 0)] + [(2, 1, 4, 20, 0)])
WORLD_FLAGS = [2, 1 | 4, 0]


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65, 257])
def test_pair_counts_around_a_wave_and_a_block(n_pairs):
    # every allele inside [10, 320] on s0 hits t0 (and t1 inside [20, 300]); alleles on s2 and in s1's gap hit nothing
    rows, flags = [r for r in WORLD_ROWS if r[0] != 1], [2, 0]
    rows = [(t if t == 0 else 1, q, s, e, k) for t, q, s, e, k in rows]
    alleles = [al(2, 5, ord("A"), ord("C")), al(1, 60, ord("T"), ord("G"))]
    alleles += [al(0, 10 + (37 * i) % 311, SEQ0[9 + (37 * i) % 311], b"ACGTN"[i % 5]) for i in range(n_pairs)]
    alleles += [al(0, 350, ord("A"), ord("G")), al(1, 1, ord("T"), ord("t"))]
    _, n = check([SEQ0, SEQ1, SEQ2], rows, flags, alleles)
    assert n == n_pairs


def test_both_strands_every_class_and_seqids_without_partner():
    alleles = [al(0, x, SEQ0[x - 1] if x % 7 else ord("N"), b"ACGTacgtN"[x % 9]) for x in range(1, 401)]
    alleles += [al(1, x, SEQ1[x - 1], ord("A")) for x in range(1, 91, 3)] + [al(2, x, ord("G"), ord("T")) for x in (1, 25, 50)]
    check([SEQ0, SEQ1, SEQ2], WORLD_ROWS, WORLD_FLAGS, alleles)


@pytest.mark.parametrize("seed", range(6))
def test_random_transcripts_with_dropped_ones_between_kept_ones(seed):
    seqs, rows, flags, alleles = D.random_case(100 + seed, n_tr=40, n_alleles=300)
    assert 0 < sum(D.dropped(seqs, rows, flags)) < 40
    check(seqs, rows, flags, alleles)


def test_one_transcript_dropped_in_each_way_between_kept_ones():
    # t0 kept; t1 mixed (a member on s1); t2 kept; t3 unservable (beyond the end of s1); t4 kept; t5 dropped by the caller; t6 kept;
    # t7 unservable (a sequence the genome lacks); t8 kept -- all over bases 21 .. 40 of their sequence
    rows = [(0, 0, 20, 40, 0), (1, 0, 20, 30, 0), (1, 1, 32, 40, 0), (2, 0, 22, 38, 0), (3, 1, 20, 30, 0), (3, 1, 80, 91, 1), (4, 1, 20, 40, 0),
            (5, 0, 20, 40, 0), (6, 0, 24, 36, 1), (7, D.NO_SEQ, 20, 40, 0), (8, 1, 25, 35, 0)]
    flags = [0, 0, 1, 0, 2, 8, 1, 0, 4]
    seqs = [SEQ0, SEQ1]
    assert D.dropped(seqs, rows, flags) == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    alleles = [al(q, x, seqs[q][x - 1], b"ACGT"[x % 4]) for q in (0, 1) for x in range(18, 44)]
    check(seqs, rows, flags, alleles)
    off, _, recs = D.pairs(seqs, rows, flags, alleles)
    assert {r[0] for r in recs} == {0, 2, 4, 6, 8} and max(b - a for a, b in zip(off, off[1:])) == 3


@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("minus", [0, 1])
def test_codon_across_three_one_base_segments(p, minus):
    # five one-base segments a base apart, then a longer one: with every phase a codon lies across three of them
    rows = [(0, 0, s, s + 1, 0) for s in (10, 12, 14, 16, 18)] + [(0, 0, 20, 27, 0)]
    alleles = [al(0, x, SEQ0[x - 1], alt) for x in range(9, 30) for alt in b"ACGT"]
    check([SEQ0], rows, [minus | p << 1], alleles)


def test_transcripts_of_one_and_of_5000_segments():
    rng = np.random.RandomState(5)
    big = bytes(rng.choice(list(b"ACGT"), 16000).astype(np.uint8))
    rows = [(0, 0, 3 * i + 1, 3 * i + 1 + 1 + i % 2, 0) for i in range(5000)]
    rows += [(0, 0, 3 * i + 1, 3 * i + 3, 1) for i in range(0, 5000, 2)]  # exons: every other segment, a base longer
    rows += [(1, 0, 15500, 15501, 0), (2, 0, 0, 16000, 1)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    xs = list(range(1, 40)) + list(range(7480, 7520)) + list(range(14990, 15010)) + [15500, 15501, 15502, 16000]
    alleles = [al(0, x, big[x - 1], b"ACGT"[x % 4]) for x in xs]
    check([big], rows, [1 | 2, 0, 1], alleles)


def test_an_allele_with_300_transcripts_and_buffers_that_grow():
    rows, flags = [], []
    for t in range(300):  # all over base 200 of s0, each with its own segments, given from the last to the first start
        s = 199 - (t * 7) % 150
        rows += [(t, 0, s, 205 + t % 11, 0), (t, 0, 230 + t % 5, 260, 0), (t, 0, max(s - 3, 0), 205 + t % 11, 1), (t, 0, 230 + t % 5, 270 + t % 3, 1)]
        flags.append(t % 2 | (t % 3) << 1)
    rows, flags = rows + [(300, 1, 10, 30, 0)], flags + [0]
    seqs = [SEQ0, SEQ1]
    g = engine.genome_from_fasta(fasta_of(seqs))
    try:
        e = Effect(g, np.array(rows, dtype=np.uint32), flags, 64)
        try:
            small = [al(0, 390, ord("A"), ord("C")), al(1, 15, SEQ1[14], ord("G")), al(0, 200, SEQ0[199], ord("T"))]
            many = [al(0, 200 + i, SEQ0[199 + i], b"ACGT"[i % 4]) for i in range(8)] + small  # more than the pair pass's first room of 1024
            for alleles, n in ((small, 301), (many, None)):
                off, rm, rec = e.run(np.array(alleles, dtype=np.uint32))
                want_off, want_rm, want = D.pairs(seqs, rows, flags, alleles)
                assert list(off) == want_off and list(rm) == want_rm and device_tuples(rec) == D.device_records(want)
                assert n is None or len(want) == n
            assert len(want) > 1024 and [int(off[i + 1] - off[i]) for i in (8, 9, 10)] == [0, 1, 300]
            assert e.stats()["grows"] >= 1
        finally:
            e.close()
    finally:
        g.close()


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunks_through_the_two_slots(chunk):
    seqs, rows, flags, alleles = D.random_case(7, n_tr=30, n_alleles=150, bad=False)
    check(seqs, rows, flags, alleles, chunk=chunk, max_alleles=chunk)


def test_more_sequences_than_the_pair_pass_stages_in_lds():
    n = 1700  # (the direct pass stages the seqid records in LDS up to 24 KiB of them: 1536)
    seqs = [bytes(b"ACGT"[(i + j) % 4] for j in range(12)) for i in range(n)]
    rows, flags = [], []
    for t, q in enumerate((0, 1, 900, 1535, 1536, 1699)):
        rows += [(t, q, 2, 5, 0), (t, q, 7, 10, 0), (t, q, 1, 11, 1)]
        flags.append(t % 2 | (t % 3) << 1)
    alleles = [al(q, x, seqs[q][x - 1], b"TGCA"[x % 4]) for q in (0, 1, 2, 899, 900, 1535, 1536, 1537, 1699) for x in (1, 2, 4, 6, 8, 11, 12)]
    check(seqs, rows, flags, alleles)


def test_two_objects_on_one_genome_and_a_missing_sequence():
    seqs, rows, flags, alleles = D.random_case(21, n_tr=20, n_alleles=120)
    alleles += [(D.NO_SEQ, 5, ord("A") | ord("C") << 8)]
    _, rows2, flags2, alleles2 = D.random_case(22, n_tr=9, n_alleles=80)
    alleles2 = [(q, min(x, len(seqs[q])), ra) for q, x, ra in alleles2]
    rows2 = [(t, q, min(s, len(seqs[q]) - 1) if q < len(seqs) else s, e, k) for t, q, s, e, k in rows2]
    g = engine.genome_from_fasta(fasta_of(seqs))
    try:
        e1 = Effect(g, np.array(rows, dtype=np.uint32), flags, 256)
        e2 = Effect(g, np.array(rows2, dtype=np.uint32), flags2, 256)
        try:
            e1.start(0, np.array(alleles, dtype=np.uint32))
            e2.start(1, np.array(alleles2, dtype=np.uint32))
            for e, r, f, a, slot in ((e2, rows2, flags2, alleles2, 1), (e1, rows, flags, alleles, 0)):
                off, rm, rec = e.wait(slot, len(a))
                want_off, want_rm, want = D.pairs(seqs, r, f, a)
                assert list(off) == want_off and list(rm) == want_rm and device_tuples(rec) == D.device_records(want)
        finally:
            e1.close()
            e2.close()
    finally:
        g.close()


def test_no_transcript_is_kept_and_no_allele_is_given():
    rows, flags = [(0, 0, 5, 10, 0), (1, 1, 5, 95, 0)], [8, 0]  # dropped by the caller; beyond the end of s1
    alleles = [al(0, 7, SEQ0[6], ord("A")), al(1, 7, ord("N"), ord("A"))]
    stats, n = check([SEQ0, SEQ1], rows, flags, alleles)
    assert stats["kept"] == 0 and n == 0
    check([SEQ0, SEQ1], WORLD_ROWS, WORLD_FLAGS, [])


def test_a_bad_row_fails_the_run_and_the_failure_sticks():
    g = engine.genome_from_fasta(fasta_of([SEQ0, SEQ1]))
    try:
        e = Effect(g, np.array(WORLD_ROWS, dtype=np.uint32), WORLD_FLAGS, 16)
        try:
            good = np.array([al(0, 25, SEQ0[24], ord("A"))], dtype=np.uint32)
            assert len(e.run(good)[2]) == 2
            with pytest.raises(_ffi.GffxHipError) as ei:
                e.run(np.array([al(0, 25, 65, 67), al(2, 1, 65, 67)], dtype=np.uint32))  # sequence number 2 of 2
            assert ei.value.code == -5
            with pytest.raises(_ffi.GffxHipError) as ei:
                e.run(good)
            assert ei.value.code == -5 and "failed earlier" in str(ei.value)
            with pytest.raises(_ffi.GffxHipError):  # (refused for its arguments)
                Effect(g, np.array([(0, 0, 5, 5, 0)], dtype=np.uint32), [0], 16)
        finally:
            e.close()
    finally:
        g.close()


def test_the_protein_law_against_the_devices_own_translation():
    """For every coding pair the translated record of the transcript over the genome with ALT written in (SeqPlan --translate, on
    the device) differs from the original's at character c exactly as aa says, and nowhere else.  50 transcripts that do not
    overlap, one allele in each, all written into one edited genome."""
    rng = np.random.RandomState(11)
    seq = bytes(rng.choice(list(b"ACGT"), 50 * 120).astype(np.uint8))
    rows, flags, alleles = [], [], []
    for t in range(50):
        at, segs = 120 * t + 3, []
        for _ in range(rng.randint(1, 5)):
            ln = int(rng.choice((1, 2, 3, 5, 9, 14)))
            segs.append((at, at + ln))
            at += ln + int(rng.randint(1, 6))
        rows += [(t, 0, s, e, 0) for s, e in segs]
        flags.append(int(rng.randint(2)) | int(rng.randint(3)) << 1)
        s, e = segs[rng.randint(len(segs))]
        x = int(rng.randint(s, e)) + 1
        alleles.append(al(0, x, seq[x - 1], int(rng.choice([b for b in b"ACGT" if b != seq[x - 1]]))))
    edited = bytearray(seq)
    for _, x, ra in alleles:
        edited[x - 1] = ra >> 8
    g, g2 = engine.genome_from_fasta(fasta_of([seq])), engine.genome_from_fasta(fasta_of([bytes(edited)]))
    try:
        e = Effect(g, np.array(rows, dtype=np.uint32), flags, 64)
        cds = np.array([r[:4] for r in rows], dtype=np.uint32)
        p1, p2 = engine.SeqPlan(g, cds, flags, translate=True, width=0), engine.SeqPlan(g2, cds, flags, translate=True, width=0)
        try:
            off, _, rec = e.run(np.array(alleles, dtype=np.uint32))
            b1, b2 = p1.emit(), p2.emit()
            assert list(off) == list(range(51)) and list(p1.body_off) == list(p2.body_off)
            n_coding = 0
            for t, r in enumerate(rec):
                assert int(r["transcript"]) == t
                a, b = b1[int(p1.body_off[t]):int(p1.body_off[t + 1])], b2[int(p2.body_off[t]):int(p2.body_off[t + 1])]
                if 1 <= int(r["cls"]) <= 7:
                    c = int(r["c"])
                    assert a[c] == int(r["aa_ref"]) and b[c] == int(r["aa_alt"]) and a[:c] == b[:c] and a[c + 1:] == b[c + 1:]
                    n_coding += 1
                else:
                    assert int(r["cls"]) == 0 and a == b  # partial_codon: the protein does not see the base
            assert n_coding >= 30
        finally:
            e.close()
            p1.close()
            p2.close()
    finally:
        g.close()
        g2.close()
