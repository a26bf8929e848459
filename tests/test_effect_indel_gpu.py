"""engine.Effect.run_any (k_effect_alleles_any and k_effect_pairs_any of device/effect.hip) against
tests/_effect_indel_definition.py, bit for bit: the edge cases the host tool is held to (test_effect_indel_cpu.py), pair counts
around a wave and a block, alleles with 0, 1 and 300 transcripts, transcripts of 5000 segments, an unclassified_model transcript
between classified ones, an arena and a record buffer that grow, chunks of 1, 3 and 7 alleles with an indel's bytes at a chunk's
end, pieces of 65 535 bytes (ref_match over 65 535 bases in one thread of k_effect_alleles_any, windows of 21 845 codons in one
thread of k_effect_pairs_any), the sticky failure of a row whose bytes leave the arena, and a chunk of SNVs equal to Effect.run
byte for byte.  Left to the host tool (test_effect_indel_cpu.py): coordinates at 2^32 - 1, which need a genome of 4 GB on the
device, and an arena offset beyond 2^32, which needs an arena of 4 GB; neither is a test of a few seconds."""
import numpy as np
import pytest

import _effect_definition as D
import _effect_indel_definition as X
from gffx_amd import _ffi, engine

pytestmark = pytest.mark.gpu

if engine.device_count() < 1:
    pytest.skip("needs an MI355X", allow_module_level=True)

SEQ0 = bytes(b"ACGTTGCAAGCTNACGGTCA"[i % 20] for i in range(400))
SEQ1 = bytes(b"TTGACCATGGNCATCGA"[i % 17] for i in range(90))
SEQ2 = bytes(b"GATTACA"[i % 7] for i in range(50))
# t0 on s0: four CDS segments and UTR exons, phase 1; t1 its minus twin, phase 2; t2 on s1; s2 has none
WORLD_ROWS = ([(0, 0, 19, 40, 0), (0, 0, 44, 47, 0), (0, 0, 60, 130, 0), (0, 0, 140, 300, 0), (0, 0, 9, 40, 1), (0, 0, 44, 47, 1), (0, 0, 60, 130, 1), (0, 0, 140, 320, 1)] +
              [(1, 0, 19, 40, 0), (1, 0, 44, 47, 0), (1, 0, 60, 130, 0), (1, 0, 140, 300, 0)] + [(2, 1, 4, 20, 0)])
WORLD_FLAGS = [2, 1 | 4, 0]


def fasta_of(seqs):
    return b"".join(b">s%d\n" % i + s + b"\n" for i, s in enumerate(seqs))


def device_tuples(rec):
    return [(int(r["q"]), int(r["c"]), int(r["transcript"]), int(r["cls"]), int(r["k"]), int(r["ref_match"]), int(r["aa_ref"]), int(r["aa_alt"]),
             tuple(int(x) for x in r["codon_ref"]), tuple(int(x) for x in r["codon_alt"])) for r in rec]


def check(seqs, rows, flags, alleles, chunk=None, max_alleles=None):
    """Build the object, run the alleles (in chunks of `chunk`), hold everything to the definition; (stats, records, wanted)."""
    g = engine.genome_from_fasta(fasta_of(seqs))
    try:
        e = engine.Effect(g, np.array(rows, dtype=np.uint32).reshape(-1, 5), flags, max_alleles or max(len(alleles), 1))
        try:
            a, arena = engine.effect_rows_any(alleles)
            assert (a.tolist(), arena) == (list(map(list, X.device_rows(alleles)[0])), X.device_rows(alleles)[1])
            off, rm, rec = e.run_any_chunked(a, arena, chunk) if chunk else e.run_any(a, arena)
            want_off, want_rm, want = X.pairs_any(seqs, rows, flags, alleles)
            assert list(off) == want_off
            assert list(rm) == want_rm
            assert device_tuples(rec) == X.device_records(want)
            assert all(int(r["pad"]) == 0 for r in rec)
            return e.stats(), rec, want
        finally:
            e.close()
    finally:
        g.close()


def test_the_class_names_and_the_trimming():
    assert engine.EFFECT_CLASSES_ALL == X.CLASSES_ALL and engine.EFFECT_CLASSES_ALL[:15] == engine.EFFECT_CLASSES
    for pos, ref, alt in ((7, b"ATG", b"ACG"), (1, b"A", b"GA"), (5, b"acG", b"ACGT"), (9, b"TTT", b"T"), (3, b"GAT", b"gat"), (4, b"CAG", b"TAGAG")):
        assert engine.effect_trim(pos, ref, alt) == X.trim(pos, ref, alt)
    assert engine.effect_trim(7, b"ATG", b"ACG") == (8, 1, 1, b"T", b"C")


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_the_edge_cases_of_the_host_tool(name):
    seqs, rows, flags, alleles = X.CASES[name]()
    _, _, want = check(seqs, rows, flags, alleles)
    assert len(want) > 500


def test_pieces_of_65535_bytes():
    seqs, rows, flags, alleles = X.case_long_pieces()
    _, rec, want = check(seqs, rows, flags, alleles)
    assert max(len(a[2]) for a in alleles) == 65535 and max(len(a[3]) for a in alleles) == 65534
    assert [r[1] for r in want[4:10]] == ["stop_lost"] * 4 + ["inframe_deletion"] * 2  # (rule 3d over 21 845 codons)
    # the same rows in chunks of one: every chunk's arena is its own allele's bytes
    check(seqs, rows, flags, alleles, chunk=1, max_alleles=1)


@pytest.mark.parametrize("seed", range(4))
def test_random_disjoint_transcripts(seed):
    seqs, rows, flags, alleles = X.random_disjoint_case(200 + seed, n_tr=30, n_alleles=400)
    _, _, want = check(seqs, rows, flags, alleles)
    assert len({r[1] for r in want}) >= 12


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65, 256, 257])
def test_pair_counts_around_a_wave_and_a_block(n_pairs):
    # t0 spans [10, 320] of s0; every allele below lies inside it; alleles on s2 and in s1's gap hit nothing
    rows = [(0, q, s, e, k) for t, q, s, e, k in WORLD_ROWS if t == 0] + [(1, q, s, e, k) for t, q, s, e, k in WORLD_ROWS if t == 2]
    seqs = [SEQ0, SEQ1, SEQ2]
    alleles = [X.allele(seqs, 2, 5, 2, 0), X.allele(seqs, 1, 60, 0, 2)]
    alleles += [X.allele(seqs, 0, 12 + (37 * i) % 300, i % 5, (i // 5) % 4 + (1 if i % 5 == 0 else 0), salt=i) for i in range(n_pairs)]
    alleles += [X.allele(seqs, 0, 350, 3, 1), X.allele(seqs, 1, 2, 1, 0)]
    assert all(alleles)
    _, _, want = check(seqs, rows, [2, 0], alleles)
    assert len(want) == n_pairs


def test_alleles_with_0_1_and_300_transcripts_and_buffers_that_grow():
    rows, flags = [], []
    for t in range(300):  # all over base 200 of s0, each with its own segments
        s = 199 - (t * 7) % 150
        rows += [(t, 0, s, 205 + t % 11, 0), (t, 0, 230 + t % 5, 260, 0), (t, 0, max(s - 3, 0), 205 + t % 11, 1), (t, 0, 230 + t % 5, 270 + t % 3, 1)]
        flags.append(t % 2 | (t % 3) << 1)
    rows, flags = rows + [(300, 1, 10, 30, 0)], flags + [0]
    seqs = [SEQ0, SEQ1]
    g = engine.genome_from_fasta(fasta_of(seqs))
    try:
        e = engine.Effect(g, np.array(rows, dtype=np.uint32), flags, 64)
        try:
            small = [X.allele(seqs, 0, 390, 2, 0), X.allele(seqs, 1, 15, 0, 3), X.allele(seqs, 0, 200, 4, 1)]
            many = [X.allele(seqs, 0, 200 + i, i % 4, 1 + i % 3, salt=i) for i in range(8)] + small + [X.allele(seqs, 0, 198, 40, 700)]
            for alleles, n in ((small, 301), (many, None)):
                a, arena = engine.effect_rows_any(alleles)
                off, rm, rec = e.run_any(a, arena)
                want_off, want_rm, want = X.pairs_any(seqs, rows, flags, alleles)
                assert list(off) == want_off and list(rm) == want_rm and device_tuples(rec) == X.device_records(want)
                assert n is None or len(want) == n
            assert len(want) > 1024 and [int(off[i + 1] - off[i]) for i in (8, 9, 10)] == [0, 1, 300]
            stats = e.stats()
            assert stats["grows"] >= 1 and stats["arena_grows"] >= 1  # (9 bytes, then more than 700)
        finally:
            e.close()
    finally:
        g.close()


def test_transcripts_of_5000_segments():
    rng = np.random.RandomState(5)
    big = bytes(rng.choice(list(b"ACGT"), 16000).astype(np.uint8))
    rows = [(0, 0, 3 * i + 1, 3 * i + 1 + 1 + i % 2, 0) for i in range(5000)]
    rows += [(0, 0, 3 * i + 1, 3 * i + 3, 1) for i in range(0, 5000, 2)]  # exons: every other segment, a base longer; many touch
    rows += [(1, 0, 3 * i + 1, 3 * i + 2, 0) for i in range(5000)] + [(2, 0, 15500, 15501, 0), (3, 0, 0, 16000, 1)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    xs = list(range(2, 10)) + list(range(7494, 7500)) + list(range(14996, 15004)) + [15499, 15500, 15501, 15502, 15999]
    alleles = X.alleles_at([big], xs, ((1, 0), (0, 1), (2, 2), (7, 1), (0, 3), (40, 1)))
    check([big], rows, [1 | 2, 0, 0, 1], alleles)


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_chunks_through_the_two_slots(chunk):
    seqs, rows, flags, alleles = X.random_disjoint_case(7, n_tr=30, n_alleles=148)
    alleles += [X.allele(seqs, 0, 40, 9, 30)]  # (149 = 7 * 21 + 2 = 3 * 49 + 2: the last chunks end on its bytes)
    check(seqs, rows, flags, alleles, chunk=chunk, max_alleles=chunk)
    check(seqs, rows, flags, alleles[-chunk:] + alleles[:-chunk], chunk=chunk, max_alleles=chunk)  # (and the first chunk)


def test_a_chunk_of_snvs_is_run_byte_for_byte():
    seqs, rows, flags, snvs = D.random_case(100, n_tr=40, n_alleles=300)
    g = engine.genome_from_fasta(fasta_of(seqs))
    try:
        e = engine.Effect(g, np.array(rows, dtype=np.uint32).reshape(-1, 5), flags, 512)
        try:
            off, rm, rec = e.run(np.array(snvs, dtype=np.uint32))
            a, arena = engine.effect_rows_any([(q, x, bytes([ra & 255]), bytes([ra >> 8])) for q, x, ra in snvs])
            off2, rm2, rec2 = e.run_any(a, arena, slot=1)
            assert off.tobytes() == off2.tobytes() and rm.tobytes() == rm2.tobytes() and rec.tobytes() == rec2.tobytes() and len(rec) > 100
        finally:
            e.close()
    finally:
        g.close()


def test_bad_rows_fail_the_run_and_the_failure_sticks():
    seqs = [SEQ0, SEQ1]
    g = engine.genome_from_fasta(fasta_of(seqs))
    try:
        good, arena = engine.effect_rows_any([X.allele(seqs, 0, 25, 2, 0)])
        for bad, code in (([(0, 25, 2, 0, 0, 0), (0, 30, 1, 2, len(arena) - 2, 0)], -1),   # its last byte lies behind the arena
                          ([(0, 25, 2, 0, 0, 1)], -1),                                        # an offset of 2^32
                          ([(2, 25, 2, 0, 0, 0)], -5), ([(0, 0, 2, 0, 0, 0)], -5), ([(0, 25, 0, 0, 0, 0)], -5), ([(0, 1, 0, 2, 0, 0)], -5),
                          ([(0, 25, 65536, 0, 0, 0)], -5)):
            e = engine.Effect(g, np.array(WORLD_ROWS, dtype=np.uint32), WORLD_FLAGS, 16)
            try:
                assert len(e.run_any(good, arena)[2]) == 2
                with pytest.raises(_ffi.GffxHipError) as ei:
                    e.run_any(np.array(bad, dtype=np.uint32), arena)
                assert ei.value.code == code, bad
                for again in (lambda: e.run_any(good, arena), lambda: e.run(np.array([(0, 25, 65 | 67 << 8)], dtype=np.uint32))):
                    with pytest.raises(_ffi.GffxHipError) as ei:
                        again()
                    assert ei.value.code == code and "failed earlier" in str(ei.value)
            finally:
                e.close()
    finally:
        g.close()


def test_an_allele_that_reaches_beyond_the_sequence_or_lies_on_none():
    seqs = [SEQ0, SEQ1]
    alleles = [(0, 399, b"CA", b""), (0, 400, b"AC", b""), (0, 400, b"", b"GG"), (0, 401, b"", b"GG"), (D.NO_SEQ, 5, b"A", b""), (1, 89, b"GAT", b"C"), (1, 15, b"NN", b"")]
    _, rec, want = check(seqs, WORLD_ROWS, WORLD_FLAGS, alleles)
    assert len(want) == 1
