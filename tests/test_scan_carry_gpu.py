"""The two-level prefix sums behind `gffx seq`, `gffx effect` and `gffx annotate` past one step of their carry walk, bit for bit
against the definitions (tests/_seq_definition.py, _effect_definition.py, _annotate_definition.py).

Every scan here reduces tiles of `tile` values, then ONE block walks the tile sums in steps of `carry_tiles` tiles with a running
value from step to step.  The second step runs only when a scan has more than STEP = tile * carry_tiles values; the library
reports both numbers (engine.scan64_constants, engine._classmap_constants) and every case below asserts the size that makes it
meaningful, so a changed constant fails a test instead of quietly un-crossing it.

  scan64.hpp   k_scan64_carry behind the genome's kept bytes per line (`dst`), the seq plan's `pre` (rows) and `body_off`
               (records) and the effect build's `pre` (rows).  The genome's other scan, the line counts per 4 KiB text tile, gets
               its second scan TILE here; its second carry STEP cannot be reached (chunk_bytes is capped at 1 GiB, which is
               exactly carry_tiles scan tiles of text tiles).
  classmap.hip k_classmap_carry (the XOR of the toggles and the mask behind the last tail, from step to step),
               k_classmap_carry_sum (points per tile) and k_classmap_carry_bases (bases per class and tile of POINTS).
Beside them: the u64 sums `pre` across 2^32 (the rows of records the caller dropped count, so no large allocation is needed), and
the sort plans of seq and effect at the record / transcript counts where they take another key byte.

Inputs are drawn with numpy; the definitions are the cost of these tests, the device work is milliseconds."""
import numpy as np
import pytest

import _annotate_definition as ad
import _effect_definition as D
import _seq_definition as sd
from gffx_amd import engine
from test_annotate_gpu import device as classmap_device
from test_seq_gpu import _check_genome

pytestmark = pytest.mark.gpu

TEXT_TILE = 4096  # bytes per tile of the line kernels (line_scan.hpp); the library does not report it
BASES = np.frombuffer(b"ACGTacgtNn", np.uint8)


def scan_step():
    tile, carry_tiles = engine.scan64_constants()
    return tile * carry_tiles


def key_bytes(top):
    """The key bytes a sort plan takes for keys 0 .. top: byte b > 0 while top >> 8 b is not 0."""
    return max(1, (int(top).bit_length() + 7) // 8)


def one_base_lines(rng, k):
    two = np.empty((k, 2), np.uint8)
    two[:, 0], two[:, 1] = rng.choice(BASES, k), 10
    return two.tobytes()


def n_lines_of(text):
    return text.count(b"\n") + (0 if text.endswith(b"\n") or not text else 1)


# ---- the genome: the kept-bytes scan over lines --------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["STEP-1", "STEP", "STEP+1", "2*STEP+1"])
def test_genome_line_counts_around_the_carry_step(which):
    """Lines of one base; the count is the sub-batch's lines WITH the header line: the values k_scan64_carry's scan is over."""
    STEP = scan_step()
    n_lines = {"STEP-1": STEP - 1, "STEP": STEP, "STEP+1": STEP + 1, "2*STEP+1": 2 * STEP + 1}[which]
    text = b">s0 one base per line\n" + one_base_lines(np.random.default_rng(n_lines), n_lines - 1)
    assert n_lines_of(text) == n_lines and (n_lines > STEP) == (which in ("STEP+1", "2*STEP+1"))
    g = engine.genome_from_fasta(text)  # (one sub-batch: the text is far below the default chunk)
    try:
        assert g.n_bases == n_lines - 1
        _check_genome(g, text)
    finally:
        g.close()


def mixed_text(STEP):
    """STEP + 64 lines: a header on the last line of step 0 (its sequence is empty) and one on the first line of step 1, so
    k_genome_header_dst reads a `dst` carried across the step; two more headers; empty lines; CR LF ends on both sides of the
    step; no final newline.  (Past STEP + 1 lines: with that count alone the only line of step 1 would be the last header.)"""
    n = STEP + 64
    rng = np.random.default_rng(5)
    bases = rng.choice(BASES, n).tobytes()
    lines, ends = [bases[i:i + 1] for i in range(n)], [b"\n"] * n
    for i in range(n):
        if i % 7 == 3:
            ends[i] = b"\r\n"
        if i % 11 == 5:
            lines[i] = b""
    lines[0], ends[0] = b">s0 first", b"\n"
    lines[1000] = b">s1\tdesc"
    lines[STEP - 2], ends[STEP - 2] = b"G", b"\r\n"
    lines[STEP - 1], ends[STEP - 1] = b">empty sequence", b"\r\n"
    lines[STEP], ends[STEP] = b">s2", b"\r\n"
    lines[STEP + 1], ends[STEP + 1] = b"T", b"\r\n"
    lines[STEP + 2], ends[STEP + 2] = b"", b"\r\n"
    lines[STEP + 30], ends[STEP + 30] = b">s3", b"\n"
    lines[n - 1], ends[n - 1] = b"ACGTN", b""
    return b"".join(a + b for a, b in zip(lines, ends))


def test_genome_headers_on_both_sides_of_the_carry_step():
    STEP = scan_step()
    text = mixed_text(STEP)
    raw = text.split(b"\n")
    assert n_lines_of(text) == STEP + 64 > STEP + 1 and not text.endswith(b"\n")
    assert raw[STEP - 1].startswith(b">empty") and raw[STEP].startswith(b">s2") and raw[STEP - 2] == b"G\r" and raw[STEP + 1] == b"T\r"
    names, seqs = sd.parse_fasta(text)
    assert names == [b"s0", b"s1", b"empty", b"s2", b"s3"] and seqs[2] == b"" and all(len(s) for k, s in enumerate(seqs) if k != 2)
    g = engine.genome_from_fasta(text)
    try:
        _check_genome(g, text)
    finally:
        g.close()


def test_genome_sub_batches_past_the_step_cut_inside_a_line():
    """chunk_bytes of an odd size: the first two sub-batches have more than STEP lines each, the second begins inside a bases
    line (the cut has bases on both sides) at an arena offset that is no multiple of 16; a short third one follows."""
    STEP = scan_step()
    head = b">s0\n"
    k, long_at = 2 * STEP + 40, STEP + 10
    body = one_base_lines(np.random.default_rng(9), k)
    at = 2 * long_at
    text = head + body[:at] + b"ACGTACGTA\n" + body[at + 2:]
    chunk = len(head) + at + 1  # behind the long line's first base
    first, second = text[:chunk], text[chunk:2 * chunk]
    kept_first = len(first) - len(head) - first.count(b"\n")
    assert chunk % 2 == 1 and first[-1:] == b"A" and second[:1] == b"C" and kept_first % 16 != 0
    assert n_lines_of(first) > STEP and n_lines_of(second) > STEP and 0 < len(text) - 2 * chunk < chunk
    g = engine.genome_from_fasta(text, chunk_bytes=chunk)
    try:
        _check_genome(g, text)
    finally:
        g.close()


# ---- the genome: the line-count scan over text tiles -----------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1", "2*tile+1"])
def test_genome_text_tiles_around_the_scan_tile(which):
    """60-base lines, 4 .. 8 MiB in one sub-batch: `line_base` gets its second and third scan tile.  The carry STEP of this scan
    cannot be reached: chunk_bytes is capped at 1 GiB = carry_tiles * tile text tiles of 4 KiB, exactly one step."""
    tile, carry_tiles = engine.scan64_constants()
    assert tile * carry_tiles * TEXT_TILE >= 1 << 30  # (the cap of chunk_bytes in gffx_hip_genome_create)
    tiles = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2*tile+1": 2 * tile + 1}[which]
    # the last text tile: 5 bytes short, full, and holding one byte only
    N = {"tile-1": tiles * TEXT_TILE - 5, "tile": tiles * TEXT_TILE, "tile+1": (tiles - 1) * TEXT_TILE + 1, "2*tile+1": (tiles - 1) * TEXT_TILE + 1}[which]
    head = b">s0 sixty per line\n"
    full, rem = divmod(N - len(head), 61)
    rng = np.random.default_rng(tiles)
    body = np.empty((full, 61), np.uint8)
    body[:, :60], body[:, 60] = rng.choice(BASES, (full, 60)), 10
    text = head + body.tobytes() + (rng.choice(BASES, rem - 1).tobytes() + b"\n" if rem else b"")
    assert len(text) == N and -(-N // TEXT_TILE) == tiles and (tiles > tile) == (which in ("tile+1", "2*tile+1"))
    g = engine.genome_from_fasta(text)
    try:
        _check_genome(g, text)
    finally:
        g.close()


# ---- the seq plan --------------------------------------------------------------------------------------------------------------------

def np_genome(seed, lengths):
    rng = np.random.default_rng(seed)
    seqs = [rng.choice(np.frombuffer(b"ACGTacgtNnRYKMBVDHSWUu", np.uint8), n).tobytes() for n in lengths]
    text = b"".join(b">s%d\n" % i + sd.wrap(s, 60) for i, s in enumerate(seqs))
    return engine.genome_from_fasta(text), seqs


@pytest.fixture(scope="module")
def genome():
    g, seqs = np_genome(3, (30000, 997))
    yield g, seqs
    g.close()


@pytest.fixture(scope="module")
def genome_1m():
    g, seqs = np_genome(4, (1 << 20,))
    yield g, seqs
    g.close()


def check_plan(genome, rows, flags, translated, w, slices=()):
    g, seqs = genome
    rows, flags = np.ascontiguousarray(rows, np.uint32).reshape(-1, 4), np.ascontiguousarray(flags, np.uint8)
    want, off, dropped = sd.bodies(seqs, rows.tolist(), flags.tolist(), translated, w)
    p = engine.SeqPlan(g, rows, flags, translated, w)
    try:
        assert np.array_equal(p.body_off, np.array(off, np.uint64)) and p.dropped.tolist() == dropped and p.body_bytes == len(want)
        assert p.emit() == want
        for s in slices:
            assert p.emit_sliced(s) == want, s
    finally:
        p.close()
    return off, dropped


def short_rows(rng, records, per_record):
    """`per_record` rows of 1 .. 7 bases on sequence 0 for each of `records` records; strands and phases drawn, a few records
    dropped by the caller."""
    n = records * per_record
    s = rng.integers(0, 30000 - 7, n)
    rows = np.stack([np.repeat(np.arange(records), per_record), np.zeros(n, np.int64), s, s + rng.integers(1, 8, n)], 1)
    flags = (rng.integers(0, 2, records) | rng.integers(0, 3, records) << 1).astype(np.uint8)
    flags[rng.integers(0, records, 5)] |= 8
    return rows, flags


@pytest.mark.parametrize("which", ["STEP-1", "STEP", "STEP+1"])
def test_seq_one_row_records_around_the_carry_step(genome, which):
    """R = n: the scan of `pre` (rows) and the scan of `body_off` (records) take their second carry step together."""
    STEP = scan_step()
    R = {"STEP-1": STEP - 1, "STEP": STEP, "STEP+1": STEP + 1}[which]
    rows, flags = short_rows(np.random.default_rng(R), R, 1)
    assert len(rows) == len(flags) == R and (R > STEP) == (which == "STEP+1")
    off, dropped = check_plan(genome, rows, flags, False, 60, slices=(engine.SEQ_TILE + 1,) if which == "STEP+1" else ())
    assert off[-1] > 2 * R and sum(dropped) >= 1


@pytest.mark.parametrize("translated", [False, True])
def test_seq_shuffled_rows_past_the_carry_step(genome, translated):
    STEP = scan_step()
    R = STEP + 1
    rng = np.random.default_rng(11)
    rows, flags = short_rows(rng, R, 1)
    assert len(rows) == R > STEP and set((flags & 7).tolist()) == {0, 1, 2, 3, 4, 5}  # both strands, all phases
    check_plan(genome, rows[rng.permutation(R)], flags, translated, 60)


@pytest.mark.parametrize("translated", [False, True])
def test_seq_rows_past_the_carry_step_records_below_it(genome, translated):
    STEP = scan_step()
    R = STEP // 4 + 1
    rng = np.random.default_rng(12)
    rows, flags = short_rows(rng, R, 4)
    assert len(rows) > STEP >= R
    check_plan(genome, rows[rng.permutation(len(rows))], flags, translated, 0 if translated else 60)


def rows_across_2_32():
    """(the rows of a dropped first unit whose lengths sum to 2^32 - 50, the three segments of the units behind it): `pre` at the
    first of them is 2^32 - 50 and passes 2^32 inside the second."""
    big = np.zeros((4096, 2), np.int64)
    big[:, 1] = 1 << 20
    big[4095, 1] -= 50
    segments = [(100, 130), (200, 230), (300, 340)]
    before = int((big[:, 1] - big[:, 0]).sum())
    assert before == (1 << 32) - 50 and before + 30 < 1 << 32 < before + 60
    return big, segments


@pytest.mark.parametrize("translated", [False, True])
def test_seq_row_sums_across_2_32(genome_1m, translated):
    """Record 0 (dropped by the caller) holds 2^32 - 50 bases of rows; record 1's sum passes 2^32 inside its second row; record 2,
    its minus twin, lies wholly above."""
    big, segments = rows_across_2_32()
    rows = [(0, 0, s, e) for s, e in big.tolist()] + [(r, 0, s, e) for r in (1, 2) for s, e in segments]
    rows = np.array(rows, np.int64)[np.random.default_rng(2).permutation(len(rows))]
    for p in (0, 1, 2):
        for w in (60, 0):
            off, dropped = check_plan(genome_1m, rows, [8, p << 1, 1 | p << 1], translated, w)
            assert dropped == [1, 0, 0] and off[1] == 0 and off[2] > 0


@pytest.mark.parametrize("R,record_bytes", [(256, 1), (257, 2), (65536, 2), (65537, 3)])
def test_seq_sort_plan_takes_another_record_byte(genome, R, record_bytes):
    """The rows of record 0 and of record R - 1 come last in the input: without the top key byte they stay among each other."""
    assert key_bytes(R - 1) == record_bytes
    rng = np.random.default_rng(R)
    rows, flags = short_rows(rng, R, 2)
    ends = (rows[:, 0] == 0) | (rows[:, 0] == R - 1)
    mid = rows[~ends]
    rows = np.concatenate([mid[rng.permutation(len(mid))], rows[ends][[0, 2, 1, 3]]])
    flags[[0, R - 1]] &= 7
    _, dropped = check_plan(genome, rows, flags, False, 60)
    assert dropped[0] == dropped[R - 1] == 0


# ---- the effect build ------------------------------------------------------------------------------------------------------------------

def effect_tools():
    import test_effect_gpu as te  # (skips at import on a machine without a device)
    return te.check, te.al


def slot_transcripts(T, rows_of):
    """Transcript t in bases [15 t + 3, 15 t + 18) of sequence 0: `rows_of(t)` picks its member rows among CDS (a + 2, a + 5),
    (a + 7, a + 11) and exon (a + 1, a + 5), (a + 7, a + 13); strands and phases by number, every 1000th dropped by the caller."""
    t = np.arange(T, dtype=np.int64)
    a = 15 * t + 3
    z = np.zeros(T, np.int64)
    kinds = [np.stack([t, z, a + 2, a + 5, z], 1), np.stack([t, z, a + 7, a + 11, z], 1), np.stack([t, z, a + 1, a + 5, z + 1], 1),
             np.stack([t, z, a + 7, a + 13, z + 1], 1)]
    rows = np.concatenate([k[rows_of(t, j)] for j, k in enumerate(kinds)])
    flags = ((t % 2) | (t % 3) << 1 | np.where(t % 1000 == 7, 8, 0)).astype(np.uint8)
    return rows, flags


def slot_alleles(al, seq, picks):
    """Per picked transcript an allele in its leading UTR, both CDS segments, the gap between them and the trailing UTR."""
    out = []
    for t in picks:
        a = 15 * t + 3
        out += [al(0, x, seq[x - 1], b"ACGT"[(x + t) % 4]) for x in (a + 2, a + 4, a + 6, a + 7, a + 9, a + 12)]
    return out


def test_effect_rows_past_the_carry_step_and_a_third_key_byte(genome_1m):
    check, al = effect_tools()
    STEP = scan_step()
    T = 66000
    rows, flags = slot_transcripts(T, lambda t, j: np.ones(len(t), bool))
    assert len(rows) == 4 * T > STEP and key_bytes(2 * T - 1) == 3 and 15 * T + 18 <= 1 << 20
    rng = np.random.default_rng(6)
    rows = rows[rng.permutation(len(rows))]
    picks = [0, 1, 7, 127, 128, 32767, 32768, T - 1]  # (7: dropped by the caller)
    alleles = slot_alleles(al, genome_1m[1][0], picks) + [al(0, 1, ord("A"), ord("C")), al(0, 1 << 20, ord("A"), ord("C"))]
    _, n = check(genome_1m[1], rows.tolist(), flags.tolist(), alleles, genome=genome_1m[0])
    assert n == 6 * (len(picks) - 1)  # every allele of a kept pick lies in its span


@pytest.mark.parametrize("T,key", [(128, 1), (129, 2), (32768, 2), (32769, 3)])
def test_effect_sort_plan_takes_another_key_byte(genome_1m, T, key):
    """Keys are 2 t + kind: transcripts of one row (CDS) and of two (CDS and exon), alleles on transcript 0, T - 1 and on both
    sides of keys 255 | 256 and, where there are such, 65535 | 65536."""
    check, al = effect_tools()
    assert key_bytes(2 * T - 1) == key
    rows, flags = slot_transcripts(T, lambda t, j: (j == 0) | ((j == 3) & (t % 2 == 1)))
    rng = np.random.default_rng(T)
    rows = rows[rng.permutation(len(rows))]
    picks = sorted({t for t in (0, 126, 127, 128, 32767, 32768, T - 1) if t < T})
    alleles = [a for t in picks for a in slot_alleles(al, genome_1m[1][0], [t])[:2] + slot_alleles(al, genome_1m[1][0], [t])[4:]]
    assert 12 <= len(alleles) <= 24
    _, n = check(genome_1m[1], rows.tolist(), flags.tolist(), alleles, genome=genome_1m[0])
    assert n >= len(picks)  # (the allele in the first CDS segment, at the least)


@pytest.mark.parametrize("p", [0, 1, 2])
def test_effect_row_sums_across_2_32(genome_1m, p):
    """Transcript 0 (dropped by the caller) holds 2^32 - 50 bases of CDS rows; the D of transcript 1 straddles 2^32; transcript
    2, its minus twin, and the exon rows of both lie above.  Alleles on every base from before the first exon to behind the last:
    every D row, the gaps with their splice sites, both UTRs."""
    check, al = effect_tools()
    big, segments = rows_across_2_32()
    exons = [(90, 130), (200, 230), (300, 350)]
    rows = [(0, 0, s, e, 0) for s, e in big.tolist()]
    rows += [(t, 0, s, e, 0) for t in (1, 2) for s, e in segments] + [(t, 0, s, e, 1) for t in (1, 2) for s, e in exons]
    rows = np.array(rows, np.int64)[np.random.default_rng(p).permutation(len(rows))]
    seq = genome_1m[1][0]
    alleles = [al(0, x, seq[x - 1], b"ACGT"[x % 4]) for x in range(85, 360)]
    _, n = check(genome_1m[1], rows.tolist(), [8, p << 1, 1 | p << 1], alleles, genome=genome_1m[0])
    assert n == 2 * (350 - 90)
    want = D.pairs(genome_1m[1], rows.tolist(), [8, p << 1, 1 | p << 1], alleles[15:45])[2]  # x = 100 .. 129: the first D row
    assert sum(1 for r in want if r[1] in D.CODING) >= 40


# ---- the class map ---------------------------------------------------------------------------------------------------------------------

def classmap_step():
    S, _, carry_tiles = engine._classmap_constants()
    return S, S * carry_tiles


def regions_for(rng, n_seq, want, around=()):
    """2000 drawn regions, and regions that begin or end exactly on, one base before and one behind the points `around` (indices
    into the map's points), the first and the last point."""
    p_off, pos = want[0].astype(np.int64), want[1].astype(np.int64)
    top = int(pos.max()) + 50
    out = [np.stack([rng.integers(0, n_seq, 2000), rng.integers(0, top, 2000), rng.integers(0, top, 2000)], 1)]
    for i in sorted({0, len(pos) - 1} | {i for i in around if 0 <= i < len(pos)}):
        c = int(np.searchsorted(p_off, i, side="right")) - 1
        x, nxt = int(pos[i]), int(pos[min(i + 1, len(pos) - 1)])
        out.append(np.array([[c, x, nxt], [c, max(x - 1, 0), x + 1], [c, 0, x], [c, x, ad.U32_MAX], [c, x + 1, nxt + 1], [c, x, x]], np.int64))
    return np.concatenate(out).astype(np.uint32)


def check_map(n_seq, T, rows, around=(), slow_regions=0):
    """The device against sparse_np: points, p_off, cb, counts and class bytes.  -> (what sparse_np gave, the regions)"""
    rng = np.random.default_rng(len(rows))
    points = ad.sparse_np(n_seq, T, rows, np.zeros((0, 3), np.uint32))
    regions = regions_for(rng, n_seq, points, around)
    want = ad.sparse_np(n_seq, T, rows, regions)
    got = classmap_device(n_seq, T, rows, regions)
    for name, g, w in zip(("p_off", "pos", "cls", "cb", "counts", "class"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    if slow_regions:  # ... and sparse itself, which walks every point for every region
        few = np.concatenate([regions[:slow_regions // 2], regions[-slow_regions // 2:]])
        assert ad.same(ad.sparse(n_seq, T, rows, few), want[:4] + (np.concatenate([want[4][:slow_regions // 2], want[4][-slow_regions // 2:]]),
                                                                 np.concatenate([want[5][:slow_regions // 2], want[5][-slow_regions // 2:]])))
    return want


@pytest.mark.parametrize("which", ["STEP-2", "STEP", "STEP+2", "2*STEP+2"])
def test_classmap_events_and_points_around_the_carry_step(which):
    """E - 2 events of disjoint rows in layers 0 and 1 under one cover row of layer 2: every one of the E events is a point, so
    the tiles of EVENTS (k_classmap_carry, k_classmap_carry_sum) and the tiles of POINTS (k_classmap_carry_bases) cross the step
    together.  (A span gives two events: the counts are even.)"""
    _, STEP = classmap_step()
    E = {"STEP-2": STEP - 2, "STEP": STEP, "STEP+2": STEP + 2, "2*STEP+2": 2 * STEP + 2}[which]
    inner = ad.events_case(E - 2, T=2)
    rows = np.concatenate([inner, np.array([[2, 0, 0, int(inner[:, 3].max()) + 9]], np.uint32)])
    assert 2 * len(rows) == E and (E > STEP) == (which in ("STEP+2", "2*STEP+2"))
    want = check_map(1, 3, rows, around=range(STEP - 3, STEP + 4), slow_regions=24 if which == "STEP-2" else 0)
    assert len(want[1]) == E  # no row merged into another, every event a point
    assert want[3].max() > 0 and want[3][2].max() > 0


def test_classmap_a_run_of_equal_keys_across_the_carry_step():
    """32 layers toggle at one position: the 32 equal keys are events STEP - 16 .. STEP + 15, the last tile of step 0 and the
    first of step 1."""
    _, STEP = classmap_step()
    lead = ad.events_case(STEP - 16, T=32)
    P = 1 << 21
    assert int(lead[:, 3].max()) < P - 50
    run = np.array([[k, 0, P, P + 100 + k] for k in range(32)], np.uint32)
    want = check_map(1, 32, np.concatenate([lead, run]))
    assert 2 * (len(lead) + 32) > STEP and want[1].tolist().count(P) == 1 and len(want[1]) == len(lead) * 2 + 1 + 32


def test_classmap_a_seqid_change_at_the_carry_step():
    S, STEP = classmap_step()
    a, b = ad.events_case(STEP, T=2, seq=0), ad.events_case(S + 2, T=2, seq=1)
    want = check_map(2, 2, np.concatenate([a, b]), around=range(STEP - 2, STEP + 3))
    assert want[0].tolist() == [0, STEP, STEP + S + 2]  # every event a point: seqid 1 begins with the first tile of step 1


def test_classmap_a_tile_that_cancels_under_a_mask_as_the_first_tile_of_a_step():
    """Rows of layers 0 and 2 open first, STEP - 2 events of layer 1 fill step 0, and the first tile of step 1 holds S / 2 whole rows
    of layer 1: its toggles cancel, and the mask behind the last tail before it comes from the step before (run_tail, not the
    scan inside the step).  The class is 0 all the way: two points."""
    S, STEP = classmap_step()
    m = (STEP - 2 + S) // 2
    i = np.arange(m, dtype=np.int64)
    inner = np.stack([np.full(m, 1), np.zeros(m, np.int64), 10 + 7 * i, 13 + 7 * i], 1).astype(np.uint32)
    top = 1 << 21
    assert 2 + 2 * m == STEP + S and 13 + 7 * m < top
    cover = np.array([[0, 0, 0, top], [2, 0, 1, top]], np.uint32)
    want = check_map(1, 3, np.concatenate([inner, cover]))
    assert want[1].tolist() == [0, top] and want[2].tolist() == [0, 3]
