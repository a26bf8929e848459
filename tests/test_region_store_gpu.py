"""The region store (gffx_hip_regions_*: two pinned staging buffers, a ring of two chunk slots or a keep_all arena) and its three
consumers -- gffx_hip_batch_set_regions_store, gffx_hip_union_add_store, gffx_hip_lines_test_store -- at the C-ABI, at chunk sizes
of a few hundred rows: what `gffx intersect`, `depth` and `coverage` do once a BED file spans more than one chunk.  Join A results
are compared with the oracle's, Join B's with the oracle's line predicate, the union's with the spans of the same rows added
from the host.  The commands' protocol is kept throughout: wait_staging(k), and sync() of a batch that ran on slot k, before
staging buffer k is written again."""
import numpy as np
import pytest

from gffx_amd import engine, synth
from gffx_amd.engine import OverlapMode
from oracle import binding as ob

from _join_a_parity import _sorted_rows

pytestmark = pytest.mark.gpu

E = engine._ffi.GffxHipError
PAIRS = engine.OUT_FIDS | engine.OUT_OFFSETS
ROOTS_PASS = engine.OUT_ROOT_BITMAP | engine.OUT_NO_COUNTS  # what the streaming commands run, + OUT_BITMAP_KEEP after a batch's first chunk
EVERYTHING = engine.OUT_FIDS | engine.OUT_TRIPLES | engine.OUT_ROOT_BITMAP | engine.OUT_OFFSETS
N_SEQ = 3     # chr1, chr2 and a seqid without roots
GAP = (2, 7, 7 + 123457)  # a row that must never reach the device: the rootless seqid, a sentinel width


class _World:
    """One index (+ its oracle) and a pool of BED rows, built once per module."""

    def __init__(self, n_roots, seed):
        roots = synth.gencode_like_roots(n_roots, seed=seed, chroms=synth.SMALL2)
        co = np.append(roots["chr_offsets"], roots["chr_offsets"][-1]).astype(np.uint32)  # seqid 2: no roots
        self.roots, self.co = roots, co
        self.ix = engine.TreeIndexData.from_roots(co, roots["start"], roots["end"], roots["fid"])
        self.oix = ob.OracleIndex.from_roots(co, roots["start"], roots["end"], roots["fid"])


@pytest.fixture(scope="module")
def world():
    w = _World(400, seed=31)
    w.pool = synth.synth_bed(6000, seed=32, chroms=synth.SMALL2, width=(20, 40000), edge_frac=0.25, roots=w.roots)
    w.pool.setflags(write=False)
    yield w
    w.ix.close()


@pytest.fixture(scope="module")
def wide_world():
    w = _World(3000, seed=21)
    yield w
    w.ix.close()


def _take(pool, at, n):
    return pool[(at + np.arange(n)) % len(pool)]


def _pairs(counts, offsets, fids):
    """(query, root_fid) rows of a PAIRS pass, sorted."""
    c = counts.astype(np.int64)
    qid = np.repeat(np.arange(len(c), dtype=np.int64), c)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
    got = np.stack([qid, fids[offsets[:-1].astype(np.int64)[qid] + within].astype(np.int64)], axis=1)
    return got[np.lexsort((got[:, 1], got[:, 0]))]


def _oracle_pairs(oix, rows, mode, invert):
    """(counts, sorted (query, root_fid) rows, triples) of the oracle for `rows`."""
    want_t, want_c = oix.query_features(rows, int(mode), invert)
    wc = want_c.astype(np.int64)
    by_chr = np.argsort(rows[:, 0], kind="stable")  # the oracle walks seqid after seqid, regions in input order
    want = np.stack([np.repeat(by_chr, wc[by_chr]), want_t[:, 0].astype(np.int64)], axis=1)
    return want_c, want[np.lexsort((want[:, 1], want[:, 0]))], want_t


def _assert_pairs_pass(b, oix, rows, mode, invert, what):
    """A waited PAIRS pass of batch b over `rows` against the oracle: counts in input order and every query's root_fids."""
    want_c, want_p, want_t = _oracle_pairs(oix, rows, mode, invert)
    assert b.n_queries == len(rows) and b.total_hits == len(want_t), what
    got_c = b.counts()
    assert np.array_equal(got_c, want_c), what
    assert np.array_equal(_pairs(got_c, b.offsets(), b.fids()), want_p), what
    return len(want_t)


def _everything(b):
    """Every output of a waited EVERYTHING pass in a form that does not depend on the order of the segments."""
    c, off, t = b.counts(), b.offsets(), b.triples()
    assert np.array_equal(b.fids(), t[:, 0]) and int(off[-1]) == len(t) == b.total_hits
    segs = [_sorted_rows(t[int(off[i]):int(off[i]) + int(c[i])]) for i in range(len(c))]
    return c, (np.concatenate(segs) if segs else np.zeros((0, 3), np.uint32)), b.unique_roots()


def _assert_same_outputs(a, b, what):
    for x, y, name in zip(_everything(a), _everything(b), ("counts", "triples per query", "unique roots")):
        assert np.array_equal(x, y), (what, name)


# ---------------------------------------------------------------------------------------------- ring store, many chunks
def _chunk_sizes(cr):
    # 12 chunks; each slot sees 0 rows (slot 1 as its first chunk), chunk_rows - 1 and chunk_rows rows
    return [cr, 0, 1, cr - 1, 0, cr, 7, cr // 2 + 1, cr, 3, cr - 1, cr]


@pytest.mark.parametrize("chunk_rows", [257, 4096])
@pytest.mark.parametrize("mode,invert", [(OverlapMode.Contained, False), (OverlapMode.ContainsRegion, False),
                                         (OverlapMode.Overlap, False), (OverlapMode.Contained, True)])
def test_ring_store_many_chunks_through_two_batches(world, chunk_rows, mode, invert):
    """Twelve chunks alternate over the two slots of a ring store and the two batches bound to them.  Per chunk the pairs equal the
    oracle's; then the commands' own pass (root bitmap, counts waived, OUT_BITMAP_KEEP from a batch's second chunk on): the OR of
    the two bitmaps == the oracle's unique roots over ALL rows, the accumulated kept pairs == its pair count, and a zero-row chunk
    at the end changes neither."""
    store = engine.RegionStore(0, chunk_rows, False)
    batch = [engine.QueryBatch(world.ix, chunk_rows) for _ in range(2)]
    sizes = _chunk_sizes(chunk_rows)
    chunks, at = [], 0
    for n in sizes:
        chunks.append(_take(world.pool, at, n))
        at += n + 5
    assert store.rows() == 0
    for i, rows in enumerate(chunks):
        k = i & 1
        store.wait_staging(k)  # (batch k was waited below: its pass is over)
        stage = store.staging(k)
        stage[:] = GAP  # what the previous chunk of this buffer left behind must not matter
        stage[:len(rows)] = rows
        store.append(k, len(rows))
        batch[k].set_regions_store(store, k, 0, len(rows))
        batch[k].run(mode, invert, PAIRS)
        batch[k].wait()
        _assert_pairs_pass(batch[k], world.oix, rows, mode, invert, ("chunk", i, len(rows)))
    assert store.rows() == 0  # (a ring keeps nothing)

    def roots_and_kept():
        bits, kept = np.zeros(world.ix.n_roots, bool), 0
        for b in batch:
            b.wait()
            bits |= b.root_bitmap()
            kept += b.kept_pairs_accumulated
        return np.unique(world.ix.sorted_fids()[bits]), kept

    used = [False, False]
    for i, rows in enumerate(chunks):  # the streamed form: nothing is waited for between the chunks but the staging buffer
        k = i & 1
        if used[k]:
            batch[k].sync()
        store.wait_staging(k)
        stage = store.staging(k)
        stage[:len(rows)] = rows
        store.append(k, len(rows))
        batch[k].set_regions_store(store, k, 0, len(rows))
        batch[k].run(mode, invert, ROOTS_PASS | (engine.OUT_BITMAP_KEEP if used[k] else 0))
        used[k] = True
    want_t, _ = world.oix.query_features(np.concatenate(chunks), int(mode), invert)
    assert len(want_t) > 100
    got_roots, got_kept = roots_and_kept()
    assert np.array_equal(got_roots, np.unique(want_t[:, 0])) and got_kept == len(want_t)
    for k in (0, 1):  # one more chunk per slot, of no rows
        batch[k].sync()
        store.wait_staging(k)
        store.staging(k)[:] = world.pool[:chunk_rows]  # (rows in the buffer, none of them appended)
        store.append(k, 0)
        batch[k].set_regions_store(store, k, 0, 0)
        batch[k].run(mode, invert, ROOTS_PASS | engine.OUT_BITMAP_KEEP)
    again_roots, again_kept = roots_and_kept()
    assert np.array_equal(again_roots, got_roots) and again_kept == got_kept
    for b in batch:
        b.close()
    store.close()


# ---------------------------------------------------------------------------------------------- sub-ranges of an append
def _check_subranges(world, store, k, appended, batch_store, batch_host):
    """set_regions_store(first, m) over the last append from buffer k == set_regions(appended[first:first + m]), every output."""
    n = len(appended)
    for first in (1, 3, 5, n - 1):
        for m in sorted({1, n - first}):
            for mode in OverlapMode:
                batch_store.set_regions_store(store, k, first, m)
                batch_store.run(mode, False, EVERYTHING)
                batch_host.set_regions(appended[first:first + m])
                batch_host.run(mode, False, EVERYTHING)
                batch_store.wait()
                batch_host.wait()
                _assert_same_outputs(batch_store, batch_host, (first, m, mode))
            want_t, want_c = world.oix.query_features(appended[first:first + m], int(OverlapMode.Overlap), False)
            assert np.array_equal(batch_store.counts(), want_c) and np.array_equal(_sorted_rows(batch_store.triples()), _sorted_rows(want_t))
    for first, m in ((0, n + 1), (1, n), (n, 1), (n + 1, 0)):
        with pytest.raises(E):
            batch_store.set_regions_store(store, k, first, m)


@pytest.mark.parametrize("k", [0, 1])
def test_subranges_of_a_ring_slot(world, k):
    """A batch may take rows [first, first + m) of an append: the rows then start 12, 36 or 60 bytes past a 16-byte boundary
    (the pair kernels' 16-byte loads take their element-wise path), and in slot 1 behind chunk_rows other rows."""
    chunk_rows, n = 300, 211
    store = engine.RegionStore(0, chunk_rows, False)
    bs, bh = engine.QueryBatch(world.ix, chunk_rows), engine.QueryBatch(world.ix, chunk_rows)
    for kk in (0, 1):  # both slots hold rows; slot 1 - k holds other ones
        store.staging(kk)[:n] = _take(world.pool, 1000 + 2000 * (kk != k), n)
        store.append(kk, n)
    _check_subranges(world, store, k, _take(world.pool, 1000, n), bs, bh)
    bs.close(), bh.close(), store.close()


def test_subranges_of_the_last_append_to_a_keep_all_store(world):
    """keep_all: the last append starts behind all rows before it (here 12 * 158 bytes in: not a 16-byte boundary either)."""
    chunk_rows, sizes = 128, (101, 57, 83)
    store = engine.RegionStore(sum(sizes), chunk_rows, True)
    bs, bh = engine.QueryBatch(world.ix, chunk_rows), engine.QueryBatch(world.ix, chunk_rows)
    at = 0
    for i, n in enumerate(sizes):
        k = i & 1
        store.wait_staging(k)
        store.staging(k)[:n] = _take(world.pool, 3000 + at, n)
        store.append(k, n)
        at += n
    assert store.rows() == sum(sizes)
    _check_subranges(world, store, 0, _take(world.pool, 3000 + sizes[0] + sizes[1], sizes[2]), bs, bh)
    _check_subranges(world, store, 1, _take(world.pool, 3000 + sizes[0], sizes[1]), bs, bh)  # (buffer 1's last append: the middle one)
    bs.close(), bh.close(), store.close()


# ---------------------------------------------------------------------------------------------- append_parts
def _lines_of(world):
    """A line per root, and lines over the GAP row: a gap row that reached the device flips them."""
    co = world.roots["chr_offsets"]
    chr_of = np.repeat(np.arange(len(co) - 1), np.diff(co)).astype(np.uint32)
    seq = np.concatenate([chr_of, [2, 2, 2]]).astype(np.uint32)
    s = np.concatenate([world.roots["start"] + 1, [GAP[1], GAP[1] + 5, 1]]).astype(np.uint32)
    e = np.concatenate([world.roots["end"], [GAP[2], GAP[1] + 9, 3]]).astype(np.uint32)
    return seq, s, e


def _oracle_keep(seq, s, e, regions, n_seq, mode):
    """gff_line_overlaps_queries (commands/intersect.rs:500-521) line by line through the oracle's predicate."""
    order = np.argsort(regions[:, 0], kind="stable")
    r = regions[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(r[:, 0], minlength=n_seq))])
    out = np.zeros(len(seq), dtype=bool)
    for i in range(len(seq)):
        c = int(seq[i])
        if c >= n_seq or off[c + 1] == off[c]:
            continue
        out[i] = ob.line_predicate(int(s[i]), int(e[i]), r[off[c]:off[c + 1], 1], r[off[c]:off[c + 1], 2], int(mode))
    return out


PIECES = [(300, 40), (100, 0), (20, 33), (512 - 29, 29), (350, 1)]  # (first staging row, rows): out of order, gaps, an empty one, the buffer's last row


def _stage_pieces(store, k, world, seed_at):
    """Fills buffer k with GAP rows and the pieces' rows; returns the rows in piece order."""
    stage = store.staging(k)
    stage[:] = GAP
    parts, at = [], seed_at
    for first, n in PIECES:
        stage[first:first + n] = _take(world.pool, at, n)
        parts.append(_take(world.pool, at, n))
        at += n
    return np.concatenate(parts)


@pytest.mark.parametrize("k", [0, 1])
def test_append_parts_gathers_the_pieces_in_the_order_given(world, k):
    chunk_rows = 512
    store = engine.RegionStore(0, chunk_rows, False)
    bs, bh = engine.QueryBatch(world.ix, chunk_rows), engine.QueryBatch(world.ix, chunk_rows)
    concat = _stage_pieces(store, k, world, 500)
    store.append_parts(k, [f for f, _ in PIECES], [n for _, n in PIECES])
    for mode in OverlapMode:
        bs.set_regions_store(store, k, 0, len(concat))
        bs.run(mode, False, PAIRS)
        bh.set_regions(concat)
        bh.run(mode, False, PAIRS)
        bs.wait()
        bh.wait()
        assert np.array_equal(bs.counts(), bh.counts()), mode  # (per query, in input order)
        assert _assert_pairs_pass(bs, world.oix, concat, mode, False, mode) > 0
    with pytest.raises(E):  # the rows after the last piece's are not part of the append
        bs.set_regions_store(store, k, 0, len(concat) + 1)
    # a piece outside the buffer; pieces that are inside it but too many rows together: refused, and the store works on
    for first, rows in (([0, chunk_rows - 3], [5, 4]), ([chunk_rows + 1], [0]), ([0, 0], [300, 300])):
        with pytest.raises(E):
            store.append_parts(k, first, rows)
    store.wait_staging(k)
    rows = _take(world.pool, 77, 100)
    store.staging(k)[:100] = rows
    store.append_parts(k, [0], [100])
    bs.set_regions_store(store, k, 0, 100)
    bs.run(OverlapMode.Overlap, False, PAIRS)
    bs.wait()
    _assert_pairs_pass(bs, world.oix, rows, OverlapMode.Overlap, False, "after the refusals")
    bs.close(), bh.close(), store.close()


def test_append_parts_to_a_keep_all_store_seen_through_join_b(world):
    chunk_rows = 512
    store = engine.RegionStore(2000, chunk_rows, True)
    head = _take(world.pool, 4000, 131)
    store.staging(0)[:131] = head
    store.append(0, 131)
    concat = _stage_pieces(store, 1, world, 4500)
    store.append_parts(1, [f for f, _ in PIECES], [n for _, n in PIECES])
    tail = _take(world.pool, 5000, 9)
    store.wait_staging(0)
    store.staging(0)[:] = GAP
    store.staging(0)[3:12] = tail
    store.append_parts(0, [3], [9])
    all_rows = np.concatenate([head, concat, tail])
    assert store.rows() == len(all_rows)
    seq, s, e = _lines_of(world)
    lt = engine.LineTable(seq, s, e)
    for mode in OverlapMode:
        got = lt.test_store(store, N_SEQ, mode)
        assert np.array_equal(got, lt.test(all_rows, N_SEQ, mode)), mode
        assert np.array_equal(got, _oracle_keep(seq, s, e, all_rows, N_SEQ, mode)), mode
        assert not got[-3:].any() and (got.any() or mode != OverlapMode.Overlap)  # (no region on the rootless seqid: no GAP row came along)
    lt.close(), store.close()


# ---------------------------------------------------------------------------------------------- keep_all store -> Join B, union
KEEP_SIZES = (64, 0, 17, 64, 5)  # five appends to a store of 64-row chunks


def _fill_keep_all(store, chunks):
    for i, rows in enumerate(chunks):
        k = i & 1
        store.wait_staging(k)
        store.staging(k)[:] = GAP
        store.staging(k)[:len(rows)] = rows
        store.append(k, len(rows))
        yield i, k, rows


@pytest.mark.parametrize("seed", range(3))
def test_keep_all_store_feeds_join_b(seed):
    """Small coordinates, so that every clause of the line predicate fires; a fifth of the rows have start > end, a tenth are
    zero-length.  Lines as in test_join_b_gpu.py::test_random_small_coordinates_all_modes."""
    rng = np.random.default_rng(100 + seed)
    n_seq, n_lines, span = 4, 3000, int(rng.choice([12, 60, 1000]))
    seq = rng.integers(0, n_seq + 1, n_lines).astype(np.uint32)  # n_seq == "unknown seqid" lines
    seq[rng.random(n_lines) < 0.05] = engine.LineTable.NO_SEQ
    s = rng.integers(0, span, n_lines).astype(np.uint32)
    e = rng.integers(0, span, n_lines).astype(np.uint32)
    nq = sum(KEEP_SIZES)
    a, w = rng.integers(1, span, nq), rng.integers(1, max(2, span // 3), nq)
    kind = rng.random(nq)
    end = np.where(kind < 0.2, a - np.minimum(a, w), np.where(kind < 0.3, a, a + w))  # start > end, start == end, start < end
    all_rows = np.stack([rng.integers(0, n_seq - 1, nq), a, end], axis=1).astype(np.uint32)  # seqid n_seq - 1 never has a region
    assert (all_rows[:, 1] > all_rows[:, 2]).any() and (all_rows[:, 1] == all_rows[:, 2]).any()
    store = engine.RegionStore(nq, 64, True)
    cuts = np.cumsum((0,) + KEEP_SIZES)
    for i, k, rows in _fill_keep_all(store, [all_rows[cuts[i]:cuts[i + 1]] for i in range(len(KEEP_SIZES))]):
        assert store.rows() == cuts[i + 1]
    assert store.rows() == nq
    lt = engine.LineTable(seq, s, e)
    for mode in OverlapMode:
        got = lt.test_store(store, n_seq, mode)
        assert np.array_equal(got, lt.test(all_rows, n_seq, mode)), mode
        assert np.array_equal(got, _oracle_keep(seq, s, e, all_rows, n_seq, mode)), mode
    lt.close(), store.close()


def test_keep_all_store_feeds_the_union(world):
    """add_store over every chunk as it is appended, one chunk in two halves (first > 0): the spans of add(all rows).  The union
    takes rows with start < end only (it refuses others from either source: see the end), so this store holds such rows."""
    pool = world.pool[world.pool[:, 1] < world.pool[:, 2]]
    cuts = np.cumsum((0,) + KEEP_SIZES)
    all_rows = pool[200:200 + cuts[-1]]
    store = engine.RegionStore(cuts[-1], 64, True)
    u = engine.RegionUnion(N_SEQ)
    for i, k, rows in _fill_keep_all(store, [all_rows[cuts[i]:cuts[i + 1]] for i in range(len(KEEP_SIZES))]):
        if i == 3:
            u.add_store(store, k, 0, 23)
            u.add_store(store, k, 23, len(rows) - 23)
        else:
            u.add_store(store, k, 0, len(rows))
    with pytest.raises(E):
        u.add_store(store, 0, 1, KEEP_SIZES[-1])  # beyond the last append from buffer 0
    u.finish()
    want = engine.RegionUnion(N_SEQ)
    want.add(all_rows)
    want.finish()
    assert want.n_spans > 20
    for g, w, name in zip(u.spans(), want.spans(), ("u_off", "us", "ue", "pb")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    u.close(), want.close()
    # a zero-length row: refused from the store as from the host
    store2 = engine.RegionStore(0, 64, False)
    store2.staging(0)[:2] = [[0, 5, 9], [1, 7, 7]]
    store2.append(0, 2)
    bad = engine.RegionUnion(N_SEQ)
    with pytest.raises(E) as ei:
        bad.add_store(store2, 0, 0, 2)
        bad.finish()
    assert ei.value.code == -1
    bad.close(), store2.close(), store.close()


# ---------------------------------------------------------------------------------------------- width sample per sub-range
def _width_rows(n_half, seed):
    narrow = synth.synth_bed(n_half, seed=seed, chroms=synth.SMALL2, width=(1, 3000))
    wide = synth.synth_bed(n_half, seed=seed + 1, chroms=synth.SMALL2, width=(20000, 600000))
    return narrow, wide


def _assert_forms(wide_world, store, b, device_rows, ranges):
    """AUTO in overlap mode over sub-ranges of the append in slot 0: the form taken and the pairs."""
    for first, m, want_wide in ranges:
        b.set_regions_store(store, 0, first, m)
        b.run(OverlapMode.Overlap, False, PAIRS, engine.STRATEGY_AUTO)
        assert b.wide_form is want_wide, (first, m)
        b.wait()
        assert _assert_pairs_pass(b, wide_world.oix, device_rows[first:first + m], OverlapMode.Overlap, False, (first, m)) > 0


def test_width_sample_counts_the_rows_a_batch_takes(wide_world):
    """AUTO's prior is a sample of the chunk's rows taken at the append; a batch that takes a sub-range counts the sampled rows
    inside it only.  400 narrow rows, then 400 rows wider than a window line answers."""
    narrow, wide = _width_rows(400, 41)
    store = engine.RegionStore(0, 800, False)
    b = engine.QueryBatch(wide_world.ix, 800)
    stage = store.staging(0)
    stage[:400], stage[400:] = narrow, wide
    store.append(0, 800)
    _assert_forms(wide_world, store, b, np.concatenate([narrow, wide]), [(0, 400, False), (400, 400, True), (0, 800, True)])
    # the same buffer as two parts, wide rows first: the answers are mirrored
    b.sync()
    store.wait_staging(0)
    store.append_parts(0, [400, 0], [400, 400])
    _assert_forms(wide_world, store, b, np.concatenate([wide, narrow]), [(0, 400, True), (400, 400, False), (0, 800, True)])
    # ... and with the wide rows first in the BUFFER, the narrow ones first on the device: a sampled row is filed under the row
    # of the chunk it becomes, not the one of the buffer or of its part
    b.sync()
    store.wait_staging(0)
    stage[:400], stage[400:] = wide, narrow
    store.append_parts(0, [400, 0], [400, 400])
    _assert_forms(wide_world, store, b, np.concatenate([narrow, wide]), [(0, 400, False), (400, 400, True), (0, 800, True)])
    b.close(), store.close()


def test_width_sample_of_every_fourth_row(wide_world):
    """16 384 rows: the sample takes every fourth row of each part."""
    narrow, wide = _width_rows(8192, 43)
    store = engine.RegionStore(0, 16384, False)
    b = engine.QueryBatch(wide_world.ix, 16384)
    stage = store.staging(0)
    stage[:8192], stage[8192:] = narrow, wide
    store.append(0, 16384)
    _assert_forms(wide_world, store, b, np.concatenate([narrow, wide]), [(0, 8192, False), (8192, 8192, True)])
    b.sync()
    store.wait_staging(0)
    store.append_parts(0, [8192, 0], [8192, 8192])
    _assert_forms(wide_world, store, b, np.concatenate([wide, narrow]), [(0, 8192, True), (8192, 8192, False)])
    b.sync()
    store.wait_staging(0)
    stage[:8192], stage[8192:] = wide, narrow
    store.append_parts(0, [8192, 0], [8192, 8192])
    _assert_forms(wide_world, store, b, np.concatenate([narrow, wide]), [(0, 8192, False), (8192, 8192, True)])
    b.close(), store.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_store_usable(world):
    """Argument checks that return before any device work; after each, a good append and run still equal the oracle."""
    with pytest.raises(E):
        engine.RegionStore(0, 0, False)
    chunk_rows = 100
    ring = engine.RegionStore(0, chunk_rows, False)
    full = engine.RegionStore(150, chunk_rows, True)
    big, small = engine.QueryBatch(world.ix, chunk_rows), engine.QueryBatch(world.ix, 40)
    seq, s, e = _lines_of(world)
    lt = engine.LineTable(seq, s, e)
    rows = _take(world.pool, 900, 90)

    def good(store, k):
        store.wait_staging(k)
        store.staging(k)[:90] = rows
        store.append(k, 90)
        for b, n in ((big, 90), (small, 40)):
            b.set_regions_store(store, k, 0, n)
            b.run(OverlapMode.Overlap, False, PAIRS)
            b.wait()
            _assert_pairs_pass(b, world.oix, rows[:n], OverlapMode.Overlap, False, "after a refusal")

    good(ring, 0)
    with pytest.raises(ValueError):
        ring.staging(2)
    for call in (lambda: ring.wait_staging(2), lambda: ring.append(2, 1), lambda: ring.append_parts(2, [0], [1]),
                 lambda: big.set_regions_store(ring, 2, 0, 1)):
        with pytest.raises(E):  # k == 2
            call()
        good(ring, 1)
    with pytest.raises(E):  # n_rows > chunk_rows
        ring.append(0, chunk_rows + 1)
    good(ring, 0)
    with pytest.raises(E):  # more rows than the batch holds
        small.set_regions_store(ring, 0, 0, 41)
    good(ring, 0)
    with pytest.raises(E):  # Join B reads a keep_all store
        lt.test_store(ring, N_SEQ, OverlapMode.Overlap)
    good(ring, 1)
    good(full, 0)  # 90 of 150 rows
    assert full.rows() == 90
    with pytest.raises(E):  # a full keep_all store: 90 + 61 > 150
        full.append(1, 61)
    assert full.rows() == 90
    full.staging(1)[:60] = rows[:60]
    full.append(1, 60)
    assert full.rows() == 150
    with pytest.raises(E):
        full.append(0, 1)
    both = np.concatenate([rows, rows[:60]])
    assert np.array_equal(lt.test_store(full, N_SEQ, OverlapMode.Overlap), _oracle_keep(seq, s, e, both, N_SEQ, OverlapMode.Overlap))
    big.set_regions_store(full, 1, 0, 60)
    big.run(OverlapMode.Overlap, False, PAIRS)
    big.wait()
    _assert_pairs_pass(big, world.oix, rows[:60], OverlapMode.Overlap, False, "the full store's last append")
    lt.close(), big.close(), small.close(), ring.close(), full.close()


# ---------------------------------------------------------------------------------------------- the slot check of the seven consumers
def test_every_consumer_refuses_rows_beyond_the_last_append(world):
    """Four rows are appended from buffer 0.  Every entry point that reads a slot refuses first = 2^64 - 1 with two rows (the
    sum wraps to 1) and first = 5 with none, with GFFX_E_INVALID and before anything is launched; the same call over the
    four rows then gives what the object gives for the rows handed over from the host."""
    pool = world.pool[world.pool[:, 1] < world.pool[:, 2]]
    rows = np.ascontiguousarray(pool[40:44])
    store = engine.RegionStore(0, 16, False)
    store.staging(0)[:4] = rows
    store.append(0, 4)
    seg = (rows[:, 0], rows[:, 1], rows[:, 2] + 50)  # the pileup's segments: the rows themselves, a little longer

    def refused(call):
        for first, n in ((2 ** 64 - 1, 2), (5, 0)):
            with pytest.raises(E) as ei:
                call(first, n)
            assert ei.value.code == -1 and "rows beyond the last append" in str(ei.value), (first, n)

    def same(got, want):
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))

    b = engine.QueryBatch(world.ix, 16)
    refused(lambda f, n: b.set_regions_store(store, 0, f, n))
    b.set_regions_store(store, 0, 0, 4)
    b.run(OverlapMode.Overlap, False, PAIRS)
    b.wait()
    _assert_pairs_pass(b, world.oix, rows, OverlapMode.Overlap, False, "after the refusals")
    b.close()

    u, want = engine.RegionUnion(N_SEQ), engine.RegionUnion(N_SEQ)
    refused(lambda f, n: u.add_store(store, 0, f, n))
    u.add_store(store, 0, 0, 4), u.finish()
    want.add(rows), want.finish()
    assert u.n_spans > 0
    same(tuple(u.spans()), tuple(want.spans()))
    u.close(), want.close()

    p, want = engine.Pileup(N_SEQ, *seg), engine.Pileup(N_SEQ, *seg)
    refused(lambda f, n: p.add_store(store, 0, f, n))
    p.add_store(store, 0, 0, 4), want.add(rows)
    assert p.bases().sum() > 0
    same(p.bases(), want.bases())
    p.close(), want.close()

    d, want = engine.DepthProfile(N_SEQ), engine.DepthProfile(N_SEQ)
    refused(lambda f, n: d.add_store(store, 0, f, n))
    d.add_store(store, 0, 0, 4), d.finish()
    want.add(rows), want.finish()
    assert d.n_points > 0
    same(tuple(d.points()), tuple(want.points()))
    d.close(), want.close()

    c = engine.Closest(world.ix, 16)
    want = c.run(rows)
    refused(lambda f, n: c.run_store(store, 0, f, n))
    same(tuple(c.run_store(store, 0, 0, 4)), tuple(want))
    c.close()

    m = engine.ClassMap(N_SEQ, 2)
    m.add_rows(np.array([[0, 0, 100, 60000], [1, 1, 5, 900000], [1, 0, 30000, 200000]], dtype=np.uint32))
    m.finish()
    want = m.run(rows)
    refused(lambda f, n: m.run_store(store, 0, f, n))
    same(tuple(m.run_store(store, 0, 0, 4)), tuple(want))
    seq_len = np.full(N_SEQ, 1 << 28, dtype=np.uint32)
    m.perm_begin(seq_len, 3, seed=7)
    m.perm_run(rows)
    want = m.perm_totals()
    m.perm_begin(seq_len, 3, seed=7)
    refused(lambda f, n: m.perm_run_store(store, 0, f, n))
    m.perm_run_store(store, 0, 0, 4)
    got = m.perm_totals()
    assert got[2] == want[2]
    same(got[:2], want[:2])
    m.close(), store.close()
