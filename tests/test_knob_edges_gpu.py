"""Join A at the edges of the batch's launch-shape knobs (kBatchKnobs, engine_private.hpp): a grid of one block, a grid above the
slot count, chunk boundaries of the partitioned strategy, the direct strategy's block sums filling the host status buffer, root
slabs regrown between GFFX_OUT_BITMAP_KEEP passes, group launches on grids smaller than the group, and what AUTO resolves to under
GFFX_HIP_AUTO_STRATEGY.  Every pass is compared with the oracle (tests/_join_a_parity.py); results never depend on a knob.
"""
import numpy as np
import pytest

from gffx_amd import engine, synth
from gffx_amd.engine import OverlapMode
from oracle import binding as ob

from _join_a_parity import _check, _sorted_rows

pytestmark = pytest.mark.gpu

PART_CHUNK = 4096  # kPartChunk: sub_cap of a batch on an index of >= 16 tiles under a 1 MB budget
MODES_INV = [(m, inv) for m in OverlapMode for inv in (False, True)]
SORTED, DIRECT, FUSED, WINDOWS = engine.STRATEGY_SORTED, engine.STRATEGY_DIRECT, engine.STRATEGY_FUSED, engine.STRATEGY_WINDOWS
# the kernel that only a strategy launches (profiling: kernel_ms)
SIGNATURE = {DIRECT: engine.K_JOIN_COUNT, SORTED: engine.K_SORT, FUSED: engine.K_FUSED_DIRECT}


class _Ix:
    def __init__(self, roots):
        self.roots = roots
        co, s, e, f = roots["chr_offsets"], roots["start"], roots["end"], roots["fid"]
        self.ix = engine.TreeIndexData.from_roots(co, s, e, f)
        self.oix = ob.OracleIndex.from_roots(co, s, e, f)

    def check(self, regions, mode, invert, **kw):
        return _check(self.roots, regions, mode, invert, ix=self.ix, oix=self.oix, **kw)

    def close(self):
        self.ix.close()


def _dense_roots(n_chr=20, span=5000, per=300, seed=0):
    """small dense coordinates on many seqids (>= one tile each): deep nesting, ties, hundreds of hits per region"""
    rng = np.random.default_rng(seed)
    co = np.arange(n_chr + 1, dtype=np.uint32) * per
    start = np.concatenate([np.sort(rng.integers(0, span, per)) for _ in range(n_chr)]).astype(np.uint32)
    end = (start + rng.integers(1, span // 10, len(start))).astype(np.uint32)
    return {"chr_offsets": co, "start": start, "end": end, "fid": rng.permutation(len(start)).astype(np.uint32) * 3}


def _dense_regions(n, seed, n_chr=20, span=5000):
    rng = np.random.default_rng(seed)
    qs = rng.integers(0, span + 5, n)
    qe = qs + rng.integers(-3, 400, n)  # includes qs >= qe rows
    return np.stack([rng.integers(0, n_chr, n), qs, np.maximum(qe, 0)], axis=1).astype(np.uint32)


@pytest.fixture(scope="module")
def gencode():
    i = _Ix(synth.gencode_like_roots(20000, seed=61))  # 25 seqids: >= 25 tiles
    yield i
    i.close()


@pytest.fixture(scope="module")
def dense():
    i = _Ix(_dense_roots())
    yield i
    i.close()


def _gencode_regions(ix, n, seed, width=(100, 10000)):
    return synth.synth_bed(n, seed=seed, width=width, edge_frac=0.02, roots=ix.roots)


def _regions(ixw, kind, n, seed):
    return _gencode_regions(ixw, n, seed) if kind == "gencode" else _dense_regions(n, seed)


def _launches(b, kernel_id):
    return b.kernel_ms(kernel_id)[1]


def _pairs_check(b, oix, regions, mode, invert, offsets=None):
    """a waited pass with counts + root_fids (+ per-region offsets, or the given segment starts) == the oracle's, region by region"""
    want_t, want_c = oix.query_features(regions, int(mode), invert)
    c = b.counts()
    assert np.array_equal(c, want_c)
    assert b.total_hits == len(want_t)
    wc = want_c.astype(np.int64)
    off = (b.offsets()[:-1] if offsets is None else offsets).astype(np.int64)
    qid = np.repeat(np.arange(len(regions), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    f = b.fids()
    got = np.stack([qid, f[off[qid] + within].astype(np.int64)], axis=1)
    by_chr = np.argsort(regions[:, 0], kind="stable")  # the oracle walks seqid after seqid, regions in input order
    want = np.stack([np.repeat(by_chr, wc[by_chr]), want_t[:, 0].astype(np.int64)], axis=1)
    order = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(order(got), order(want))
    return want_t


# ---------------------------------------------------------------------------------------------------- partitioned strategy: chunks


@pytest.mark.parametrize("kind", ["gencode", "dense"])
@pytest.mark.parametrize("nq", [1, 4095, 4096, 4097, 3 * 4096 + 1, 100_000])
def test_partition_budget_chunks(request, kind, nq):
    """GFFX_HIP_PARTITION_BUDGET_MB=1: sub_cap = kPartChunk, a pass is ceil(nq / 4096) partition + join pairs (q0 > 0, the cursor
    sets alternating inside the pass, the pair cursor carried across chunks, k_unpermute over all of them)"""
    if kind == "dense" and nq == 100_000:
        nq = 30_000  # (hundreds of pairs per region)
    ixw = request.getfixturevalue(kind)
    regions = _regions(ixw, kind, nq, seed=100 + nq % 1000)
    b = engine.QueryBatch(ixw.ix, nq)
    b.set_option("PARTITION_BUDGET_MB", 1)
    b.reserve_hits(len(ixw.oix.query_features(regions, int(OverlapMode.Overlap), False)[0]))  # (no capacity replay: it re-runs every chunk)
    b.set_regions(regions)
    b.set_profiling(True)
    b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_OFFSETS, SORTED)
    b.wait()
    assert _launches(b, engine.K_SORT) == (nq + PART_CHUNK - 1) // PART_CHUNK  # the chunking this test is about
    _pairs_check(b, ixw.oix, regions, OverlapMode.Overlap, False)
    b.close()
    for i, (mode, inv) in enumerate(MODES_INV):
        ixw.check(regions, mode, inv, soa=bool(i & 1), strategy=SORTED, knobs={"PARTITION_BUDGET_MB": 1})


@pytest.mark.parametrize("mode", list(OverlapMode))
def test_partition_emit_order_records_across_chunks(gencode, mode):
    regions = _gencode_regions(gencode, 100_000, seed=7)
    want_t, want_c = gencode.oix.query_features(regions, int(mode), False)
    b = engine.QueryBatch(gencode.ix, len(regions))
    b.set_option("PARTITION_BUDGET_MB", 1)
    b.set_regions(regions)
    for _ in range(3):  # an odd chunk count (25) per pass: the cursor sets alternate across passes as well
        b.run(mode, False, engine.OUT_FIDS | engine.OUT_OFFSETS | engine.OUT_EMIT_ORDER, SORTED)
        b.wait()
        assert b.total_hits == len(want_t)
        rows, cnt, off = b.query_records()
        assert np.array_equal(np.sort(rows), np.arange(len(regions), dtype=np.uint32))
        assert np.array_equal(cnt, want_c[rows])
        fids = b.fids()
        nz = cnt > 0  # the segments tile [0, pairs)
        lo, hi = off[nz].astype(np.int64), off[nz].astype(np.int64) + cnt[nz]
        o = np.argsort(lo)
        assert len(lo) == 0 or (lo[o][0] == 0 and hi[o][-1] == len(want_t) and np.array_equal(hi[o][:-1], lo[o][1:]))
        seg_of_row = off[np.argsort(rows)]
        for qi in np.random.default_rng(2).choice(len(regions), size=200, replace=False):
            one_t, _ = gencode.oix.query_features(regions[qi:qi + 1], int(mode), False)
            assert np.array_equal(np.sort(fids[int(seg_of_row[qi]):int(seg_of_row[qi]) + int(want_c[qi])]), np.sort(one_t[:, 0]))
        assert np.array_equal(b.counts(), want_c)
        assert np.array_equal(b.offsets()[:-1][rows], off)
    b.close()


@pytest.mark.parametrize("kind,nq", [("gencode", 100_000), ("dense", 3 * 4096 + 1), ("dense", 4097)])
def test_partition_capacity_replay_across_chunks(request, kind, nq):
    """reserve_hits(1024): every pass overflows its pair buffers and the wait replays ALL chunks"""
    ixw = request.getfixturevalue(kind)
    regions = _regions(ixw, kind, nq, seed=300 + nq % 97)
    for mode, inv in [(OverlapMode.Overlap, False), (OverlapMode.Contained, True), (OverlapMode.ContainsRegion, False)]:
        ixw.check(regions, mode, inv, soa=inv, strategy=SORTED, knobs={"PARTITION_BUDGET_MB": 1}, reserve=1024)


def test_partition_reused_batch_odd_and_even_chunk_counts(gencode, dense):
    """one batch, region sets of 3, 4, 5, 2, 1 chunks, the fused and windows strategies between the partitioned passes: a cursor
    phase left stale by an odd chunk count, or by another strategy's pass, would show"""
    for ixw, kind in ((gencode, "gencode"), (dense, "dense")):
        b = engine.QueryBatch(ixw.ix, 5 * PART_CHUNK)
        b.set_option("PARTITION_BUDGET_MB", 1)
        b.set_profiling(True)
        for step, n in enumerate([2 * 4096 + 1, 4 * 4096, 5 * 4096, 4097, 1, 3 * 4096 + 5]):
            regions = _regions(ixw, kind, n, seed=400 + step)
            b.set_regions(regions)
            mode = OverlapMode(step % 3)
            b.reserve_hits(len(ixw.oix.query_features(regions, int(mode), False)[0]))  # (no capacity replay: it re-runs every chunk)
            for strategy in (SORTED, FUSED if step % 2 else WINDOWS, SORTED):
                b.reset_profile()
                b.run(mode, False, engine.OUT_FIDS | engine.OUT_OFFSETS, strategy)
                b.wait()
                if strategy == SORTED:
                    assert _launches(b, engine.K_SORT) == (n + PART_CHUNK - 1) // PART_CHUNK
                _pairs_check(b, ixw.oix, regions, mode, False)
        b.close()


def test_partition_many_seqids_chunks():
    """4000 scaffolds (>= 4000 tiles: the partition kernel's LDS opt-in) cut into chunks of 4096 regions"""
    chroms = [("scaf%d" % i, 50_000 + 13 * i) for i in range(4000)]
    ixw = _Ix(synth.gencode_like_roots(12000, seed=8, chroms=chroms))
    regions = synth.synth_bed(30000, seed=9, chroms=chroms, width=(10, 5000), edge_frac=0.05, roots=ixw.roots)
    for i, (mode, inv) in enumerate(MODES_INV):
        ixw.check(regions, mode, inv, soa=bool(i & 1), strategy=SORTED, knobs={"PARTITION_BUDGET_MB": 1})
    ixw.close()


def test_partition_budget_changed_after_the_first_pass(gencode):
    """partition_prepare sizes sub_cap on the batch's FIRST partitioned pass; a later set_option does not resize it.  Whatever the
    chunking then is, the passes stay exact."""
    regions = _gencode_regions(gencode, 20_000, seed=11)
    for first, later in ((None, 1), (1, 12 * 1024)):
        b = engine.QueryBatch(gencode.ix, len(regions))
        if first:
            b.set_option("PARTITION_BUDGET_MB", first)
        b.set_regions(regions)
        for i, mode in enumerate(OverlapMode):
            b.run(mode, False, engine.OUT_FIDS | engine.OUT_OFFSETS, SORTED)
            b.wait()
            _pairs_check(b, gencode.oix, regions, mode, False)
            if i == 0:
                b.set_option("PARTITION_BUDGET_MB", later)
        b.close()


@pytest.mark.parametrize("budget", [None, 1])
@pytest.mark.parametrize("join_blocks", [1, 3, 65535])
def test_join_blocks(gencode, dense, join_blocks, budget):
    """GFFX_HIP_JOIN_BLOCKS: k_tile_join at grid 1 (one block walks a whole sub-batch), 3, and far above the 512 default"""
    knobs = {"JOIN_BLOCKS": join_blocks}
    if budget:
        knobs["PARTITION_BUDGET_MB"] = budget
    regions = _gencode_regions(gencode, 20_000, seed=500 + join_blocks)
    for i, (mode, inv) in enumerate(MODES_INV):
        gencode.check(regions, mode, inv, soa=bool(i & 1), strategy=SORTED, knobs=knobs)
    dregions = _dense_regions(9000, seed=501)
    dense.check(dregions, OverlapMode.Overlap, False, strategy=SORTED, knobs=knobs, reserve=1024)


# ---------------------------------------------------------------------------------------------------- direct strategy: block counts


@pytest.mark.parametrize("max_blocks", [1, 7])
def test_direct_max_blocks_small(gencode, dense, max_blocks):
    """GFFX_HIP_MAX_BLOCKS=1: one block walks every tile; 7: a block count that does not divide the tiles"""
    regions = _gencode_regions(gencode, 20_000 + 13, seed=600 + max_blocks)
    for i, (mode, inv) in enumerate(MODES_INV):
        gencode.check(regions, mode, inv, soa=bool(i & 1), strategy=DIRECT, knobs={"MAX_BLOCKS": max_blocks})
    dense.check(_dense_regions(5000, seed=601), OverlapMode.Contained, False, strategy=DIRECT, knobs={"MAX_BLOCKS": max_blocks})


def test_direct_max_blocks_8192():
    """GFFX_HIP_MAX_BLOCKS=8192 = kMaxBlocks with 8192 tiles of 256 regions, the last one partial: n_blocks reaches kMaxBlocks and the
    block sums fill the host status buffer to its last word"""
    nq = 8192 * 256 - 77
    ixw = _Ix(synth.gencode_like_roots(5000, seed=62))
    regions = synth.synth_bed(nq, seed=63, width=(100, 20000), edge_frac=0.001, roots=ixw.roots)
    ixw.check(regions, OverlapMode.Overlap, False, soa=True, strategy=DIRECT, knobs={"MAX_BLOCKS": 8192})
    ixw.close()


# ---------------------------------------------------------------------------------------------------- one-kernel strategies: grids


@pytest.mark.parametrize("fused_blocks", [1, 2, 65535])
def test_fused_blocks(gencode, dense, fused_blocks):
    """GFFX_HIP_FUSED_BLOCKS on the fused strategy: one block, two, and the knob's maximum (capped by the rounds); with and without
    the capacity replay"""
    knobs = {"FUSED_BLOCKS": fused_blocks}
    regions = _gencode_regions(gencode, 30_000, seed=700 + fused_blocks)
    for i, (mode, inv) in enumerate(MODES_INV):
        gencode.check(regions, mode, inv, soa=bool(i & 1), strategy=FUSED, knobs=knobs, reserve=1024 if i % 3 == 0 else 0)
    dense.check(_dense_regions(6000, seed=701), OverlapMode.Overlap, False, strategy=FUSED, knobs=knobs, reserve=1024)


@pytest.fixture(scope="module")
def small_genes():
    i = _Ix(synth.gencode_like_roots(5000, seed=64))
    yield i
    i.close()


@pytest.fixture(scope="module")
def big_regions(small_genes):
    """1.3 M regions: 635 rounds of 512-thread blocks, more than the 512 slots of the device"""
    return synth.synth_bed(1_300_000, seed=65, width=(100, 8000), edge_frac=0.002, roots=small_genes.roots)


@pytest.mark.parametrize("fused_blocks", [1, 600, 65535])
def test_windows_pair_pass_blocks_above_the_slots(small_genes, big_regions, fused_blocks):
    """GFFX_HIP_FUSED_BLOCKS on a windows pair pass: one block, and more blocks than slots (600, and the knob's maximum, which the
    rounds cap)"""
    knobs = {"FUSED_BLOCKS": fused_blocks, "WIN_THREADS": 512}
    rounds = (len(big_regions) + 2047) // 2048
    b = engine.QueryBatch(small_genes.ix, len(big_regions))
    for k, v in knobs.items():
        b.set_option(k, v)
    b.set_regions(big_regions)
    b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_SEGBASE, WINDOWS)
    b.wait()
    assert (b.block_threads, b.block_count) == (512, min(rounds, fused_blocks))
    _pairs_check(b, small_genes.oix, big_regions, OverlapMode.Overlap, False, offsets=b.offsets_from_segbase())
    b.close()
    small = big_regions[:40_000]
    for i, (mode, inv) in enumerate(MODES_INV):
        small_genes.check(small, mode, inv, soa=bool(i & 1), strategy=WINDOWS, knobs=knobs, reserve=1024 if i == 2 else 0)


def _root_pass(b, mode, inv, keep=False):
    b.run(mode, inv, engine.OUT_ROOT_BITMAP | engine.OUT_NO_COUNTS | (engine.OUT_BITMAP_KEEP if keep else 0), WINDOWS)
    b.wait()


@pytest.mark.parametrize("bitmap_blocks", [1, 3, 8192])
def test_bitmap_blocks_root_pass(gencode, bitmap_blocks):
    """GFFX_HIP_BITMAP_BLOCKS on a windows root pass (roots only, counts waived): unique roots and the pass's pair total"""
    regions = _gencode_regions(gencode, 50_000, seed=800 + bitmap_blocks)
    b = engine.QueryBatch(gencode.ix, len(regions))
    b.set_option("BITMAP_BLOCKS", bitmap_blocks)
    b.set_regions(regions)
    for mode, inv in MODES_INV:
        want_t, _ = gencode.oix.query_features(regions, int(mode), inv)
        _root_pass(b, mode, inv)
        assert np.array_equal(b.unique_roots(), np.unique(want_t[:, 0]))
        assert b.total_hits == len(want_t) and b.kept_pairs_accumulated == len(want_t)
    b.close()


@pytest.mark.parametrize("mode,inv", [(OverlapMode.Overlap, False), (OverlapMode.Contained, True)])
def test_bitmap_keep_chain_with_the_grid_changing(small_genes, big_regions, mode, inv):
    """one batch, three region sets, GFFX_OUT_BITMAP_KEEP from the second on, BITMAP_BLOCKS 64 -> 1 -> 600 between the passes: blocks
    below slab_valid OR into their slab, the others overwrite theirs, and 600 > 512 slabs regrow with a copy of the valid ones"""
    sets = [big_regions[:200_000], big_regions[200_000:250_000], big_regions]  # 98, 25, 635 rounds of 512-thread blocks
    b = engine.QueryBatch(small_genes.ix, len(big_regions))
    b.set_option("WIN_THREADS", 512)
    seen, pairs = np.zeros(0, np.uint32), 0
    for step, (regions, blocks) in enumerate(zip(sets, [64, 1, 600])):
        b.set_option("BITMAP_BLOCKS", blocks)
        b.set_regions(regions)
        _root_pass(b, mode, inv, keep=step > 0)
        want_t, _ = small_genes.oix.query_features(regions, int(mode), inv)
        seen = np.union1d(seen, want_t[:, 0])
        pairs += len(want_t)
        assert np.array_equal(b.unique_roots(), seen), step
        assert b.total_hits == len(want_t)
        assert b.kept_pairs_accumulated == pairs, step
    b.close()


# ---------------------------------------------------------------------------------------------------- group launches


@pytest.mark.parametrize("blocks", [1, 3])
def test_group_launches_on_grids_smaller_than_the_group(gencode, blocks):
    """eight batches, FUSED_BLOCKS / BITMAP_BLOCKS forced to 1 or 3 on all of them: two groups of four whose grid (one block per
    member at least) is larger than the knob; pair and root passes equal the oracle.  Then members whose knobs differ: the groups are
    refused and the passes run one by one, each on its own forced grid."""
    sizes = [20_000, 1, 9000, 4097, 30_000, 512, 12_289, 2048]
    sets = [_gencode_regions(gencode, n, seed=900 + i, width=(100, 3000)) for i, n in enumerate(sizes)]
    bs = []
    for r in sets:
        b = engine.QueryBatch(gencode.ix, len(r))
        b.set_option("WIN_WIDE", 0)  # (one form for every member, whatever a batch's sample of widths says)
        b.set_option("FUSED_BLOCKS", blocks)
        b.set_option("BITMAP_BLOCKS", blocks)
        b.set_regions(r)
        bs.append(b)
    assert engine.batches_plan(bs) == (2, 4, 2)
    for differ in (False, True):
        if differ:
            for i, b in enumerate(bs):
                b.set_option("FUSED_BLOCKS", blocks + (i % 2))
                b.set_option("BITMAP_BLOCKS", blocks + (i % 2))
        for mode, inv in [(OverlapMode.Overlap, False), (OverlapMode.ContainsRegion, True)]:
            for flags in (engine.OUT_FIDS | engine.OUT_SEGBASE, engine.OUT_FIDS | engine.OUT_OFFSETS):
                engine.run_batches(bs, mode, inv, flags, WINDOWS, 2 * len(bs))
                for i, (b, r) in enumerate(zip(bs, sets)):
                    b.wait()
                    if not differ:
                        assert b.block_count >= 4  # (the whole group launch's grid)
                    else:
                        assert b.block_count == min(blocks + i % 2, (len(r) + 2047) // 2048)  # (its own launch)
                    seg = b.offsets_from_segbase() if flags & engine.OUT_SEGBASE else None
                    _pairs_check(b, gencode.oix, r, mode, inv, offsets=seg)
            engine.run_batches(bs, mode, inv, engine.OUT_ROOT_BITMAP | engine.OUT_NO_COUNTS, WINDOWS)
            for b, r in zip(bs, sets):
                b.wait()
                want_t, _ = gencode.oix.query_features(r, int(mode), inv)
                assert np.array_equal(b.unique_roots(), np.unique(want_t[:, 0]))
                assert b.kept_pairs_accumulated == len(want_t)
    for b in bs:
        b.close()


# ---------------------------------------------------------------------------------------------------- AUTO_STRATEGY


def _strategy_ran(b):
    ran = [s for s, k in SIGNATURE.items() if _launches(b, k)]
    if _launches(b, engine.K_WAVE) or _launches(b, engine.K_WINDOWS):
        ran.append(WINDOWS)
    assert len(ran) == 1, ran
    return ran[0]


FLAGSETS = {
    "plain": engine.OUT_FIDS | engine.OUT_OFFSETS,
    "offsets32": engine.OUT_FIDS | engine.OUT_OFFSETS32,
    "segbase": engine.OUT_FIDS | engine.OUT_SEGBASE,
    "bitmap_keep": engine.OUT_ROOT_BITMAP | engine.OUT_BITMAP_KEEP,
    "no_counts": engine.OUT_ROOT_BITMAP | engine.OUT_NO_COUNTS,
}


@pytest.mark.parametrize("flagset", list(FLAGSETS))
@pytest.mark.parametrize("value", [1, 2, 3, 4, 5])
def test_auto_strategy(gencode, value, flagset):
    """GFFX_HIP_AUTO_STRATEGY under STRATEGY_AUTO: 1 direct, 2 partitioned, 3 fused, 5 windows, 4 (retired) = the engine's own choice;
    OFFSETS32 / SEGBASE / BITMAP_KEEP and a root pass with its counts waived take the windows strategy whatever the knob says"""
    flags = FLAGSETS[flagset]
    regions = _gencode_regions(gencode, 30_000, seed=1000 + value, width=(100, 5000))
    first = _gencode_regions(gencode, 10_000, seed=1100 + value, width=(100, 5000))
    b = engine.QueryBatch(gencode.ix, len(regions))
    b.set_option("AUTO_STRATEGY", value)
    b.set_option("WIN_WIDE", 0)  # (AUTO's mixed form would take the windows strategy for a batch with some wide rows)
    b.set_profiling(True)
    keep = flags & engine.OUT_BITMAP_KEEP
    if keep:  # a first set of roots under the knob's strategy, the kept pass on top of it
        b.set_regions(first)
        b.run(OverlapMode.Overlap, False, engine.OUT_ROOT_BITMAP)
        b.wait()
        b.reset_profile()
    b.set_regions(regions)
    b.run(OverlapMode.Overlap, False, flags)
    b.wait()
    forced = flagset != "plain"
    want = WINDOWS if forced or value in (4, 5) else {1: DIRECT, 2: SORTED, 3: FUSED}[value]
    assert _strategy_ran(b) == want
    want_t, want_c = gencode.oix.query_features(regions, int(OverlapMode.Overlap), False)
    if flags & engine.OUT_ROOT_BITMAP:
        roots = want_t[:, 0]
        if keep:
            roots = np.concatenate([roots, gencode.oix.query_features(first, int(OverlapMode.Overlap), False)[0][:, 0]])
        assert np.array_equal(b.unique_roots(), np.unique(roots))
    elif flags & engine.OUT_OFFSETS32:
        _pairs_check(b, gencode.oix, regions, OverlapMode.Overlap, False, offsets=b.offsets32())
    elif flags & engine.OUT_SEGBASE:
        _pairs_check(b, gencode.oix, regions, OverlapMode.Overlap, False, offsets=b.offsets_from_segbase())
    else:
        _pairs_check(b, gencode.oix, regions, OverlapMode.Overlap, False)
    b.close()
    # 4 is what the engine picks without the knob
    if value == 4:
        b0 = engine.QueryBatch(gencode.ix, len(regions))
        b0.set_option("WIN_WIDE", 0)
        b0.set_profiling(True)
        b0.set_regions(regions)
        b0.run(OverlapMode.Overlap, False, flags & ~engine.OUT_BITMAP_KEEP)
        b0.wait()
        assert _strategy_ran(b0) == want
        b0.close()


def test_auto_strategy_partitioned_not_possible():
    """GFFX_HIP_AUTO_STRATEGY=2 on an index with more seqids than the partitioned strategy supports: the fused strategy serves it"""
    chroms = [("scaf%d" % i, 50_000 + 13 * i) for i in range(5000)]
    ixw = _Ix(synth.gencode_like_roots(12000, seed=8, chroms=chroms))
    regions = synth.synth_bed(20000, seed=9, chroms=chroms, width=(10, 5000), edge_frac=0.05, roots=ixw.roots)
    b = engine.QueryBatch(ixw.ix, len(regions))
    b.set_option("AUTO_STRATEGY", 2)
    b.set_profiling(True)
    b.set_regions(regions)
    for mode, inv in MODES_INV:
        b.reset_profile()
        b.run(mode, inv, engine.OUT_FIDS | engine.OUT_OFFSETS | engine.OUT_TRIPLES)
        b.wait()
        if not (mode == OverlapMode.Overlap and inv):
            assert _strategy_ran(b) == FUSED
        want_t = _pairs_check(b, ixw.oix, regions, mode, inv)
        assert np.array_equal(_sorted_rows(b.triples()), _sorted_rows(want_t))
    b.close()
    ixw.check(regions, OverlapMode.Contained, False, knobs={"AUTO_STRATEGY": 2})
    ixw.close()
