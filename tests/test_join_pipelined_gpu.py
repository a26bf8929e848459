"""k_join_pairs' round loop carries state from one round to the next: the next round's regions are requested a round
ahead and unpacked at that round's top (QAHEAD), beside the two pending rounds and the reservation in flight.  The smallest shapes
where a loop that works ahead goes wrong: one to four rounds per block at both block widths, batches a region short of, at and over
a whole round, the tail by ticket from a block's second round on, groups whose blocks start and end in different iterations, full /
overfull / synchronous rounds next to each other, rows the exact sweep answers, and a seqid out of range in a full and in a partial
round.  The passes that take the QAHEAD instantiations are the GROUP launches without per-region offsets (run_batches with OUT_FIDS |
OUT_SEGBASE: what bench.py times).  _group plans 2, 3, 4, 5 and 8 batches as ONE launch each (GFFX_HIP_GROUP = 1) and asserts the
plan; every member reports the launch's grid.  Through such launches go: one to ten rounds per block, full and partial last
rounds, overfull and synchronous rounds in both orders, the capacity replay, every mode and inversion, swept rows and bad seqids.
A lone batch's launches and the passes with offsets keep the one-step loader and are pinned at the same shapes (the tests that
call _seg_pass and _check: rounds per block, tickets).  Everything against the oracle.
Two things the API does not let a test reach.  A block without a round (lb >= n_rounds): the host gives every batch of a launch
between one block and a block per round, and an empty batch is neither launched nor grouped -- so the grids are forced BELOW the
rounds (FUSED_BLOCKS 1 and 2) and the engine's clamp is asserted.  The counts of a pass that failed with a seqid out of range: the
wait fails, the batch is not "waited", and every copy-out is refused (GFFX_E_STATE) -- that is asserted instead.
(The file's name: it was written for a software-pipelined order of the loop, which was measured and not kept -- DESIGN.md 10.000.)
"""
import numpy as np
import pytest

from gffx_amd import engine, synth
from gffx_amd.engine import OverlapMode
from oracle import binding as ob

from _join_a_parity import _check

pytestmark = pytest.mark.gpu

WINDOWS = engine.STRATEGY_WINDOWS
SEG = engine.OUT_FIDS | engine.OUT_SEGBASE
MODES_INV = [(OverlapMode.Overlap, False), (OverlapMode.Contained, False), (OverlapMode.Contained, True),
             (OverlapMode.ContainsRegion, False), (OverlapMode.ContainsRegion, True)]


class _Ix:
    def __init__(self, roots):
        self.roots = roots
        co, s, e, f = roots["chr_offsets"], roots["start"], roots["end"], roots["fid"]
        self.ix = engine.TreeIndexData.from_roots(co, s, e, f)
        self.oix = ob.OracleIndex.from_roots(co, s, e, f)

    def check(self, regions, mode, invert, **kw):
        return _check(self.roots, regions, mode, invert, ix=self.ix, oix=self.oix, strategy=WINDOWS, **kw)

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module")
def genes():
    i = _Ix(synth.gencode_like_roots(20000, seed=71))
    yield i
    i.close()


def _regions(ixw, n, seed, width=(100, 10000)):
    return synth.synth_bed(n, seed=seed, width=width, edge_frac=0.02, roots=ixw.roots)


def _seg_pass_check(b, oix, regions, mode, invert):
    """a waited OUT_FIDS | OUT_SEGBASE pass: counts, and the (region, root_fid) pairs of every region, equal the oracle's"""
    want_t, want_c = oix.query_features(regions, int(mode), invert)
    c = b.counts()
    assert np.array_equal(c, want_c)
    assert b.total_hits == len(want_t)
    wc = want_c.astype(np.int64)
    off = b.offsets_from_segbase(c).astype(np.int64)
    qid = np.repeat(np.arange(len(regions), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    got = np.stack([qid, b.fids()[off[qid] + within].astype(np.int64)], axis=1)
    by_chr = np.argsort(regions[:, 0], kind="stable")  # the oracle walks seqid after seqid, regions in input order
    want = np.stack([np.repeat(by_chr, wc[by_chr]), want_t[:, 0].astype(np.int64)], axis=1)
    order = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(order(got), order(want))


def _seg_pass(ixw, regions, mode, invert, knobs, reserve=0):
    b = engine.QueryBatch(ixw.ix, max(len(regions), 1))
    for k, v in knobs.items():
        b.set_option(k, v)
    if reserve:
        b.reserve_hits(reserve)
    b.set_regions(regions)
    b.run(mode, invert, SEG, WINDOWS)
    b.wait()
    _seg_pass_check(b, ixw.oix, regions, mode, invert)
    return b


def _group(ixw, sets, knobs, reserve=0):
    """one batch per region set, planned as ONE group launch on one stream (GFFX_HIP_GROUP = 1 on the first batch: the default, 2,
    runs fewer than four batches pass by pass and cuts more into two groups)"""
    bs = []
    for i, r in enumerate(sets):
        b = engine.QueryBatch(ixw.ix, max(len(r), 1))
        for k, v in dict(knobs, GROUP=1).items():
            b.set_option(k, v)
        if reserve:  # (a number for every member, or one per member)
            b.reserve_hits(reserve[i] if isinstance(reserve, list) else reserve)
        b.set_regions(r)
        bs.append(b)
    assert engine.batches_plan(bs) == (1, len(sets), 1)
    return bs


def _group_pass(bs, oix, sets, mode, invert, grid=None):
    """one pass over every batch, as one launch; grid: the launch's grid, which every member reports (a member that ran alone
    would report its own blocks)"""
    engine.run_batches(bs, mode, invert, SEG, WINDOWS)
    for b, r in zip(bs, sets):
        b.wait()
        if grid is not None:
            assert b.block_count == grid
        _seg_pass_check(b, oix, r, mode, invert)


def _close(bs):
    for b in bs:
        b.close()


# ------------------------------------------------------------------------------------------- prologue, epilogue: 1 .. 4 rounds per block


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_rounds_per_block(genes, threads, k):
    """nq = k 4T - 1, k 4T, k 4T + 1 on ONE block: k rounds (the last one partial), k full rounds, k + 1 (the last one a single
    region) -- one to four rounds per block; on two blocks the pipelines of neighbours end in different iterations"""
    chunk = 4 * threads
    for nq in (k * chunk - 1, k * chunk, k * chunk + 1):
        regions = _regions(genes, nq, seed=10 * k + nq % 7)
        for blocks in (1, 2):
            b = _seg_pass(genes, regions, OverlapMode.Overlap, False, {"WIN_THREADS": threads, "FUSED_BLOCKS": blocks, "WIN_WIDE": 0})
            assert (b.block_threads, b.block_count) == (threads, min(blocks, (nq + chunk - 1) // chunk))
            b.close()
    genes.check(_regions(genes, k * chunk + 1, seed=90 + k), OverlapMode.Overlap, False, soa=bool(k & 1),
                knobs={"WIN_THREADS": threads, "FUSED_BLOCKS": 1, "WIN_WIDE": 0})


@pytest.mark.parametrize("threads", [512, 1024])
def test_one_region(genes, threads):
    regions = _regions(genes, 1, seed=3)
    genes.check(regions, OverlapMode.Overlap, False, knobs={"WIN_THREADS": threads, "WIN_WIDE": 0})


@pytest.mark.parametrize("threads", [512, 1024])
def test_tail_by_ticket(genes, threads):
    """two blocks; 16 rounds = the fewest at which the engine takes the tail by ticket (eight per block), and 17; then TICKETS=2 on
    three and four rounds: every round but a block's first by ticket"""
    chunk = 4 * threads
    base = {"WIN_THREADS": threads, "FUSED_BLOCKS": 2, "WIN_WIDE": 0}
    for nq in (16 * chunk, 16 * chunk + 5):
        _seg_pass(genes, _regions(genes, nq, seed=nq % 11, width=(100, 3000)), OverlapMode.Overlap, False, base).close()
    for nq in (3 * chunk - 1, 4 * chunk + 1):
        regions = _regions(genes, nq, seed=nq % 13)
        _seg_pass(genes, regions, OverlapMode.Overlap, False, dict(base, TICKETS=2)).close()
        _seg_pass(genes, regions, OverlapMode.Contained, True, dict(base, TICKETS=2, FUSED_BLOCKS=1)).close()


# ------------------------------------------------------------------------------------------- groups of unequal batches


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("one_block_each", [True, False])
@pytest.mark.parametrize("n", [2, 5, 8])
def test_groups_of_unequal_batches(genes, n, threads, one_block_each):
    """the first n of 3 4T + 7, 2 4T, 1, 4T - 1, 20000, 4T, 3 4T and 4T + 1 regions in ONE launch.  One block per member (FUSED_BLOCKS
    1): 4, 2, 1, 1, 5 or 10, 1, 3 and 2 rounds per block side by side, last rounds that are full (2 4T, 4T, 3 4T), a region short
    of full, and a single region -- neighbouring blocks enter and leave their loops in different iterations.  Else the engine's own
    grid.  All three modes, the two invertible ones inverted."""
    chunk = 4 * threads
    sizes = [3 * chunk + 7, 2 * chunk, 1, chunk - 1, 20_000, chunk, 3 * chunk, chunk + 1][:n]
    sets = [_regions(genes, nq, seed=200 + i, width=(100, 3000)) for i, nq in enumerate(sizes)]
    knobs = {"WIN_THREADS": threads, "WIN_WIDE": 0}
    if one_block_each:
        knobs["FUSED_BLOCKS"] = 1
    bs = _group(genes, sets, knobs)
    for mode, inv in MODES_INV if one_block_each else MODES_INV[:2]:
        _group_pass(bs, genes.oix, sets, mode, inv, grid=n if one_block_each else None)
    if not one_block_each:
        assert all(b.block_count >= n and b.block_count == bs[0].block_count for b in bs)  # (one launch: at least a block per member)
    _close(bs)


def test_what_the_default_plan_makes_of_such_batches(genes):
    """GFFX_HIP_GROUP left at its default: two batches run pass by pass (lone launches), eight as two groups of four"""
    sets = [_regions(genes, nq, seed=300 + i, width=(100, 3000)) for i, nq in enumerate([2049, 4096, 1, 2047, 9000, 2048, 6144, 2050])]
    bs = []
    for r in sets:
        b = engine.QueryBatch(genes.ix, len(r))
        b.set_option("WIN_WIDE", 0)
        b.set_option("WIN_THREADS", 512)
        b.set_regions(r)
        bs.append(b)
    assert engine.batches_plan(bs[:2])[0] == 0
    assert engine.batches_plan(bs) == (2, 4, 2)
    engine.run_batches(bs, OverlapMode.Overlap, False, SEG, WINDOWS, 2 * len(bs))  # (every batch twice: the second launch reuses the first one's state)
    for b, r in zip(bs, sets):
        b.wait()
        _seg_pass_check(b, genes.oix, r, OverlapMode.Overlap, False)
    _close(bs)


# ------------------------------------------------------------------------------------------- full, overfull and synchronous rounds


def _layered_roots(per=400, span=100_000, seed=5):
    """one seqid, a few hundred overlapping roots: ~4 over every base"""
    rng = np.random.default_rng(seed)
    start = np.sort(rng.integers(0, span, per)).astype(np.uint32)
    end = (start + rng.integers(1, 2000, per)).astype(np.uint32)
    return {"chr_offsets": np.array([0, per], np.uint32), "start": start, "end": end, "fid": rng.permutation(per).astype(np.uint32) * 3}


@pytest.fixture(scope="module")
def layered():
    i = _Ix(_layered_roots())
    yield i
    i.close()


def _round_of(kind, n, rng, span=100_000):
    """n regions that keep nothing (beyond the roots), ~4 pairs each (more than one strip per wave round, less than all) or ~10 (more
    than all strips: the synchronous path)"""
    if kind == "none":
        qs = rng.integers(span + 5000, span + 50_000, n)
        w = rng.integers(1, 100, n)
    elif kind == "big":
        qs = rng.integers(2000, span - 2000, n)
        w = rng.integers(1, 20, n)
    else:
        qs = rng.integers(2000, span - 4000, n)
        w = rng.integers(1500, 2500, n)
    return np.stack([np.zeros(n, np.int64), qs, qs + w], axis=1).astype(np.uint32)


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("backwards", [False, True])
def test_overfull_and_synchronous_rounds_side_by_side(layered, threads, backwards):
    chunk = 4 * threads
    kinds = ["none", "big", "sync", "big", "none", "sync", "sync", "big", "none"]
    if backwards:
        kinds = kinds[::-1]
    rng = np.random.default_rng(17)
    regions = np.concatenate([_round_of(k, chunk, rng) for k in kinds] + [_round_of("sync", 77, rng)])
    _, want_c = layered.oix.query_features(regions, int(OverlapMode.Overlap), False)
    per_wave = np.add.reduceat(want_c.astype(np.int64), np.arange(0, len(want_c), 256))
    strip = 512 if threads == 1024 else 384
    assert (per_wave == 0).any() and ((per_wave > strip) & (per_wave <= 3 * strip)).any() and (per_wave > 3 * strip).any()
    knobs = {"WIN_THREADS": threads, "FUSED_BLOCKS": 1, "WIN_WIDE": 0}
    for mode, inv in MODES_INV[:3]:
        _seg_pass(layered, regions, mode, inv, knobs).close()
    _seg_pass(layered, regions, OverlapMode.Overlap, False, knobs, reserve=1024).close()  # (the capacity replay)
    layered.check(regions[: 3 * chunk + 9], OverlapMode.Overlap, False, knobs=dict(knobs, FUSED_BLOCKS=2), reserve=1024)
    # THE SAME ROUNDS IN ONE GROUP LAUNCH (the launches that request their regions a round ahead), one block per member: next to a
    # member that runs them the other way round and a light one -- every mode and inversion, then with pair buffers that are too
    # small (the capacity replay)
    sets = [regions, regions[::-1].copy(), np.concatenate([_round_of("none", chunk, rng), _round_of("big", 2 * chunk, rng)])]
    # (pair buffers that hold every member's pairs: a member that overflows is replayed ALONE at its wait and then reports its own grid)
    room = [len(layered.oix.query_features(r, int(OverlapMode.Overlap), False)[0]) + 4096 for r in sets]
    bs = _group(layered, sets, knobs, reserve=room)
    for mode, inv in MODES_INV:
        _group_pass(bs, layered.oix, sets, mode, inv, grid=3)
    _close(bs)
    bs = _group(layered, sets, knobs, reserve=1024)
    _group_pass(bs, layered.oix, sets, OverlapMode.Overlap, False)
    _group_pass(bs, layered.oix, sets, OverlapMode.Contained, True)
    _close(bs)


# ------------------------------------------------------------------------------------------- rows that re-read their region; bad rows


def _odd_rows(ixw, n, seed):
    """regions with empty, reversed and very wide rows (the exact sweep: they re-read their region) sprinkled in"""
    regions = _regions(ixw, n, seed=seed)
    rng = np.random.default_rng(seed)
    pick = rng.choice(n, size=max(3, n // 50), replace=False)
    for j, i in enumerate(pick):
        if j % 3 == 0:
            regions[i, 2] = regions[i, 1]  # empty
        elif j % 3 == 1:
            regions[i, 1], regions[i, 2] = regions[i, 2] + 50, regions[i, 1]  # reversed
        else:
            regions[i, 2] = regions[i, 1] + 3_000_000  # wider than any line answers
    return regions


@pytest.mark.parametrize("threads", [512, 1024])
def test_rows_the_sweep_answers_in_every_mode(genes, threads):
    chunk = 4 * threads
    regions = _odd_rows(genes, 3 * chunk + 7, seed=31)
    knobs = {"WIN_THREADS": threads, "FUSED_BLOCKS": 1, "WIN_WIDE": 0}
    for mode, inv in MODES_INV:
        _seg_pass(genes, regions, mode, inv, knobs).close()
    genes.check(regions, OverlapMode.Overlap, False, knobs=knobs, reserve=1024)


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("where", ["full", "partial"])
def test_a_seqid_out_of_range(genes, threads, where):
    """in a full round (the second of three) and in the last, partial one: the pass fails with GFFX_E_CHR_RANGE, once, and the batch
    serves the next region set exactly"""
    chunk = 4 * threads
    regions = _regions(genes, 2 * chunk + 300, seed=41)
    n_chr = len(genes.roots["chr_offsets"]) - 1
    bad = regions.copy()
    bad[chunk + 17 if where == "full" else 2 * chunk + 250, 0] = n_chr
    b = engine.QueryBatch(genes.ix, len(regions))
    for k, v in {"WIN_THREADS": threads, "FUSED_BLOCKS": 1, "WIN_WIDE": 0}.items():
        b.set_option(k, v)
    b.set_regions(bad)
    with pytest.raises(engine._ffi.GffxHipError) as ei:
        b.run(OverlapMode.Overlap, False, SEG, WINDOWS)
        b.wait()
    assert ei.value.code == -5
    with pytest.raises(engine._ffi.GffxHipError):  # (the failed pass's counts are not handed out: see the file's docstring)
        b.counts()
    b.set_regions(regions)
    b.run(OverlapMode.Overlap, False, SEG, WINDOWS)
    b.wait()
    _seg_pass_check(b, genes.oix, regions, OverlapMode.Overlap, False)
    b.close()


@pytest.mark.parametrize("threads", [512, 1024])
def test_a_group_with_swept_rows_and_seqids_out_of_range(genes, threads):
    """ONE launch for four batches, one block each: rows the sweep answers, a seqid out of range in a full round, a clean batch, a seqid
    out of range in the last, partial round.  The two bad members fail at their wait, the others are exact; then all four, clean"""
    chunk = 4 * threads
    n_chr = len(genes.roots["chr_offsets"]) - 1
    good = [_odd_rows(genes, 3 * chunk + 7, seed=51), _regions(genes, 2 * chunk + 300, seed=52), _regions(genes, 2 * chunk + 300, seed=53),
            _regions(genes, 2 * chunk + 300, seed=54)]
    sets = [g.copy() for g in good]
    sets[1][chunk + 17, 0] = n_chr
    sets[3][2 * chunk + 250, 0] = n_chr
    bs = _group(genes, sets, {"WIN_THREADS": threads, "FUSED_BLOCKS": 1, "WIN_WIDE": 0})
    for regs, bad in ((sets, (1, 3)), (good, ())):
        for b, r in zip(bs, regs):
            b.set_regions(r)
        engine.run_batches(bs, OverlapMode.Overlap, False, SEG, WINDOWS)
        for i, (b, r) in enumerate(zip(bs, regs)):
            if i in bad:
                with pytest.raises(engine._ffi.GffxHipError) as ei:
                    b.wait()
                assert ei.value.code == -5
            else:
                b.wait()
                _seg_pass_check(b, genes.oix, r, OverlapMode.Overlap, False)
    for b in bs:
        b.close()
