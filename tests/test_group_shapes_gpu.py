"""The launch shapes of a launch that serves a group of batches (engine_windows.hip: pair_threads, slots): 512 blocks of 512 threads
(two per CU), 256 blocks of 1024 threads (one per CU, the tables staged once per CU, room for the fine coverage filter) and 256
blocks of 512 threads (one per CU and launch: two launches side by side), each forced through GFFX_HIP_WIN_THREADS /
GFFX_HIP_FUSED_BLOCKS, and the engine's own choice.  Groups of 2, 5 and 8 batches of 1 to 9000 regions (some batches have fewer
rounds than the launch has blocks for them): every batch's results equal the same batch run alone; 16 batches handed over together
(two groups on two streams); a batch whose pair buffer is too small replays at its wait after a grouped launch at every shape.
The engine's own choice for two full groups that alternate on two streams -- 448 blocks, an eighth of the slots left to the other
group's launch -- at the size where it begins.
"""
import numpy as np
import pytest

from gffx_amd import engine, synth
from gffx_amd.engine import OverlapMode

pytestmark = pytest.mark.gpu

# (GFFX_HIP_WIN_THREADS, GFFX_HIP_FUSED_BLOCKS); 0 = the engine's choice
SHAPES = {"512x512": (512, 0), "256x1024": (1024, 0), "256x512": (512, 256), "engine": (0, 0)}
GROUPS = {2: [9000, 1], 5: [1, 4097, 9000, 2048, 513], 8: [9000, 1, 4096, 4097, 777, 8193, 2049, 300]}
SIXTEEN = [9000, 1, 4096, 4097, 777, 8193, 2049, 300, 5000, 2, 6145, 63, 8192, 1025, 3333, 7000]
FLAGS = engine.OUT_FIDS | engine.OUT_OFFSETS


def _pairs_of(b):
    wc = b.counts().astype(np.int64)
    off = b.offsets()[:-1].astype(np.int64)
    qid = np.repeat(np.arange(len(wc), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    got = np.stack([qid, b.fids()[off[qid] + within].astype(np.int64)], axis=1)
    return got[np.lexsort((got[:, 1], got[:, 0]))]


class _World:
    """the index, every batch's regions, and what each batch gives when it runs alone (computed once, shared by the tests)"""

    def __init__(self):
        self.roots = synth.gencode_like_roots(20000, seed=61)
        r = self.roots
        self.ix = engine.TreeIndexData.from_roots(r["chr_offsets"], r["start"], r["end"], r["fid"])
        self.sets, self.alone = {}, {}
        for i, n in enumerate(sorted(set(SIXTEEN + sum(GROUPS.values(), [])))):
            regs = synth.synth_bed(n, seed=9100 + i, edge_frac=0.02, roots=r, width=(100, 12000))
            b = engine.QueryBatch(self.ix, n)
            b.set_regions(regs)
            b.run(OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS)
            b.wait()
            self.sets[n], self.alone[n] = regs, (b.counts().copy(), _pairs_of(b), b.total_hits)
            b.close()

    def batches(self, sizes, shape, group=2):
        threads, blocks = SHAPES[shape]
        out = []
        for n in sizes:
            b = engine.QueryBatch(self.ix, n)
            b.set_option("WIN_THREADS", threads)
            b.set_option("FUSED_BLOCKS", blocks)
            b.set_option("GROUP", group)
            b.set_regions(self.sets[n])
            out.append(b)
        return out

    def check(self, b, n):
        counts, pairs, total = self.alone[n]
        assert np.array_equal(b.counts(), counts), n
        assert b.total_hits == total, n
        assert np.array_equal(_pairs_of(b), pairs), n


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.ix.close()


def _check_shape(bs, sizes, shape):
    threads, blocks = SHAPES[shape]
    if threads:
        assert {b.block_threads for b in bs} == {threads}
    width = bs[0].block_threads
    rounds = [(n + 4 * width - 1) // (4 * width) for n in sizes]
    grid = bs[0].block_count
    assert {b.block_count for b in bs} == {grid}  # (the launch's grid) ...
    assert sum(b.block_share for b in bs) == grid  # ... of which every batch has its share
    assert all(1 <= b.block_share <= r for b, r in zip(bs, rounds))
    if shape != "engine":
        assert grid == min(sum(rounds), blocks or (256 if width == 1024 else 512))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("members", list(GROUPS))
def test_a_group_at_every_shape_equals_its_batches_run_alone(world, members, shape):
    sizes = GROUPS[members]
    bs = world.batches(sizes, shape, group=1)  # (GROUP=1: one launch on one stream, also for two or three batches)
    assert engine.batches_plan(bs)[:2] == (1, members)
    engine.run_batches(bs, OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS, 3 * len(bs))  # three launches over the same buffers
    for b, n in zip(bs, sizes):
        b.wait()
        world.check(b, n)
    _check_shape(bs, sizes, shape)
    for b in bs:
        b.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sixteen_batches_in_two_groups_on_two_streams(world, shape):
    bs = world.batches(SIXTEEN, shape)
    assert engine.batches_plan(bs) == (2, 8, 2)
    engine.run_batches(bs, OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS, 4 * len(bs))
    for b, n in zip(bs, SIXTEEN):
        b.wait()
        world.check(b, n)
    _check_shape(bs[:8], SIXTEEN[:8], shape)
    _check_shape(bs[8:], SIXTEEN[8:], shape)
    for b in bs:
        b.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_capacity_replay_after_a_grouped_launch_at_every_shape(world, shape):
    sizes = GROUPS[5]
    bs = world.batches(sizes, shape, group=1)
    for b in bs:
        b.reserve_hits(16)  # far too few for all but the one-region batch
    engine.run_batches(bs, OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS)
    for b, n in zip(bs, sizes):
        b.wait()
        world.check(b, n)
    for b in bs:
        b.close()


def _keys(b):
    """(region, root_fid) of a waited pass as sorted 64-bit keys"""
    wc = b.counts().astype(np.int64)
    off = b.offsets()[:-1].astype(np.int64)
    qid = np.repeat(np.arange(len(wc), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    return np.sort((qid << 32) | b.fids()[off[qid] + within].astype(np.int64))


def test_full_groups_alternating_on_two_streams_leave_an_eighth_of_the_slots(world):
    """16 batches handed over together are two groups of eight that alternate on two streams: from four rounds per block on
    (8 x 224 rounds of 2048 regions on 448 blocks) such a launch takes 448 blocks of 512 threads, 56 per batch, and leaves 64 slots
    to the other group's launch; one round per batch fewer and it takes all 512.  Either way every batch's results are what the
    batch gives alone -- and serial launches of one group (timed_group_runs) keep every slot."""
    n = 224 * 2048
    regs = synth.synth_bed(n, seed=9300, edge_frac=0.01, roots=world.roots)
    alone = engine.QueryBatch(world.ix, n)
    alone.set_regions(regs)
    alone.run(OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS)
    alone.wait()
    want_c, want_k = alone.counts().copy(), _keys(alone)
    alone.close()
    bs = []
    for _ in range(16):
        b = engine.QueryBatch(world.ix, n)
        b.set_regions(regs)
        bs.append(b)
    try:
        assert engine.batches_plan(bs) == (2, 8, 2)
        engine.run_batches(bs, OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS, 2 * len(bs))
        for b in bs:
            b.wait()
            assert (b.block_threads, b.block_count, b.block_share, b.filter_level) == (512, 448, 56, 1)
            assert np.array_equal(b.counts(), want_c)
        for b in (bs[0], bs[7], bs[8], bs[15]):
            assert np.array_equal(_keys(b), want_k)
        us, grouped = engine.timed_group_runs(bs[:8], OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS, 2)
        assert grouped and (bs[0].block_threads, bs[0].block_count) == (1024, 256)  # (nothing else in flight: one 1024-thread block per CU)
        for b in bs[:8]:
            b.set_option("WIN_THREADS", 512)
        us, grouped = engine.timed_group_runs(bs[:8], OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS, 2)
        assert grouped and (bs[0].block_threads, bs[0].block_count) == (512, 512)
        for b in bs[:8]:
            b.set_option("WIN_THREADS", 0)
        short = n - 2048  # 223 rounds per batch: 3.98 per block of 448
        for b in bs:
            b.set_regions(regs[:short])
        engine.run_batches(bs, OverlapMode.Overlap, False, FLAGS, engine.STRATEGY_WINDOWS, 2 * len(bs))  # (the walk's first launch finds nothing in flight)
        for b in bs:
            b.wait()
            assert (b.block_threads, b.block_count, b.block_share) == (512, 512, 64)
            assert np.array_equal(b.counts(), want_c[:short])
    finally:  # (a batch that ran in a group must not outlive its index: the group's stream is the index's)
        for b in bs:
            b.close()
