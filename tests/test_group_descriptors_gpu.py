"""The group launch's narrow pair kernel reads its buffers through descriptors the host made (PairDescs): the
regions, the counts, the pair buffer and the segment bases each through ONE descriptor of the whole buffer, the round's or the run's
place in the vector offset, the hardware's range check in place of every bounds test.  What can go wrong is at the edges: a partial
last round, a last segment-base group, a run that crosses the capacity, a buffer the pass does not have.  Everything goes through
the C-ABI against the oracle: counts in input order, the multiset of root_fids per region (placed by the segment bases), the total.
Reference semantics: utils/tree.rs:98-121, commands/intersect.rs:139-165.

A round is 2048 regions (512 threads x 4), a segment-base group 256.  run_batches takes ONE set of flags for all its batches and
batches of different flags do not group (windows_groupable), so "a counts-only batch among pair batches" cannot be formed: whole
groups without pair output / without segment bases are what runs with an empty descriptor, and that is what is tested.
"""
import numpy as np
import pytest

from gffx_amd import engine, synth
from gffx_amd.engine import OverlapMode
from oracle import binding as ob

pytestmark = pytest.mark.gpu

PAIRS = engine.OUT_FIDS | engine.OUT_SEGBASE


# A genome small enough that 2000 roots are hit: at scale 1 a wave's 256 regions keep ~330 pairs -- most rounds fit one strip (384
# words), some take all three --, at 0.4 ~860 (every round takes the three strips and is flushed at once), at 0.25 ~1400 (beyond the
# strips: the synchronous path, which keeps reading the plain pointers).
SCALES = [1.0, 0.4, 0.25]


def _chroms(scale):
    return [("c1", int(20e6 * scale)), ("c2", int(12e6 * scale)), ("c3", int(9e6 * scale)), ("c4", int(5e6 * scale)),
            ("c5", int(2e6 * scale)), ("c6", 300_000)]


@pytest.fixture(scope="module", params=SCALES, ids=lambda s: "genome%g" % s)
def world(request):
    chroms = _chroms(request.param)
    roots = synth.gencode_like_roots(2000, seed=77, chroms=chroms)
    co, s, e, f = roots["chr_offsets"], roots["start"], roots["end"], roots["fid"]
    w = {"roots": roots, "chroms": chroms, "oix": ob.OracleIndex.from_roots(co, s, e, f),
         "ix": engine.TreeIndexData.from_roots(co, s, e, f), "want": {}}
    yield w
    w["ix"].close()


def _regions(world, n, seed):
    return synth.synth_bed(n, seed=seed, chroms=world["chroms"], edge_frac=0.02, roots=world["roots"])


def _want(world, key, regions, mode, invert):
    """(sorted (region, root_fid) rows, counts) of the oracle, computed once per (set, mode, invert)"""
    k = (key, int(mode), bool(invert))
    if k not in world["want"]:
        t, c = world["oix"].query_features(regions, int(mode), invert)
        wc = c.astype(np.int64)
        by_chr = np.argsort(regions[:, 0], kind="stable")  # the oracle walks seqid after seqid, regions in input order
        rows = np.stack([np.repeat(by_chr, wc[by_chr]), t[:, 0].astype(np.int64)], axis=1)
        world["want"][k] = (rows[np.lexsort((rows[:, 1], rows[:, 0]))], c)
    return world["want"][k]


def _pairs_of(b, counts):
    wc = counts.astype(np.int64)
    off = b.offsets_from_segbase(counts).astype(np.int64)
    qid = np.repeat(np.arange(len(wc), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    f = b.fids()
    assert len(f) == wc.sum()
    got = np.stack([qid, f[off[qid] + within].astype(np.int64)], axis=1)
    return got[np.lexsort((got[:, 1], got[:, 0]))]


def _batches(world, sets, soa=()):
    bs = []
    for i, r in enumerate(sets):
        b = engine.QueryBatch(world["ix"], len(r))
        if i in soa:
            b.set_regions_soa(np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1]), np.ascontiguousarray(r[:, 2]))
        else:
            b.set_regions(r)  # rows: the batch's own AoS copy
        b.reserve_hits(12 * len(r) + 1024)  # (room for the densest genome's ~5.3 pairs per region: what is checked is the group's pass, not a replay)
        bs.append(b)
    bs[0].set_option("GROUP", 1)  # one group per walk: 4 batches -> a launch of 4, 8 -> a launch of 8
    assert engine.batches_plan(bs) == (1, len(bs), 1)
    return bs


def _check_pairs(world, b, key, regions, mode=OverlapMode.Overlap, invert=False):
    b.wait()
    want, wc = _want(world, key, regions, mode, invert)
    c = b.counts()
    assert np.array_equal(c, wc)
    assert b.total_hits == len(want)
    assert np.array_equal(_pairs_of(b, c), want)


def _close(bs):
    for b in bs:
        b.close()


EDGES = [1, 255, 256, 257, 2047, 2048, 2049, 4097]


def test_round_and_group_edges_in_one_launch(world):
    """batches of 1 .. 4097 regions in ONE launch of eight: less than a segment-base group, one exactly, one more; a round less one,
    exactly, one more; two rounds and a row.  The last batch's regions are columns, the others rows.  Two passes: the second runs on
    the cursor words the first one zeroed."""
    sets = [_regions(world, n, 9000 + n) for n in EDGES]
    bs = _batches(world, sets, soa={len(sets) - 1})
    assert bs[0].device_regions and not bs[-1].device_regions  # (rows / columns)
    engine.run_batches(bs, OverlapMode.Overlap, False, PAIRS, engine.STRATEGY_WINDOWS, 2 * len(bs))
    for b, r, n in zip(bs, sets, EDGES):
        _check_pairs(world, b, ("edge", n), r)
        assert b.block_threads == 512 and b.block_count >= len(bs)  # (the group's launch: a block per batch at least)
    _close(bs)


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("mode,invert", [(OverlapMode.Overlap, False), (OverlapMode.Contained, False), (OverlapMode.Contained, True),
                                         (OverlapMode.ContainsRegion, False), (OverlapMode.ContainsRegion, True)])
def test_modes_in_groups_of_four_and_eight(world, group, mode, invert):
    sizes = [3000, 2049, 700, 4100, 256, 2048, 1, 5000][:group]
    sets = [_regions(world, n, 9100 + i) for i, n in enumerate(sizes)]
    bs = _batches(world, sets, soa={1})
    engine.run_batches(bs, mode, invert, PAIRS, engine.STRATEGY_WINDOWS)
    for i, (b, r) in enumerate(zip(bs, sets)):
        _check_pairs(world, b, ("mode", i), r, mode, invert)
    _close(bs)


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("short", [0, 1])
def test_a_run_that_ends_at_the_capacity_and_one_that_crosses_it(world, group, short):
    """batch 0's pair buffer holds exactly its P pairs (complete at once), or P - 1 (the run that crosses the capacity loses its
    last word to the range check and nothing is written beyond the buffer; the engine's capacity replay completes the results)"""
    sizes = [4097, 2048, 300, 2049, 1000, 257, 2047, 600][:group]
    sets = [_regions(world, n, 9200 + i) for i, n in enumerate(sizes)]
    want0, _ = _want(world, ("cap", 0), sets[0], OverlapMode.Overlap, False)
    P = len(want0)
    assert P > 1024  # (below that the engine's smallest buffer would hold them all)
    bs = _batches(world, sets)  # fresh batches: the first grouped pass allocates exactly what was reserved
    bs[0].reserve_hits(P - short)
    engine.run_batches(bs, OverlapMode.Overlap, False, PAIRS, engine.STRATEGY_WINDOWS)
    for i, (b, r) in enumerate(zip(bs, sets)):
        _check_pairs(world, b, ("cap", i), r)
    assert bs[0].total_hits == P
    # ... and once more in a group, on the buffers as the first pass (and the replay) left them
    engine.run_batches(bs, OverlapMode.Overlap, False, PAIRS, engine.STRATEGY_WINDOWS)
    for i, (b, r) in enumerate(zip(bs, sets)):
        _check_pairs(world, b, ("cap", i), r)
    _close(bs)


@pytest.mark.parametrize("group", [4, 8])
def test_groups_without_pair_output_and_without_segment_bases(world, group):
    """counts only (no pair buffer, no segment bases: two empty descriptors), then root_fids without segment bases (one), then the
    full pair pass on the same batches"""
    sizes = [2049, 4097, 255, 2048, 3000, 1, 257, 2047][:group]
    sets = [_regions(world, n, 9300 + i) for i, n in enumerate(sizes)]
    bs = _batches(world, sets, soa={group - 1})
    engine.run_batches(bs, OverlapMode.Overlap, False, 0, engine.STRATEGY_WINDOWS)
    for i, (b, r) in enumerate(zip(bs, sets)):
        b.wait()
        want, wc = _want(world, ("out", i), r, OverlapMode.Overlap, False)
        assert np.array_equal(b.counts(), wc) and b.total_hits == len(want)
    engine.run_batches(bs, OverlapMode.Overlap, False, engine.OUT_FIDS, engine.STRATEGY_WINDOWS)
    for i, (b, r) in enumerate(zip(bs, sets)):
        b.wait()
        want, wc = _want(world, ("out", i), r, OverlapMode.Overlap, False)
        assert np.array_equal(b.counts(), wc) and b.total_hits == len(want)
        assert np.array_equal(np.sort(b.fids()), np.sort(want[:, 1].astype(np.uint32)))
    engine.run_batches(bs, OverlapMode.Overlap, False, PAIRS, engine.STRATEGY_WINDOWS)
    for i, (b, r) in enumerate(zip(bs, sets)):
        _check_pairs(world, b, ("out", i), r)
    _close(bs)
