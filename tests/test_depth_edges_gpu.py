"""k_depth_regions / k_depth_extent at the places where their bookkeeping changes: a run of equal groups that ends on, starts on
or crosses lane 63 / 64 of a block's 64-line chunks, the carry through a chunk without a hit, the two-item walk, the pair step
(duplicate fids, fids without lines), nq at the wave and block edges, the extents and the table's state, and every shape of
Join A pass `accumulate` is handed.  Tables are hand-shaped (tests/_depth_definition.py: hand_table): a region over window w of a
block's root overlaps exactly the lines tagged w.  Every case states, from its inputs alone, that the situation it is named
for is there; then depth, min start and max end must equal the numpy definition, the rule applied to the intended hit set, and
-- for the small cases -- numbers worked out by hand.  The case builders need no GPU: tests/test_depth_edges_cpu.py runs them
against the definition."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gffx_amd import engine
from gffx_amd.engine import OverlapMode
from oracle import binding as ob

from _depth_definition import ABOVE, BELOW, NO_BLOCK, ROOT_STRIDE, _numpy_depth, hand_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
E = engine._ffi.GffxHipError
PAIRS = engine.OUT_FIDS | engine.OUT_OFFSETS
STRATEGIES = [engine.STRATEGY_AUTO, engine.STRATEGY_DIRECT, engine.STRATEGY_SORTED, engine.STRATEGY_FUSED, engine.STRATEGY_WINDOWS]
NONE, ZERO = 0xFFFFFFFF, 0  # min start / max end of a group no region touched


def _rows(regions):
    return np.asarray(regions, np.uint32).reshape(-1, 3)


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("depth", "min start", "max end")):
        assert np.array_equal(g, w), (what, name, np.nonzero(np.asarray(g) != np.asarray(w))[0][:8].tolist())


def _add(want, more):
    return [want[0] + more[0], np.minimum(want[1], more[1]), np.maximum(want[2], more[2])]


class _Device:
    """Index, depth table and one batch for a HandTable."""

    def __init__(self, T, max_q=1024, block_of_fid=None):
        r = T.roots
        self.T = T
        self.ix = engine.TreeIndexData.from_roots(r["chr_offsets"], r["start"], r["end"], r["fid"])
        self.table = engine.DepthTable(T.n_groups, T.block_off, T.ls, T.le, T.lg, T.block_of_fid if block_of_fid is None else block_of_fid)
        self.batch = engine.QueryBatch(self.ix, max_q)

    def add(self, regions, strategy=engine.STRATEGY_AUTO, flags=PAIRS):
        self.batch.set_regions(_rows(regions))
        self.batch.run(OverlapMode.Overlap, False, flags, strategy)
        self.batch.wait()
        self.table.accumulate(self.batch)

    def fresh(self, regions, **kw):
        self.table.reset()
        self.add(regions, **kw)
        return self.table.results()

    def close(self):
        self.batch.close(), self.table.close(), self.ix.close()


@contextlib.contextmanager
def _device(T, **kw):
    d = _Device(T, **kw)
    try:
        yield d
    finally:
        d.close()


class Case:
    """A table, a batch of regions and what the batch must give.  `hits`: [(block, lines)] per (region, block) as intended;
    the builders assert that the regions overlap exactly those lines and that the rule over them equals the definition."""

    def __init__(self, T, regions, hits=None, literal=None, block_of_fid=None):
        self.T, self.regions = T, _rows(regions)
        self.want = T.definition(self.regions, block_of_fid)
        if hits is not None:
            _same(T.expect(hits), self.want, "the rule over the intended hit set against the definition")
        if literal is not None:
            _same([np.array(x) for x in literal], self.want, "the hand-worked numbers against the definition")


# ====================================================================================== a. run and chunk edges
LAYOUTS = {"1": [1], "63": [63], "64": [64], "65": [65], "64+1": [64, 1], "63+2": [63, 2], "1+64": [1, 64], "130": [130],
           "64+64": [64, 64], "200x1": [1] * 200, "63x1+66": [1] * 63 + [66], "empty": []}
NAMES = list(LAYOUTS)
# lines 63 and 64 of the block: one group (a run across the chunk boundary) or two (a run that ends on lane 63)
ONE_RUN_ACROSS_64 = {"65": True, "64+1": False, "63+2": True, "1+64": True, "130": True, "64+64": False, "200x1": False, "63x1+66": True}


def _edge_tags(n):
    """Lines 0, 128, 63, 64 and n - 1 get windows 0 .. 4 (a line takes the first it is named for); every other line lies outside
    all windows, odd ones before them (the smallest starts of the block), even ones behind (the largest ends)."""
    tags = [BELOW if k % 2 else ABOVE for k in range(n)]
    seen = set()
    for w, line in enumerate((0, 128, 63, 64, n - 1)):
        if 0 <= line < n and line not in seen:
            tags[line] = w
            seen.add(line)
    return tags


def _hit_sets(n):
    """name -> block-local lines a region shall overlap, for a block of n lines"""
    out = {}
    if n > 0:
        out["first"], out["last"] = [0], [n - 1]
    if n > 63:
        out["line63"] = [63]
    if n > 64:
        out["line64"], out["lines63+64"] = [64], [63, 64]
    if n > 128:
        out["third_chunk"], out["chunks_one_and_three"] = [128], [0, 128]
    if n > 0:
        out["every"] = list(range(n))
    out["none"] = []
    return out


def family_table():
    return hand_table([LAYOUTS[k] for k in NAMES], [_edge_tags(sum(LAYOUTS[k])) for k in NAMES])


def family_region(T, b, name, lines):
    """The region of hit set `name` of block b, with the presence checks of the set."""
    n = T.n_lines[b]
    if name == "every":
        region = T.whole(b)
    elif name == "none":
        region = T.quiet(b)
    else:
        tags = _edge_tags(n)
        region = T.window(b, min(tags[l] for l in lines), max(tags[l] for l in lines))
    assert T.lines_hit(b, region) == lines, (NAMES[b], name)  # exactly the intended lines, from the table's coordinates
    assert T.roots_hit(region) == [b]  # ... of this block only, and the root is hit even where no line is
    layout = NAMES[b]
    if name == "lines63+64":
        assert (T.group_of_line(b, 63) == T.group_of_line(b, 64)) is ONE_RUN_ACROSS_64[layout]
    if name in ("third_chunk", "chunks_one_and_three") and layout == "130":
        # one run over three chunks; the middle chunk (lines 64 .. 127) holds no hit: the carry passes through it
        assert T.group_of_line(b, 0) == T.group_of_line(b, 128) and not set(lines) & set(range(64, 128))
    if name == "line63" and layout == "63+2":
        assert T.group_of_line(b, 62) != T.group_of_line(b, 63)  # lane 63 starts its run
    if name == "every" and layout in ("63+2", "200x1"):
        assert T.group_of_line(b, 62) != T.group_of_line(b, 63)  # hits before lane 63 in the chunk, in other runs
    return region


FAMILY = [(b, name) for b, k in enumerate(NAMES) for name in _hit_sets(sum(LAYOUTS[k]))]


def case_family_one(T, b, name):
    lines = _hit_sets(T.n_lines[b])[name]
    return Case(T, [family_region(T, b, name, lines)], hits=[(b, lines)])


def case_family_all(T, order=1):
    regions, hits = [], []
    for b, name in FAMILY[::order]:
        lines = _hit_sets(T.n_lines[b])[name]
        regions.append(family_region(T, b, name, lines))
        hits.append((b, lines))
    items = [T.items(r) for r in regions]
    assert len(regions) > 64 and [] in items  # more than one wave; a lane without an item (the block without lines)
    assert all(len({tuple(i) for i in items[w:w + 64]}) >= 3 for w in (0, 64))  # the lanes of a wave own items of different lengths
    return Case(T, regions, hits=hits)


def case_named_literals():
    """[130] with hits in chunks one and three; [63, 2] and [64, 1] with lines 63 and 64 hit.  Block b's root starts at b * 100 000,
    window w at + 2000 + 100 w; line k of a block starts 7 k mod 31 inside its window and ends 5 k mod 29 before its end."""
    T = hand_table([[130], [63, 2], [64, 1]], [_edge_tags(130), _edge_tags(65), _edge_tags(65)])
    regions = [T.window(0, 0, 1), T.window(1, 2, 3), T.window(2, 2, 3)]
    assert [T.lines_hit(b, regions[b]) for b in range(3)] == [[0, 128], [63, 64], [63, 64]]
    assert T.sizes == [[130], [63, 2], [64, 1]]
    # line 0: window 0, [2000, 2100); line 128: window 1, 2100 + 896 % 31 = 2128 .. 2200 - 640 % 29 = 2198
    # line 63: window 2, + 2200 + 441 % 31 = + 2207 .. + 2300 - 315 % 29 = + 2275; line 64: window 3, + 2314 .. + 2399
    literal = ([1, 0, 1, 1, 1],
               [2000, NONE, 102207, 202207, 202314],
               [2198, ZERO, 102399, 202275, 202399])
    return Case(T, regions, hits=[(0, [0, 128]), (1, [63, 64]), (2, [63, 64])], literal=literal)


def case_lines_that_touch_the_region():
    """A block's first line fills its window to both ends: it touches the regions over the windows beside it, and half-open
    intervals that touch do not overlap (depth.rs:78-82)."""
    T = hand_table([[1, 1, 1]], [[1, 0, 2]])
    regions = [T.window(0, 0), T.window(0, 2)]
    assert T.ls[0] == regions[0][2] and T.le[0] == regions[1][1]  # line 0 starts where region 0 ends, ends where region 1 starts
    assert [T.lines_hit(0, r) for r in regions] == [[1], [2]]
    return Case(T, regions, hits=[(0, [1]), (0, [2])], literal=([0, 1, 1], [NONE, 2007, 2214], [ZERO, 2095, 2290]))


@pytest.fixture(scope="module")
def family():
    d = _Device(family_table())
    yield d
    d.close()


@pytest.mark.parametrize("b,name", FAMILY, ids=["%s-%s" % (NAMES[b], name) for b, name in FAMILY])
def test_one_region_on_a_run_or_chunk_edge(family, b, name):
    c = case_family_one(family.T, b, name)
    _same(family.fresh(c.regions), c.want)


@pytest.mark.parametrize("order", [1, -1])
def test_every_run_and_chunk_edge_region_in_one_batch(family, order):
    c = case_family_all(family.T, order)
    _same(family.fresh(c.regions), c.want)


@pytest.mark.parametrize("case", [case_named_literals, case_lines_that_touch_the_region])
def test_named_edges_give_the_hand_worked_numbers(case):
    c = case()
    with _device(c.T) as d:
        _same(d.fresh(c.regions), c.want)


# ====================================================================================== b. item pairing
def pairing_table():
    return hand_table([[1], [130], [5], [64, 64]], [None, _edge_tags(130), None, None])


def pairing_cases(T):
    """name -> (regions, the items [line counts] each region owns).  Region i of a batch is lane i % 64 of its wave; the wave
    pairs the lanes that own an item in lane order."""
    gap = T.gap(0)
    return {
        "1_line_then_130": ([T.whole(0), T.whole(1)], [[1], [130]]),
        "130_lines_then_1": ([T.whole(1), T.whole(0)], [[130], [1]]),
        "1_line_then_the_third_chunk_of_130": ([T.whole(0), T.window(1, 1)], [[1], [130]]),
        "three_items": ([T.whole(0), T.whole(1), T.whole(2)], [[1], [130], [5]]),
        "one_item_on_lane_63": ([gap] * 63 + [T.whole(1)], [[]] * 63 + [[130]]),
        "items_on_lanes_0_and_63": ([T.whole(1)] + [gap] * 62 + [T.whole(3)], [[130]] + [[]] * 62 + [[128]]),
        "64_regions_on_one_block": ([T.whole(1), T.window(1, 0, 1)] * 32, [[130]] * 64),
    }


PAIRINGS = list(pairing_cases(pairing_table()))


def case_pairing(T, name):
    regions, items = pairing_cases(T)[name]
    assert [T.items(r) for r in regions] == items and len(regions) <= 64  # one wave; who owns what, from the index and the table
    c = Case(T, regions)
    if name == "1_line_then_the_third_chunk_of_130":
        assert T.lines_hit(1, regions[1]) == [128]  # the longer item's only hit comes two chunks after the shorter one ended
    if name == "64_regions_on_one_block":
        assert int(c.want[0][T.group0[1]]) == 64  # both item slots add to the same depth[g]
    return c


@pytest.fixture(scope="module")
def pairing():
    d = _Device(pairing_table())
    yield d
    d.close()


@pytest.mark.parametrize("name", PAIRINGS)
def test_the_two_item_walk(pairing, name):
    c = case_pairing(pairing.T, name)
    _same(pairing.fresh(c.regions), c.want)


# ====================================================================================== c. pair step
def case_pair_step():
    """One wave of regions with 1, 2, 4 and 5 pairs.  Index order of the roots: blocks 0, 1, 2, a second root of block 0's fid,
    block 3 (no lines), a root whose fid 7 has no block, blocks 4, 5, 6; the device table knows fids below 11 only, so block 6
    (fid 12) is out of its range."""
    T = hand_table([[2], [1, 1], [3], [], [2], [1], [1]],
                   extra_roots=[(270_000, 270_500, 0), (370_000, 370_500, 7)])
    known = T.block_of_fid[:11].copy()              # what the device table is built with
    for_definition = T.block_of_fid.copy()
    for_definition[11:] = NO_BLOCK                  # ... which the definition sees as: those fids have no block
    dup = (0, 0, 270_100)
    five = (0, 300_000, 660_000)
    regions = [T.whole(0), T.whole(0, 1), dup, five, T.whole(4), T.whole(4, 5), T.whole(6)]
    fid = T.roots["fid"]
    assert [len(T.roots_hit(r)) for r in regions] == [1, 2, 4, 5, 1, 2, 1]  # lanes of one wave with different pair counts
    assert fid[T.roots_hit(dup)].tolist() == [0, 2, 4, 0]  # one fid on two roots that are not neighbours in the index
    assert fid[T.roots_hit(five)].tolist() == [6, 7, 8, 10, 12]
    assert T.n_lines[3] == 0 and T.block_of_fid[6] == 3            # a block without lines
    assert T.block_of_fid[7] == NO_BLOCK                            # a fid without a block
    assert int(fid.max()) == 12 and len(known) == 11 and T.n_lines[6] > 0 and T.lines_hit(6, five)  # a fid >= the table's n_fid
    # groups: block 0: 0; block 1: 1, 2; block 2: 3; block 4: 4; block 5: 5; block 6: 6
    c = Case(T, regions, block_of_fid=for_definition)
    assert c.want[0].tolist() == [3, 2, 2, 1, 3, 2, 0]  # group 0: regions 0, 1 and `dup` ONCE; group 6 is never reached
    assert c.want[1][6] == NONE and c.want[2][6] == ZERO
    c.known = known
    return c


def test_the_pair_step_dedups_and_skips():
    c = case_pair_step()
    with _device(c.T, block_of_fid=c.known) as d:
        for strategy in STRATEGIES:  # (the order of a region's pairs is the strategy's own)
            _same(d.fresh(c.regions, strategy=strategy), c.want, strategy)


# ====================================================================================== d. nq
NQS = [1, 63, 64, 65, 255, 256, 257]


def case_nq(T, nq, late):
    """The family's regions over and over; the last region overlaps every line of [130].  late: no region before row
    min(192, nq - 1) has a pair -- the first three waves of a block have nothing to do (or, below 193 rows, only the last lane has)."""
    pool = [family_region(T, b, name, _hit_sets(T.n_lines[b])[name]) for b, name in FAMILY]
    regions = [pool[i % len(pool)] for i in range(nq)]
    b130 = NAMES.index("130")
    regions[-1] = T.whole(b130)
    if late:
        for i in range(min(192, nq - 1)):
            regions[i] = T.gap(i % len(NAMES))
        assert not any(T.roots_hit(r) for r in regions[:min(192, nq - 1)])
    assert len(regions) == nq and T.lines_hit(b130, regions[-1]) == list(range(130))
    c = Case(T, regions)
    assert int(c.want[0][T.group0[b130]]) >= 1
    return c


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("nq", NQS)
def test_nq_at_the_wave_and_block_edges(family, nq, late):
    c = case_nq(family.T, nq, late)
    b = engine.QueryBatch(family.ix, nq)  # (a batch of exactly nq rows)
    try:
        b.set_regions(c.regions)
        b.run(OverlapMode.Overlap, False, PAIRS)
        b.wait()
        family.table.reset()
        family.table.accumulate(b)
        _same(family.table.results(), c.want)
    finally:
        b.close()


# ====================================================================================== e. extents and state
def case_extent_over_the_overlapped_lines_only():
    T = hand_table([[3]], [[BELOW, 0, ABOVE]])
    region = T.window(0, 0)
    assert T.lines_hit(0, region) == [1]
    assert T.ls[0] < T.ls[1] and T.le[2] > T.le[1] and T.lg.tolist() == [0, 0, 0]  # the group's other lines: smaller start, larger end
    return Case(T, [region], hits=[(0, [1])], literal=([1], [2007], [2095]))


def test_extent_is_taken_over_the_overlapped_lines_only():
    c = case_extent_over_the_overlapped_lines_only()
    with _device(c.T) as d:
        _same(d.fresh(c.regions), c.want)


def case_state():
    """Blocks [3, 2] and [2]; windows 0, 1, 2 hold lines 0 | 3, 1 | 4 and 2 of block 0; nothing ever overlaps block 1."""
    T = hand_table([[3, 2], [2]], [[0, 1, 2, 0, 1], None])
    first, second = [T.window(0, 0)], [T.window(0, 1)]
    assert T.lines_hit(0, first[0]) == [0, 3] and T.lines_hit(0, second[0]) == [1, 4]  # other lines of the same two groups
    c1 = Case(T, first, hits=[(0, [0, 3])], literal=([1, 1, 0], [2000, 2021, NONE], [2100, 2085, ZERO]))
    c2 = Case(T, second, hits=[(0, [1, 4])], literal=([1, 1, 0], [2107, 2128, NONE], [2195, 2180, ZERO]))
    both = Case(T, first + second, literal=([2, 2, 0], [2000, 2021, NONE], [2195, 2180, ZERO]))
    return T, c1, c2, both


def test_results_twice_between_accumulates_and_after_reset():
    T, c1, c2, both = case_state()
    with _device(T) as d:
        r1 = d.fresh(c1.regions)
        _same(r1, c1.want)
        _same(d.table.results(), r1, "results() read a second time")
        d.add(c2.regions)  # accumulate -> results -> accumulate -> results
        _same(d.table.results(), both.want)
        _same(d.table.results(), both.want, "results() read a second time")
        d.table.reset()
        _same(d.table.results(), (np.zeros(3, np.uint64), np.full(3, NONE, np.uint32), np.zeros(3, np.uint32)), "after reset()")
        d.add(c2.regions)  # the old line flags are gone: the extents are those of lines 1 and 4 alone
        _same(d.table.results(), c2.want, "other lines of the same groups after reset()")


def test_tables_without_groups_or_lines():
    T = hand_table([[]])
    assert T.n_groups == 0 and len(T.ls) == 0 and T.roots_hit(T.quiet(0)) == [0]
    with _device(T) as d:
        got = d.fresh([T.quiet(0), T.whole(0)])
        assert [len(a) for a in got] == [0, 0, 0]
        d.table.close()
        # groups, and no line in any of them
        d.table = engine.DepthTable(3, T.block_off, T.ls, T.le, T.lg, T.block_of_fid)
        _same(d.fresh([T.quiet(0), T.whole(0)]), (np.zeros(3, np.uint64), np.full(3, NONE, np.uint32), np.zeros(3, np.uint32)))


def test_an_index_closed_before_its_batches_outlives_them():
    """gffx_hip_batch_destroy reads its index (the device, the count of busy batches).  When a failing test leaves an index and
    its batches to the collector, their finalisers run in no particular order: an index finalised first was freed under its
    batches, and the next pass of any batch met the error that left behind.  close() of an index now waits for its batches."""
    T, c1, _, _ = case_state()
    d = _Device(T)
    second = engine.QueryBatch(d.ix, 8)
    d.ix.close()
    assert d.ix._h is not None  # two batches are open
    _same(d.fresh(c1.regions), c1.want)  # ... and still work
    d.batch.close()
    assert d.ix._h is not None
    second.close()
    assert d.ix._h is None  # the last one took the index along
    d.table.close()
    with _device(T) as again:  # nothing was left behind for the next launch to find
        _same(again.fresh(c1.regions), c1.want)


# ====================================================================================== f. pass shapes
SHAPE_LAYOUTS = [[], [1], [3, 1, 2], [64], [65, 5], [1] * 70, [130], [20, 20, 30], [2], [63, 2]]


def shapes_world():
    """40 blocks of the layouts above with random window tags (8 windows), and 320 regions: window ranges, whole roots, rows that
    hit a root and no line, rows without a pair, zero-length and reversed rows, and rows 2 to 30 roots wide
    (whole roots from block 10 on only: before it, a group without a line in a window stays untouched)."""
    rng = np.random.default_rng(5)
    blocks = [SHAPE_LAYOUTS[int(rng.integers(len(SHAPE_LAYOUTS)))] for _ in range(40)]
    blocks[:len(SHAPE_LAYOUTS)] = SHAPE_LAYOUTS  # (every layout at least once)
    tags = [[int(rng.choice([BELOW, ABOVE, 0, 1, 2, 3, 4, 5, 6, 7])) for _ in range(sum(bl))] for bl in blocks]
    T = hand_table(blocks, tags)
    assert 1000 < len(T.ls) < 2000
    regions = []
    for i in range(320):
        b, kind = int(rng.integers(40)), i % 8
        if kind < 3:
            w = int(rng.integers(8))
            regions.append(T.window(b, w, min(7, w + int(rng.integers(3)))))
        elif kind == 3:
            regions.append(T.whole(10 + b % 30))
        elif kind == 4:
            regions.append(T.quiet(b))
        elif kind == 5:
            regions.append(T.gap(b))
        elif kind == 6:
            regions.append(T.whole(10 + b % 30, min(39, 11 + b % 30 + int(rng.integers(30)))))
        else:
            s = T.window(b, 3)[1] + 50
            regions.append((0, s, s) if i % 16 == 7 else (0, s + 40, s))
    regions = _rows(regions)
    n_pairs = np.array([len(T.roots_hit(r)) for r in regions])
    assert (n_pairs == 0).sum() >= 40 and (n_pairs >= 10).sum() >= 10
    assert (regions[:, 2].astype(np.int64) - regions[:, 1] >= 10 * ROOT_STRIDE).sum() >= 10  # rows of a million bases and more
    want = T.definition(regions)
    assert int(want[0].sum()) > 1000 and (want[0] == 0).any()
    return T, regions, want


@pytest.fixture(scope="module")
def shapes():
    T, regions, want = shapes_world()
    regions.setflags(write=False)
    for a in want:
        a.setflags(write=False)
    d = _Device(T, max_q=len(regions))
    d.regions, d.want = regions, want
    yield d
    d.close()


def _accumulate_fresh(d, b):
    d.table.reset()
    d.table.accumulate(b)
    return d.table.results()


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("flags", [PAIRS, PAIRS | engine.OUT_COUNTS | engine.OUT_TRIPLES], ids=["pairs", "pairs+counts+triples"])
def test_host_regions_aos_and_soa_under_every_strategy(shapes, strategy, flags):
    b = shapes.batch
    b.set_regions(shapes.regions)
    b.run(OverlapMode.Overlap, False, flags, strategy)
    b.wait()
    _same(_accumulate_fresh(shapes, b), shapes.want, "AoS")
    b.set_regions_soa(shapes.regions[:, 0], shapes.regions[:, 1], shapes.regions[:, 2])
    b.run(OverlapMode.Overlap, False, flags, strategy)
    b.wait()
    _same(_accumulate_fresh(shapes, b), shapes.want, "SoA")


def test_auto_takes_the_wide_form_for_these_regions(shapes):
    b = shapes.batch
    b.set_regions(shapes.regions)
    b.run(OverlapMode.Overlap, False, PAIRS, engine.STRATEGY_AUTO)
    assert b.wide_form
    b.wait()
    _same(_accumulate_fresh(shapes, b), shapes.want)


@pytest.mark.parametrize("shift", [0, 1])
def test_device_resident_regions_aligned_and_shifted(shapes, shift):
    hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    regions, cols = shapes.regions, []
    for c in range(3):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), 4 * (len(regions) + 8)) == 0
        col = np.ascontiguousarray(regions[:, c])
        assert hip.hipMemcpy(p.value + 4 * shift, col.ctypes.data, col.nbytes, 1) == 0  # hipMemcpyHostToDevice
        cols.append(p)
    b = engine.QueryBatch(shapes.ix, len(regions))
    b.set_regions_device(*(p.value + 4 * shift for p in cols), len(regions))
    for strategy in STRATEGIES:
        b.run(OverlapMode.Overlap, False, PAIRS, strategy)
        b.wait()
        _same(_accumulate_fresh(shapes, b), shapes.want, strategy)
    b.close()
    for p in cols:
        hip.hipFree(p)


@pytest.mark.parametrize("strategy", [engine.STRATEGY_AUTO, engine.STRATEGY_SORTED])
def test_region_store_slots_and_subranges(shapes, strategy):
    """What the CLI does: set_regions_store + STRATEGY_AUTO, over both slots of the ring, and a batch that starts inside a slot."""
    regions, n = shapes.regions, len(shapes.regions)
    store = engine.RegionStore(0, n, False)
    b = engine.QueryBatch(shapes.ix, n)
    other = np.ascontiguousarray(regions[::-1])
    for k in (0, 1):
        store.staging(k)[:n] = regions if k == 0 else other
        store.append(k, n)
    for k, rows in ((0, regions), (1, other)):
        for first, m in ((0, n), (3, n - 3), (65, 130)):
            b.set_regions_store(store, k, first, m)
            b.run(OverlapMode.Overlap, False, PAIRS, strategy)
            b.wait()
            want = shapes.want if (first, m) == (0, n) else shapes.T.definition(rows[first:first + m])
            _same(_accumulate_fresh(shapes, b), want, (k, first, m))
    b.close(), store.close()


@pytest.mark.parametrize("strategy", [engine.STRATEGY_AUTO, engine.STRATEGY_WINDOWS])
def test_offsets32_beside_the_64_bit_offsets(shapes, strategy):
    """accumulate reads the 64-bit offsets; a pass that also writes the 32-bit ones must still write those."""
    b = shapes.batch
    b.set_regions(shapes.regions)
    b.run(OverlapMode.Overlap, False, PAIRS | engine.OUT_OFFSETS32, strategy)
    b.wait()
    assert np.array_equal(b.offsets32(), b.offsets()[:-1].astype(np.uint32))
    _same(_accumulate_fresh(shapes, b), shapes.want)


@pytest.mark.parametrize("read_counts_first", [False, True])
def test_sorted_pass_left_in_emission_order(shapes, read_counts_first):
    """STRATEGY_SORTED with OUT_EMIT_ORDER leaves counts and offsets in emission order until someone asks for the input-order
    view; accumulate asks for it itself."""
    b = shapes.batch
    b.set_regions(shapes.regions)
    b.run(OverlapMode.Overlap, False, PAIRS | engine.OUT_EMIT_ORDER, engine.STRATEGY_SORTED)
    b.wait()
    assert b.device_pointers()[0] == 0  # no input-order view yet: the pass was partitioned and is in emission order
    rows, _, _ = b.query_records()
    assert not np.array_equal(rows, np.arange(len(rows)))  # ... which is another order than the input's
    if read_counts_first:
        counts = b.counts()
        assert np.array_equal(counts, [len(shapes.T.roots_hit(r)) for r in shapes.regions])
        assert b.device_pointers()[0] != 0
    _same(_accumulate_fresh(shapes, b), shapes.want)
    assert b.device_pointers()[0] != 0


def test_one_batch_reused_at_other_sizes(shapes):
    b = engine.QueryBatch(shapes.ix, 300)
    shapes.table.reset()
    want = [np.zeros(shapes.T.n_groups, np.uint64), np.full(shapes.T.n_groups, NONE, np.uint32), np.zeros(shapes.T.n_groups, np.uint32)]
    for first, n in ((0, 300), (300, 10), (0, 0), (21, 299)):
        part = shapes.regions[first:first + n]
        assert len(part) == n
        b.set_regions(part)
        b.run(OverlapMode.Overlap, False, PAIRS)
        b.wait()
        shapes.table.accumulate(b)
        want = _add(want, shapes.T.definition(part))
        _same(shapes.table.results(), want, n)
    b.close()


def test_refused_passes_leave_the_results_alone(shapes):
    b = shapes.batch
    b.set_regions(shapes.regions)
    b.run(OverlapMode.Overlap, False, PAIRS)
    b.wait()
    before = _accumulate_fresh(shapes, b)
    _same(before, shapes.want)
    refused = [(OverlapMode.Contained, False, PAIRS), (OverlapMode.ContainsRegion, False, PAIRS), (OverlapMode.Overlap, True, PAIRS),
               (OverlapMode.Overlap, False, engine.OUT_FIDS), (OverlapMode.Overlap, False, engine.OUT_OFFSETS),
               (OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_OFFSETS32),
               (OverlapMode.Overlap, False, engine.OUT_COUNTS | engine.OUT_TRIPLES)]
    for mode, invert, flags in refused:
        b.run(mode, invert, flags)
        b.wait()
        with pytest.raises(E):
            shapes.table.accumulate(b)
        _same(shapes.table.results(), before, (mode, invert, flags))
    b.run(OverlapMode.Overlap, False, PAIRS)
    with pytest.raises(E):  # not waited for
        shapes.table.accumulate(b)
    b.wait()
    _same(shapes.table.results(), before, "unwaited")
    shapes.table.accumulate(b)  # ... and the same batch, waited for, counts
    _same(shapes.table.results(), _add(before, before))


def capacity_world(k=400, nq=3000):
    """k nested roots, each with a block of two groups, and nq copies of one region that hits every root: k * nq pairs, far more
    than a pass's first guess of max(2 nq, 1024)."""
    i = np.arange(k, dtype=np.uint32)
    roots = {"chr_offsets": np.array([0, k], np.uint32), "start": i.copy(), "end": (10_000 - i).astype(np.uint32), "fid": i * 3}
    block_of_fid = np.full(3 * k, NO_BLOCK, np.uint32)
    block_of_fid[i * 3] = i
    ls = np.stack([1000 + i, 3000 + i, np.full(k, 1500, np.uint32)], axis=1).reshape(-1).astype(np.uint32)
    le = np.stack([1010 + i, 3010 + i, 1600 + i], axis=1).reshape(-1).astype(np.uint32)
    lg = np.stack([2 * i, 2 * i, 2 * i + 1], axis=1).reshape(-1).astype(np.uint32)
    block_off = (3 * np.arange(k + 1)).astype(np.uint64)
    regions = np.tile(np.array([[0, 1000, 2000]], np.uint32), (nq, 1))
    assert k * nq > max(2 * nq, 1024)
    one = _numpy_depth(roots, block_of_fid, block_off, ls, le, lg, 2 * k, regions[:1])
    want = (one[0] * np.uint64(nq), one[1], one[2])  # (nq equal regions: nq times one region's depth, the same extents)
    # by hand: every group nq; group 2 i from line (1000 + i, 1010 + i) alone -- (3000 + i, ...) is not overlapped --, group 2 i + 1
    # from (1500, 1600 + i)
    assert np.array_equal(want[0], np.full(2 * k, nq, np.uint64))
    assert np.array_equal(want[1], np.stack([1000 + i, np.full(k, 1500)], axis=1).reshape(-1))
    assert np.array_equal(want[2], np.stack([1010 + i, 1600 + i], axis=1).reshape(-1))
    return roots, block_of_fid, block_off, ls, le, lg, regions, want


def test_a_pass_replayed_after_the_capacity_guess():
    roots, block_of_fid, block_off, ls, le, lg, regions, want = capacity_world()
    ix = engine.TreeIndexData.from_roots(roots["chr_offsets"], roots["start"], roots["end"], roots["fid"])
    table = engine.DepthTable(len(want[0]), block_off, ls, le, lg, block_of_fid)
    for strategy in STRATEGIES:
        b = engine.QueryBatch(ix, len(regions))  # (a new batch: its pair buffers start at the guess)
        b.set_regions(regions)
        b.run(OverlapMode.Overlap, False, PAIRS, strategy)
        b.wait()
        assert b.total_hits == len(regions) * len(roots["fid"])
        table.reset()
        table.accumulate(b)
        _same(table.results(), want, strategy)
        b.close()
    table.close(), ix.close()


# ====================================================================================== g. the CLI against the oracle
def write_cli_inputs(d):
    """gene A: 130 CDS lines that share one ID (CDS i: 2001 + 200 i .. 2100 + 200 i, 1-based closed), and an exon `shared`;
    gene B: 70 exons with IDs of their own, an exon `shared` again, and an exon that ends 1000 bases behind its gene."""
    col = "chr1\tt\t%s\t%d\t%d\t.\t+\t.\t%s\n"
    lines = ["##gff-version 3\n", col % ("gene", 1001, 50000, "ID=geneA"), col % ("mRNA", 1001, 50000, "ID=mA;Parent=geneA")]
    lines += [col % ("CDS", 2001 + 200 * i, 2100 + 200 * i, "ID=cdsA;Parent=mA") for i in range(130)]
    lines += [col % ("exon", 30001, 30100, "ID=shared;Parent=mA")]
    lines += [col % ("gene", 100001, 180000, "ID=geneB"), col % ("mRNA", 100001, 180000, "ID=mB;Parent=geneB")]
    lines += [col % ("exon", 101001 + 1000 * i, 101500 + 1000 * i, "ID=exB%d;Parent=mB" % i) for i in range(70)]
    lines += [col % ("exon", 175001, 175100, "ID=shared;Parent=mB"), col % ("exon", 179901, 181000, "ID=out;Parent=mB")]
    gff, bed = os.path.join(d, "hand.gff"), os.path.join(d, "hand.bed")
    open(gff, "w").write("".join(lines))
    rows = [(2000, 2100),     # CDS 0 only
            (27800, 27900),   # CDS 129, the last
            (14600, 14700),   # CDS 63
            (14800, 14900),   # CDS 64
            (14650, 14850),   # CDS 63 and 64
            (27600, 27700),   # CDS 128: the third chunk of 64
            (1900, 28000),    # every CDS
            (2120, 2180),     # between CDS 0 and 1: the gene and the mRNA, no CDS
            (30000, 30100),   # `shared` in gene A
            (175000, 175100),  # `shared` in gene B
            (163900, 166100),  # exons 63, 64 (and 62's end is before it)
            (179950, 180100),  # the exon that sticks out, inside the gene
            (180500, 180600),  # ... and behind the gene's end: no root, no row
            (60000, 60010)]   # no root
    open(bed, "w").write("".join("chr1\t%d\t%d\n" % r for r in rows))
    return gff, bed, len(rows)


CDS_ROW = b"cdsA\tchr1\t2000\t27900\t7"  # seven regions overlap a CDS line; 0-based start of CDS 0, end of CDS 129
SHARED_ROW = b"shared\tchr1\t30000\t175100\t2"  # one ID in two genes: the groups' depths add up, the extent spans both
OUT_ROW = b"out\tchr1\t179900\t181000\t1"


def _tsv_rows(data):
    lines = data.split(b"\n")
    assert lines[0] == b"id\tchr\tstart\tend\tdepth" and lines[-1] == b""
    return sorted(lines[1:-1])


def test_cli_on_a_hand_written_gff(tmp_path):
    gff, bed, n_rows = write_cli_inputs(str(tmp_path))
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.depth_run(gff, bed, want)
    assert rc == 0, msg
    want_rows = _tsv_rows(open(want, "rb").read())
    for row in (CDS_ROW, SHARED_ROW, OUT_ROW):
        assert row in want_rows
    out = str(tmp_path / "got.tsv")
    for batch_rows in (None, 5):  # 14 rows: one batch, then three
        env = {k: v for k, v in os.environ.items() if k != "GFFX_DEPTH_BATCH_ROWS"}
        if batch_rows:
            assert 2 * batch_rows < n_rows <= 3 * batch_rows
            env["GFFX_DEPTH_BATCH_ROWS"] = str(batch_rows)
        r = subprocess.run([GFFX, "depth", "-i", gff, "-s", bed, "-o", out], capture_output=True, env=env)
        assert r.returncode == 0, r.stderr
        got_rows = _tsv_rows(open(out, "rb").read())
        assert got_rows == want_rows, batch_rows
        assert CDS_ROW in got_rows and SHARED_ROW in got_rows and OUT_ROW in got_rows
