"""Join B's region sort on the GPU: how many radix passes ran, and what a reused LineTable carries from one run into the next.

The sort's last two passes ("byte 3 of start", "seqid") become ONE pass over the mixed-radix digit lut[seqid] + (start >> 24) when that
digit fits 256 values (radix_sort.hpp).  Whether it fits is decided on the device and posted to the host, which enqueues
one pass or two; `LineTable.last_sort_passes` says what ran.  Every case here compares that count with the documented rule restated
in numpy AND with the literal number the case was built for, the region tables with the numpy definition bit for bit, and the keep
flags of all three modes with the oracle's literal scan -- on inputs AT the edges of the rule (digit totals of 256 / 257, starts of
2^28 - 1 / 2^28, 256 / 257 seqids, seqids without rows inside the lookup table), on three and more sort tiles, on one table driven
large -> small -> large, fits -> does not fit -> fits, degenerate rows -> none -> degenerate rows, many seqids -> few."""
import numpy as np
import pytest

from gffx_amd import engine
from gffx_amd.engine import OverlapMode
from _join_b_tables import _host_tables, _oracle_keep

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
MODES = (OverlapMode.Contained, OverlapMode.ContainsRegion, OverlapMode.Overlap)  # Overlap last: its tables carry dq_off / de
N_LINES = 2000


def expected_passes(regions, n_seq):
    """The documented rule (header comment of radix_sort.hpp), not read off the device: four passes over the start, then
    the seqid's bytes -- or, with <= 256 seqids, every start below 2^28 and sum over the seqids of (largest top byte + 1) <= 256, four
    passes in all.  (No regions: nothing is sorted.)"""
    if len(regions) == 0:
        return 0
    seq_bytes = 1 if n_seq <= 256 else 2 if n_seq <= 1 << 16 else 3 if n_seq <= 1 << 24 else 4
    if n_seq <= 256 and len(regions):
        hi = regions[:, 1] >> 24
        if (hi < 16).all():
            width = np.zeros(n_seq, np.int64)
            np.maximum.at(width, regions[:, 0], hi.astype(np.int64) + 1)
            if width.sum() <= 256:
                return 4
    return 4 + seq_bytes


def _digit_values(regions, n_seq):
    """Distinct values of the top digit in `regions` (which must fit)."""
    width = np.zeros(n_seq, np.int64)
    hi = (regions[:, 1] >> 24).astype(np.int64)
    np.maximum.at(width, regions[:, 0], hi + 1)
    lut = np.cumsum(width) - width
    return len(np.unique(lut[regions[:, 0]] + hi))


def _rows(rng, seq, start, deg_frac=0.05):
    """(n, 3) u32 rows with random ends, about deg_frac of them with start > end."""
    start = np.asarray(start, np.int64)
    end = np.minimum(start + rng.integers(0, 5000, len(start)), U32)
    deg = rng.random(len(start)) < deg_frac
    end[deg] = np.maximum(start[deg] - 1 - rng.integers(0, 5000, int(deg.sum())), 0)
    return np.stack([np.asarray(seq, np.int64), start, end], axis=1).astype(np.uint32)


def _lines_near(rng, regions, n_seq, n=N_LINES):
    """Lines around the starts and ends of random rows of `regions` (so that every mode keeps some and drops some), about 8 % with a
    seqid the run does not know (>= n_seq) and 5 % with NO_SEQ."""
    pick = regions[rng.integers(0, len(regions), n)].astype(np.int64)
    anchor = np.where(rng.random(n) < 0.7, pick[:, 1], pick[:, 2])
    s = anchor + rng.integers(-3000, 3000, n)
    e = s + np.where(rng.random(n) < 0.5, rng.integers(-20, 200, n), rng.integers(0, 9000, n))
    seq = pick[:, 0].copy()
    seq[rng.random(n) < 0.08] = n_seq + rng.integers(0, 3)
    seq[rng.random(n) < 0.05] = engine.LineTable.NO_SEQ
    return seq.astype(np.uint32), s.clip(0, U32).astype(np.uint32), e.clip(0, U32).astype(np.uint32)


def _same_tables(got, want, tag, with_deg):
    keys = [k for k in want if with_deg or k not in ("dq_off", "de")]
    if not with_deg:
        assert "dq_off" not in got and "de" not in got, tag
    for k in keys:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k)


def _check(lt, lines, regions, n_seq, literal, tag, modes=MODES):
    """One region set through `modes` on the table `lt`: pass count (rule and literal), tables, keep flags."""
    want_t = _host_tables(regions, n_seq)
    rule = expected_passes(regions, n_seq)
    assert rule == literal, (tag, "the restated rule and the case disagree", rule, literal)
    for mode in modes:
        got = lt.test(regions, n_seq, mode)
        passes = lt.last_sort_passes
        # (a run without regions has no sort and no mode-specific table: dq_off / de are all empty)
        _same_tables(lt.tables(len(regions), n_seq), want_t, (tag, mode), mode == OverlapMode.Overlap or len(regions) == 0)
        want = _oracle_keep(*lines, regions, n_seq, mode)
        assert np.array_equal(got, want), (tag, mode, np.flatnonzero(got != want)[:5])
        assert passes == rule, (tag, mode, "sort passes", passes, rule)  # (last: right tables with a wrong count fail HERE)
    return want_t


# ---- A. the fit boundary -----------------------------------------------------------------------------------------------------------

GRCH38_MB = [248, 242, 198, 190, 181, 170, 159, 145, 138, 133, 135, 133, 114, 107, 101, 90, 83, 80, 58, 64, 46, 50, 156, 57]


def _spread16(rng, n_seq, n):
    """n rows over n_seq seqids, starts over all 16 top bytes; every seqid has starts 0x0F000000 and 0x0FFFFFFF (top byte 15)."""
    seq = rng.integers(0, n_seq, n)
    start = (rng.integers(0, 16, n) << 24) | rng.integers(0, 1 << 24, n)
    at = rng.permutation(n)[: 2 * n_seq]
    seq[at] = np.repeat(np.arange(n_seq), 2)
    start[at] = np.tile([0x0F000000, 0x0FFFFFFF], n_seq)
    return seq, start


def _flat256(rng, n):
    """n rows, 256 seqids, every one present (255 too), starts below 2^24: 256 digits of width 1."""
    seq = rng.integers(0, 256, n)
    seq[rng.permutation(n)[:256]] = np.arange(256)
    return seq, rng.integers(0, 1 << 24, n)


def _boundary_case(case):
    """-> (regions, n_seq, passes expected, rows of the small second run, passes expected there)"""
    rng = np.random.default_rng(BOUNDARY_CASES.index(case) + 100)
    small = slice(0, 1 + BOUNDARY_CASES.index(case) % 5)  # 1 .. 5 rows: a one-block histogram
    if case == "sum_256":  # 16 seqids x 16 top bytes = exactly 256 digits
        n_seq, want, want_small = 16, 4, 4
        regions = _rows(rng, *_spread16(rng, 16, 12000))
    elif case == "sum_257":  # ... and one record of a 17th seqid at start 0: 257
        n_seq, want, want_small = 17, 5, 4
        seq, start = _spread16(rng, 16, 12000)
        seq[7001], start[7001] = 16, 0
        regions = _rows(rng, seq, start)
    elif case == "flat_256":
        n_seq, want, want_small = 256, 4, 4
        regions = _rows(rng, *_flat256(rng, 12000))
    elif case == "flat_256_one_2pow24":  # one seqid is two digits wide: 257
        n_seq, want, want_small = 256, 5, 4
        seq, start = _flat256(rng, 12000)
        start[2] = 1 << 24
        regions = _rows(rng, seq, start)
    elif case == "gaps":  # only every third seqid has rows; their widths 1 .. 16 sum to exactly 256; the empty ones must not shift lut
        n_seq, want, want_small = 200, 4, 4
        live = np.arange(0, 200, 3)
        width = 1 + np.arange(len(live)) % 5
        width[[0, 1, 33, 66]] = 16
        width[2] = 6
        assert width.sum() == 256 and width.min() == 1 and live[-1] == 198
        k = rng.integers(0, len(live), 11000)
        top = rng.integers(0, 16, len(k)) % width[k]
        k, top = np.concatenate([k, np.arange(len(live))]), np.concatenate([top, width - 1])  # every seqid's widest row
        order = rng.permutation(len(k))
        regions = _rows(rng, live[k[order]], (top[order] << 24) | rng.integers(0, 1 << 24, len(k)))
    elif case == "edge_2pow28_below":  # the largest start the digit takes
        n_seq, want, want_small = 3, 4, 4
        start = rng.integers(0, 1 << 28, 9000)
        start[[0, 4500]] = (1 << 28) - 1
        regions = _rows(rng, rng.integers(0, 3, 9000), start)
    elif case == "edge_2pow28_at":  # one start of 2^28: top byte 16
        n_seq, want, want_small = 3, 5, 5
        start = rng.integers(0, 1 << 28, 9000)
        start[0] = 1 << 28
        regions = _rows(rng, rng.integers(0, 3, 9000), start)
    elif case == "edge_u32_max":
        n_seq, want, want_small = 3, 5, 5
        start = rng.integers(0, 1 << 28, 9000)
        start[[0, 5000, 8999]] = U32
        regions = _rows(rng, rng.integers(0, 3, 9000), start)
    elif case == "n_seq_257":  # the flat_256 rows with one seqid more: the top digit is not tried, two seqid bytes
        n_seq, want, want_small = 257, 6, 6
        regions = _rows(rng, *_flat256(rng, 12000))
    elif case == "n_seq_70000":  # three seqid bytes
        n_seq, want, want_small = 70000, 7, 7
        regions = _rows(rng, rng.integers(0, 70000, 5000), rng.integers(0, 1 << 24, 5000))
    elif case == "one_bin":  # one seqid, one top byte, bytes 0 .. 2 varied: the top-digit pass is a straight copy
        n_seq, want, want_small = 1, 4, 4
        regions = _rows(rng, np.zeros(12000, np.int64), (5 << 24) | rng.integers(0, 1 << 24, 12000))
    elif case == "one_key":  # one (seqid, start), distinct ends on both sides of it: EVERY pass is a copy, the input order stays
        n_seq, want, want_small = 1, 4, 4
        regions = np.stack([np.zeros(12000, np.int64), np.full(12000, 0x0301_0207), 0x0301_0207 - 6000 + rng.permutation(12000)],
                           axis=1).astype(np.uint32)
    else:  # grch38_small: the bench batch's shape at 12 000 rows
        assert case == "grch38_small"
        n_seq, want, want_small = 25, 4, 4
        length = np.array([mb * 1_000_000 for mb in GRCH38_MB] + [16_569])
        seq = rng.integers(0, 25, 12000)
        regions = _rows(rng, seq, (rng.random(12000) * length[seq]).astype(np.int64))
        assert regions[:, 1].max() < 1 << 28 and _digit_values(regions, n_seq) > 150
    return regions, n_seq, want, small, want_small


BOUNDARY_CASES = ["sum_256", "sum_257", "flat_256", "flat_256_one_2pow24", "gaps", "edge_2pow28_below", "edge_2pow28_at", "edge_u32_max",
                  "n_seq_257", "n_seq_70000", "one_bin", "one_key", "grch38_small"]


@pytest.mark.parametrize("case", BOUNDARY_CASES)
def test_pass_count_at_the_fit_boundary(case):
    """9 000 - 12 000 regions (three sort tiles of 4096: the top-digit pass looks back), then 1 - 5 of them on the same table."""
    regions, n_seq, want, small, want_small = _boundary_case(case)
    assert len(regions) > 2 * 4096 or case == "n_seq_70000"
    rng = np.random.default_rng(7)
    lines = tuple(np.concatenate(c) for c in zip(_lines_near(rng, regions, n_seq, N_LINES - 400), _lines_near(rng, regions[small], n_seq, 400)))
    lt = engine.LineTable(*lines)
    want_t = _check(lt, lines, regions, n_seq, want, case)
    if case == "one_key":  # the input order kept: the running max / min / degenerate count of the ends AS GIVEN
        e = regions[:, 2]
        assert np.array_equal(want_t["pm"], np.maximum.accumulate(e)) and np.array_equal(want_t["sm"], np.minimum.accumulate(e[::-1])[::-1])
        assert np.array_equal(want_t["cd"], np.cumsum(e < regions[:, 1]) - (e < regions[:, 1]))
    _check(lt, lines, regions[small], n_seq, want_small, (case, "small"))
    lt.close()


SWEEP_N_SEQ = [1, 2, 16, 17, 255, 256, 257, 300]
SWEEP_RANGE = [1 << 16, 1 << 24, 1 << 26, 1 << 28, (1 << 28) + 1, 1 << 32]
SWEEP_N = [1, 63, 4095, 4096, 4097, 12289, 16385, 20480, 20481]  # 1 .. 6 sort tiles, around the look-back window of 4
SWEEP_SEEDS = list(range(30))


def _sweep_case(seed):
    rng = np.random.default_rng(1000 + seed)
    n_seq, span, n = int(rng.choice(SWEEP_N_SEQ)), int(rng.choice(SWEEP_RANGE)), int(rng.choice(SWEEP_N))
    return _rows(rng, rng.integers(0, n_seq, n), rng.integers(0, span, n)), n_seq


def test_sweep_seeds_give_both_outcomes():
    """By the numpy rule alone: the seeds of the sweep below see the top digit fit and not fit."""
    passes = [expected_passes(*_sweep_case(seed)) for seed in SWEEP_SEEDS]
    assert sum(p == 4 for p in passes) >= 8 and sum(p > 4 for p in passes) >= 8, passes


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_pass_count_random_sweep(seed):
    regions, n_seq = _sweep_case(seed)
    rng = np.random.default_rng(seed)
    lines = _lines_near(rng, regions, n_seq)
    lt = engine.LineTable(*lines)
    _check(lt, lines, regions, n_seq, expected_passes(regions, n_seq), ("sweep", seed, n_seq, len(regions)))
    lt.close()


# ---- B. the second sort: the {seqid, end} pairs of the regions with start > end ----------------------------------------------------

def _with_n_deg(rng, n_seq, n, n_deg):
    """n rows with exactly n_deg of them start > end."""
    start = rng.integers(6000, 1 << 22, n)
    end = start + rng.integers(0, 5000, n)
    at = rng.permutation(n)[:n_deg]
    end[at] = start[at] - 1 - rng.integers(0, 5000, n_deg)
    regions = np.stack([rng.integers(0, n_seq, n), start, end], axis=1).astype(np.uint32)
    assert int((regions[:, 1] > regions[:, 2]).sum()) == n_deg
    return regions


@pytest.mark.parametrize("n_seq", [6, 700])
@pytest.mark.parametrize("n_deg", [0, 1, 4095, 4096, 4097, 8193])
def test_degenerate_pairs_sort(n_deg, n_seq):
    """0 .. 3 tiles of two-word records; 700 seqids: SeqMeta outside LDS, two seqid passes in both sorts."""
    rng = np.random.default_rng(n_deg + n_seq)
    regions = _with_n_deg(rng, n_seq, 12000, n_deg)
    lines = _lines_near(rng, regions, n_seq)
    lt = engine.LineTable(*lines)
    want_t = _check(lt, lines, regions, n_seq, 4 if n_seq == 6 else 6, ("deg", n_deg, n_seq))
    assert len(want_t["de"]) == n_deg and int(want_t["dq_off"][-1]) == n_deg
    lt.close()


def test_degenerate_pairs_all_one_key():
    """All 5 000 degenerate rows share one seqid and one end: every pass of the second sort is a copy."""
    rng = np.random.default_rng(5)
    regions = _with_n_deg(rng, 6, 12000, 0)
    at = rng.permutation(12000)[:5000]
    regions[at, 0], regions[at, 2] = 2, 77
    lines = _lines_near(rng, regions, 6)
    lt = engine.LineTable(*lines)
    want_t = _check(lt, lines, regions, 6, 4, "deg_one_key")
    assert len(want_t["de"]) == 5000 and (want_t["de"] == 77).all()
    lt.close()


# ---- C. one table, many runs -------------------------------------------------------------------------------------------------------

def _fits25(rng, n, deg_frac):
    length = np.array([mb * 1_000_000 for mb in GRCH38_MB] + [16_569])
    seq = rng.integers(0, 25, n)
    return _rows(rng, seq, (rng.random(n) * length[seq]).astype(np.int64), deg_frac)


def test_one_table_through_many_runs():
    """Grow-only buffers, the two pinned notes' shared sequence number, the degenerate state and the status words of earlier, larger
    runs: after every step the tables, the pass count and the flags are those of a first run."""
    rng = np.random.default_rng(11)
    first = _fits25(rng, 20000, 0.05)
    over = _fits25(rng, 9000, 0.05)
    over[4000, 1] = (1 << 28) + 5
    seq17, start17 = _spread16(rng, 16, 40000)
    seq17[123], start17[123] = 16, 0
    few17 = _rows(rng, [16, 3, 3, 0, 9], [0, 0x0F000000, 5000, 0x00FFFFFF, 77777], 0.0)
    few17[[1, 4], 2] = few17[[1, 4], 1] - 10
    d3 = _with_n_deg(rng, 3, 12000, 12000)
    steps = [  # (regions, n_seq, mode, passes)
        (first, 25, OverlapMode.Overlap, 4),
        (_fits25(rng, 3, 0.0), 25, OverlapMode.Overlap, 4),
        (over, 25, OverlapMode.Overlap, 5),
        (_fits25(rng, 9000, 0.05), 25, OverlapMode.Contained, 4),
        (_with_n_deg(rng, 700, 12000, 3000), 700, OverlapMode.Overlap, 6),
        (np.zeros((0, 3), np.uint32), 700, OverlapMode.Overlap, 0),
        (d3, 3, OverlapMode.Overlap, 4),
        (_with_n_deg(rng, 3, 12000, 0), 3, OverlapMode.Overlap, 4),
        (_rows(rng, seq17, start17), 17, OverlapMode.ContainsRegion, 5),
        (few17, 17, OverlapMode.Overlap, 4),
        (first, 25, OverlapMode.Overlap, 4),
    ]
    assert (d3[:, 1] > d3[:, 2]).all() and int((few17[:, 1] > few17[:, 2]).sum()) == 2 and not (steps[1][0][:, 1] > steps[1][0][:, 2]).any()
    every = np.concatenate([s[0] for s in steps[:-1]])
    lines = _lines_near(rng, every, 700, 3000)
    lt = engine.LineTable(*lines)
    tables = []
    for i, (regions, n_seq, mode, passes) in enumerate(steps):
        if i == len(steps) - 1:  # a failing call in front of the last step: a seqid >= n_seq
            bad = first.copy()
            bad[::7, 0] = 25
            with pytest.raises(engine._ffi.GffxHipError):
                lt.test(bad, 25, OverlapMode.Overlap)
        _check(lt, lines, regions, n_seq, passes, ("step", i), modes=(mode,))
        tables.append(lt.tables(len(regions), n_seq))
        fresh = engine.LineTable(*lines)
        assert np.array_equal(lt.test(regions, n_seq, mode), fresh.test(regions, n_seq, mode)), ("step", i, "fresh table")
        assert lt.last_sort_passes == fresh.last_sort_passes == passes, ("step", i)
        fresh.close()
    assert tables[0].keys() == tables[-1].keys()
    for k in tables[0]:
        assert np.array_equal(tables[0][k], tables[-1][k]), ("the first call again", k)
    lt.close()
