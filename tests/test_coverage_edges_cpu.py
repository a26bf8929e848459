"""tests/_coverage_definition.py held to account before it judges a kernel (tests/test_coverage_edges_gpu.py): merge_rows against
the per-row loop of merge_intervals, covered against a per-base count, hand-worked answers at the edges, and every builder's
claim about WHERE in the sorted order its border, break or pair sits.  No GPU."""
import numpy as np
import pytest

import _coverage_definition as cd

U32_MAX = cd.U32_MAX


def _loop_merge(rows, n_seq):
    """merge_intervals (commands/coverage.rs:92-109) row by row in Python integers."""
    u_off, us, ue, pb = [0], [], [], []
    for c in range(n_seq):
        mine = [(int(s), int(e)) for q, s, e in rows.tolist() if q == c]
        mine.sort(key=lambda t: t[0])  # (stable)
        acc, cur = 0, None
        for s, e in mine:
            if cur is not None and s <= cur[1]:
                cur[1] = max(cur[1], e)
                continue
            if cur is not None:
                us.append(cur[0]), ue.append(cur[1]), pb.append(acc)
                acc += cur[1] - cur[0]
            cur = [s, e]
        if cur is not None:
            us.append(cur[0]), ue.append(cur[1]), pb.append(acc)
        u_off.append(len(us))
    return np.array(u_off, np.uint64), np.array(us, np.uint32), np.array(ue, np.uint32), np.array(pb, np.uint64)


def _dense_covered(rows, seq, a, b):
    """Covered bases of [a, b) on seqid seq, one array cell per base (small coordinates only)."""
    mask = np.zeros(int(rows[:, 2].max()) + 2, bool)
    for q, s, e in rows.tolist():
        if q == seq:
            mask[s:e] = True
    return int(np.count_nonzero(mask[a:b])) if a < b else 0


def _same(got, want):
    for g, w, name in zip(got, want, ("u_off", "us", "ue", "pb")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


def _lists(spans):
    return [x.tolist() for x in spans]


# ---------------------------------------------------------------------------------------------------------------- merge_rows
@pytest.mark.parametrize("seed,n,n_seq,span", [(0, 1, 3, 50), (1, 40, 3, 60), (2, 700, 4, 900), (3, 3000, 7, 100000), (4, 500, 2, 30)])
def test_merge_rows_equals_the_row_loop_on_random_rows(seed, n, n_seq, span):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, span, n)
    rows = cd.rows_of(rng.integers(0, n_seq - 1, n), s, s + rng.integers(1, 12, n))  # (the last seqid stays empty)
    _same(cd.merge_rows(rows, n_seq), _loop_merge(rows, n_seq))


def test_merge_rows_hand_worked():
    # touching: s == end merges, s == end + 1 does not
    rows = np.array([[0, 10, 20], [0, 20, 30], [0, 31, 40]], np.uint32)
    assert _lists(cd.merge_rows(rows, 1)) == [[0, 2], [10, 31], [30, 40], [0, 20]]
    # equal starts, different ends, in both input orders; [5, 8) is inside the longer row only
    for pair in ([[0, 5, 7], [0, 5, 50]], [[0, 5, 50], [0, 5, 7]]):
        rows = np.array(pair + [[0, 8, 9], [0, 51, 52]], np.uint32)
        assert _lists(cd.merge_rows(rows, 1)) == [[0, 2], [5, 51], [50, 52], [0, 45]]
    # a seqid that ends at 0xFFFFFFFF, the next one starts at 0; seqid 0 and 3 have no rows
    rows = np.array([[2, 0, 3], [1, 0xFFFFFFFE, U32_MAX], [1, 0xFFFFFF00, U32_MAX], [2, 3, 4], [1, 7, 9], [2, 6, 7]], np.uint32)
    assert _lists(cd.merge_rows(rows, 4)) == [[0, 0, 2, 4, 4], [7, 0xFFFFFF00, 0, 6], [9, U32_MAX, 4, 7], [0, 2, 0, 4]]
    # nested: the end comes from the first record, not from the span's last
    rows = np.array([[0, 1, 100], [0, 2, 3], [0, 50, 60], [0, 101, 102]], np.uint32)
    assert _lists(cd.merge_rows(rows, 1)) == [[0, 2], [1, 101], [100, 102], [0, 99]]
    # no rows at all
    assert _lists(cd.merge_rows(np.zeros((0, 3), np.uint32), 2)) == [[0, 0, 0], [], [], []]
    got = cd.merge_rows(rows, 1)
    assert [x.dtype for x in got] == [np.uint64, np.uint32, np.uint32, np.uint64]


# ------------------------------------------------------------------------------------------------------------------- covered
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_covered_equals_a_count_over_bases(seed):
    rng = np.random.default_rng(seed)
    n_seq, n = 3, 60
    s = rng.integers(0, 300, n)
    rows = cd.rows_of(rng.integers(0, 2, n), s, s + rng.integers(1, 9, n))
    spans = cd.merge_rows(rows, n_seq)
    q = rng.integers(0, n_seq, 4000)
    a = rng.integers(0, 330, 4000)
    b = a + rng.integers(-3, 60, 4000)
    a, b = np.maximum(a, 0), np.maximum(b, 0)
    want = [_dense_covered(rows, int(c), int(x), int(y)) for c, x, y in zip(q, a, b)]
    got = cd.covered(spans, q, a, b)
    assert got.dtype == np.uint32 and got.tolist() == want


def test_covered_hand_worked():
    # spans of seqid 1: [10, 30) and [31, 40): pb = 0, 20
    spans = cd.merge_rows(np.array([[1, 10, 20], [1, 20, 30], [1, 31, 40]], np.uint32), 3)
    seg = [(1, 10, 30, 20),   # a segment equal to a span
           (1, 0, 10, 0),     # ... ending at us[0]
           (1, 30, 31, 0),    # ... starting at ue[0], ending at us[1]
           (1, 30, 40, 9), (1, 29, 32, 2), (1, 0, U32_MAX, 29), (1, 40, 50, 0), (1, 35, 35, 0), (1, 36, 35, 0),
           (0, 0, 100, 0), (2, 0, 100, 0)]  # seqids without spans
    q, a, b, want = (list(x) for x in zip(*seg))
    assert cd.covered(spans, q, a, b).tolist() == want
    # [0, 0xFFFFFFFF) over a union of more than 2^31 bases: (2^31 + 10) + (2^32 - 1 - 2^31 - 20) = 2^32 - 11
    n_seq, rows = cd.directory_case("more_than_2_31_bases")
    spans = cd.merge_rows(rows, n_seq)
    assert _lists(spans) == [[0, 0, 2], [0, (1 << 31) + 20], [(1 << 31) + 10, U32_MAX], [0, (1 << 31) + 10]]
    got = cd.covered(spans, [1, 1, 1, 1], [0, 5, (1 << 31) + 10, 1 << 31], [U32_MAX, U32_MAX, (1 << 31) + 20, U32_MAX])
    assert got.tolist() == [(1 << 32) - 11, (1 << 32) - 16, 0, (1 << 31) - 11]


# ------------------------------------------------------------------------------------------------------------------ builders
def test_place_keeps_every_row_on_its_sorted_position():
    rows, _ = cd.shape_rows("pairs", 300)
    rows = np.concatenate([cd.rows_of(0, rows[:9, 1], rows[:9, 2]), rows, rows[:50], cd.rows_of(1, rows[:9, 1], rows[:9, 2] + 3)])
    want = cd.sorted_rows(rows)  # (a second seqid, duplicates, equal starts with different ends)
    want[[10, 11]] = want[[11, 10]]  # rows 10 and 11 share (seqid, start) and differ in the end: ask for the OTHER order
    assert want[10, 1] == want[11, 1] and want[10, 2] != want[11, 2]
    got = cd.place(want, 5)
    assert not np.array_equal(got, want) and np.array_equal(cd.sorted_rows(got), want)


@pytest.mark.parametrize("n", cd.EDGE_SIZES)
@pytest.mark.parametrize("shape", cd.SHAPES)
def test_shapes_are_what_they_claim(shape, n):
    rows, spans = cd.shape_rows(shape, n)
    assert rows.shape == (n, 3) and np.array_equal(cd.sorted_rows(cd.place(rows, n)), rows)
    s, e = rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64)
    assert (s < e).all() and (np.diff(s) > 0).all()
    gap = s[1:] - e[:-1]
    if shape == "disjoint":
        assert (gap > 0).all()
    elif shape == "chain":
        assert (gap == 0).all()
    elif shape == "broken_chain":
        assert (gap == 1).all()
    elif shape == "first_covers_all":
        assert (e[1:] < e[0]).all() and (s[1:] > s[0]).all()
    else:
        first = 0 if shape == "pairs" else 1  # index of the first record that opens a pair
        assert (gap[first::2] == 0).all() and (gap[first + 1::2] == 1).all() and (gap[:first] == 1).all()
    want = cd.merge_rows(rows, 3)
    assert len(want[1]) == spans and want[0].tolist() == [0, 0, spans, spans]
    if n <= 257:
        _same(want, _loop_merge(rows, 3))


@pytest.mark.parametrize("p", cd.EDGE_POSITIONS)
@pytest.mark.parametrize("event", cd.EVENTS)
def test_events_sit_where_they_claim(event, p):
    rows, n_seq, spans = cd.event_rows(event, p)
    n = p + 1030
    assert rows.shape == (n, 3) and np.array_equal(cd.sorted_rows(cd.place(rows, p)), rows)
    q, s, e = (rows[:, k].astype(np.int64) for k in range(3))
    assert (s < e).all()
    cm = np.maximum.accumulate(e)  # (valid across the border too: checked per case below)
    i = np.arange(1, n)
    if event == "seqid_border":
        assert np.nonzero(q[1:] != q[:-1])[0].tolist() == [p - 1] and s[p] < cm[p - 1]  # the start alone would merge
        assert (s[1:] <= e[:-1])[i != p].all()
    elif event == "span_break":
        assert (q == 1).all() and np.nonzero(s[1:] > cm[:-1])[0].tolist() == [p - 1] and s[p] == cm[p - 1] + 1
    elif event == "touching_pair":
        assert (q == 1).all() and np.nonzero(s[1:] <= cm[:-1])[0].tolist() == [p - 1] and s[p] == e[p - 1]
    else:
        assert (q == 1).all() and s[p] == cm[p - 1] + 1 and cm[p - 1] == e[0] and (e[1:p] < e[0] - 1000).all()
        assert (s[p + 1:] > cm[p:-1]).all()
    want = cd.merge_rows(rows, n_seq)
    assert len(want[1]) == spans
    if p <= 5:
        _same(want, _loop_merge(rows, n_seq))


@pytest.mark.parametrize("pos", [4, 256, 1024])
def test_restart_rows(pos):
    rows, n_seq = cd.restart_rows(pos)
    assert np.array_equal(cd.sorted_rows(cd.place(rows, pos)), rows)
    assert rows[pos - 1].tolist() == [1, 0xFFFFFFFE, U32_MAX] and rows[pos - 2].tolist() == [1, 0xFFFFFF00, U32_MAX]
    assert rows[pos].tolist()[:2] == [2, 1] and (rows[:pos, 0] == 1).all() and (rows[pos:, 0] == 2).all()
    assert int(rows[pos:, 2].max()) < 1000
    want = cd.merge_rows(rows, n_seq)
    _same(want, _loop_merge(rows, n_seq))
    lo, hi = int(want[0][2]), int(want[0][3])
    assert (want[1][lo - 1], want[2][lo - 1]) == (0xFFFFFF00, U32_MAX) and want[1][lo] == 1 and int(want[2][lo:hi].max()) < 1000


@pytest.mark.parametrize("long_first", [False, True])
@pytest.mark.parametrize("border", [cd.THREAD, cd.WAVE, cd.TILE])
def test_equal_start_rows(border, long_first):
    rows, n_seq, spans = cd.equal_start_rows(border, long_first)
    assert np.array_equal(cd.sorted_rows(cd.place(rows, border)), rows)
    a, b, c, d = rows[border - 1:border + 3].astype(np.int64)
    assert a[1] == b[1] and (a[2] > b[2]) == long_first and {int(a[2]), int(b[2])} == {int(a[1]) + 5, int(a[1]) + 50}
    assert min(a[2], b[2]) < c[1] < c[2] < max(a[2], b[2]) < d[1]
    want = cd.merge_rows(rows, n_seq)
    _same(want, _loop_merge(rows, n_seq))
    assert len(want[1]) == spans and (int(want[1][border - 1]), int(want[2][border - 1])) == (int(a[1]), int(a[1]) + 50)


@pytest.mark.parametrize("n_seq", cd.SORT_N_SEQ)
def test_sort_plan_rows(n_seq):
    assert cd.seqid_sort_passes(n_seq) == (1 if n_seq <= 256 else 2 if n_seq <= 65536 else 3)
    ids = cd.sort_plan_seqids(n_seq)
    assert ids[0] == 0 and ids[-1] == n_seq - 1 and all((c in ids) == (c < n_seq) for c in (255, 256, 65535, 65536))
    for kind in cd.START_KINDS:
        rows = cd.sort_plan_rows(n_seq, kind)
        s = rows[:, 1]
        assert len(rows) > 4096 and (rows[:, 1] < rows[:, 2]).all() and sorted(set(rows[:, 0].tolist())) == ids
        varies = [len(set(((s >> (8 * b)) & 255).tolist())) > 1 for b in range(4)]
        assert varies == {"low_byte": [True, False, False, False], "top_byte": [False, False, False, True],
                          "all_bytes": [True] * 4}[kind]
        if kind == "top_byte":
            assert len(set(s.tolist())) == 256
        if kind == "all_bytes":
            assert int(s.min()) == 0 and int(s.max()) == U32_MAX - 1


@pytest.mark.parametrize("name", cd.DIRECTORY_CASES)
def test_directory_cases(name):
    n_seq, rows = cd.directory_case(name)
    spans = cd.merge_rows(rows, n_seq)
    assert len(spans[1]) == len(rows)  # the rows are the spans
    us = spans[1].astype(np.int64)
    rule = {c: cd.directory_rule(us[int(spans[0][c]):int(spans[0][c + 1])]) for c in range(n_seq) if spans[0][c + 1] > spans[0][c]}
    if name == "one_span_per_seqid":
        assert [rule[c] for c in range(7)] == [(0, 1), (0, 16), (1, 9), (1, 9), (24, 16), (25, 9), (28, 16)]
    elif name == "eight_spans":
        assert len(us) == 8 and rule[1] == (1, 9)  # budget 16 < 18
    elif name == "nine_spans":
        assert len(us) == 9 and rule[1] == (0, 18)  # budget 18
    elif name == "starts_on_bin_edges":
        assert rule[0] == (24, 14) and (us % (1 << 24) == 0).all()
        assert sorted(set(range(14)) - set((us >> 24).tolist())) == [5, 6, 9, 10, 11]
    elif name == "empty_bins_in_the_middle":
        shift, nb = rule[2]
        filled = set((us >> shift).tolist())
        assert nb == 15 and filled == {0, 11, 14}
    elif name == "empty_first_bins":
        shift, nb = rule[1]
        assert (shift, nb) == (28, 13) and int(us.min() >> shift) == 4
    elif name == "spread_to_the_top":
        assert int(spans[2].max()) == U32_MAX and len(us) == 40
    else:
        assert int(spans[3][-1]) + int(spans[2][-1]) - int(spans[1][-1]) > 1 << 31
    q, a, b = cd.probe_segments(spans, n_seq)
    for c, (shift, nb) in rule.items():
        lo, hi = int(spans[0][c]), int(spans[0][c + 1])
        xs = set(a[q == c].tolist())
        assert xs == set(b[q == c].tolist()) and {0, U32_MAX} <= xs
        for v in spans[1][lo:hi].tolist() + spans[2][lo:hi].tolist() + [k << shift for k in range(nb + 1)]:
            assert {x for x in (v - 1, v, v + 1) if 0 <= x <= U32_MAX} <= xs
        assert len(a[q == c]) == len(xs) ** 2  # every pair, a >= b included
    assert set(q.tolist()) == set(range(n_seq))


def test_fold_split_rows():
    rows = cd.fold_split_rows()
    n = cd.UNION_FOLD + 1025
    assert rows.shape == (n, 3) and (rows[:, 1] < rows[:, 2]).all()
    head, tail = rows[:cd.UNION_FOLD], rows[cd.UNION_FOLD:]
    spans, first = cd.merge_rows(rows, 3), cd.merge_rows(head, 3)
    assert 150 < len(first[1]) < 400 and len(spans[1]) - len(first[1]) == 257 + 1  # 257 isolated rows and one cluster are new
    # ... and the second fold lengthens the last span of seqid 0
    k = int(first[0][1]) - 1
    assert spans[1][k] == first[1][k] and spans[2][k] > first[2][k] and int(tail[tail[:, 0] == 0, 1].min()) <= int(first[2][k])
    assert int(tail[tail[:, 0] == 1, 1].min()) > int(head[head[:, 0] == 1, 2].max())
