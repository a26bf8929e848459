"""The coverage union (gffx_hip_union_*: DeviceSort::run<3>, k_union_tile_max / _carry / _heads / _emit) and k_segments_covered
at their structural edges, against the exact sparse definition of tests/_coverage_definition.py (its builders are checked without
a GPU in tests/test_coverage_edges_cpu.py).  Every test goes through engine.RegionUnion and engine.segments_covered and compares
all four arrays of spans() -- dtype and values -- or the covered counts.

A  the scan: sizes and sorted positions at a thread's 4 records, a wave's 256, a tile's 1024, k_union_carry's 262 144
B  the union's sort plan: 1 / 2 / 3 seqid bytes, start bytes that make copy passes and real ones
C  state kept across folds on one handle   D  the fold split at 8 Mi rows   E  k_segments_covered's directory and large coordinates
"""
import numpy as np
import pytest

import _coverage_definition as cd
from gffx_amd import engine

pytestmark = pytest.mark.gpu

U32_MAX = cd.U32_MAX


def _assert_spans(got, want):
    for g, w, name in zip(got, want, ("u_off", "us", "ue", "pb")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def _union(n_seq, *adds):
    u = engine.RegionUnion(n_seq)
    for rows in adds:
        u.add(np.ascontiguousarray(rows))
    u.finish()
    return u


def _check(n_seq, rows, n_spans=None, seed=1):
    """The union of the rows -- given sorted, handed over shuffled -- == the definition."""
    want = cd.merge_rows(rows, n_seq)
    if n_spans is not None:
        assert len(want[1]) == n_spans
    u = _union(n_seq, cd.place(rows, seed))
    assert u.n_spans == len(want[1])
    _assert_spans(u.spans(), want)
    u.close()


# ------------------------------------------------------------------------------------------------------------ A: the scan
@pytest.mark.parametrize("n", cd.EDGE_SIZES)
@pytest.mark.parametrize("shape", cd.SHAPES)
def test_shape_at_every_edge_size(shape, n):
    rows, spans = cd.shape_rows(shape, n)
    _check(3, rows, spans, seed=n)


@pytest.mark.parametrize("p", cd.EDGE_POSITIONS)
@pytest.mark.parametrize("event", cd.EVENTS)
def test_event_at_sorted_position(event, p):
    rows, n_seq, spans = cd.event_rows(event, p)
    _check(n_seq, rows, spans, seed=p)


@pytest.mark.parametrize("pos", [4, 256, 1024])
def test_running_maximum_restarts_at_a_seqid_border(pos):
    """Seqid 1 ends with [0xFFFFFF00, 0xFFFFFFFF) and [0xFFFFFFFE, 0xFFFFFFFF); seqid 2's small rows start at sorted position pos."""
    rows, n_seq = cd.restart_rows(pos)
    _check(n_seq, rows, seed=pos)
    u = _union(n_seq, cd.place(rows, pos))
    o, us, ue, _ = u.spans()
    lo, hi = int(o[2]), int(o[3])
    assert (us[lo - 1], ue[lo - 1]) == (0xFFFFFF00, U32_MAX) and us[lo] == 1 and int(ue[lo:hi].max()) < 1000
    u.close()


@pytest.mark.parametrize("long_first", [False, True])
@pytest.mark.parametrize("border", [cd.THREAD, cd.WAVE, cd.TILE])
def test_equal_starts_across_a_border(border, long_first):
    rows, n_seq, spans = cd.equal_start_rows(border, long_first)
    _check(n_seq, rows, spans, seed=border)


# ---------------------------------------------------------------------------------------------------- B: the sort's plan
@pytest.mark.parametrize("kind", cd.START_KINDS)
@pytest.mark.parametrize("n_seq", cd.SORT_N_SEQ)
def test_sort_plan(n_seq, kind):
    rows = cd.sort_plan_rows(n_seq, kind)
    u = _union(n_seq, rows)
    _assert_spans(u.spans(), cd.merge_rows(rows, n_seq))
    u.close()


@pytest.mark.parametrize("n_seq", cd.SORT_N_SEQ)
def test_a_row_on_seqid_n_seq_is_refused(n_seq):
    rows = cd.sort_plan_rows(n_seq, "all_bytes", n=300)
    bad = rows.copy()
    bad[150, 0] = n_seq
    u = engine.RegionUnion(n_seq)
    with pytest.raises(engine._ffi.GffxHipError) as ei:
        u.add(bad)
    assert ei.value.code == -5
    u.close()
    u = _union(n_seq, rows)  # a fresh handle works
    _assert_spans(u.spans(), cd.merge_rows(rows, n_seq))
    u.close()


@pytest.mark.parametrize("n_seq", [1, 257, 65537])
def test_a_copy_pass_becomes_a_real_pass_in_the_second_fold(n_seq):
    low = cd.sort_plan_rows(n_seq, "low_byte")
    high = cd.sort_plan_rows(n_seq, "all_bytes", n=5000, seed=1)
    high[:, 1] |= 1 << 31
    high[:, 2] = np.maximum(high[:, 2] | (1 << 31), high[:, 1] + 1)
    assert int(low[:, 1].max()) < 256 and int(high[:, 1].min()) >= 1 << 31 and (high[:, 1] < high[:, 2]).all()
    u = engine.RegionUnion(n_seq)
    u.add(low)
    u.finish()
    _assert_spans(u.spans(), cd.merge_rows(low, n_seq))
    u.add(high)
    u.finish()
    _assert_spans(u.spans(), cd.merge_rows(np.concatenate([low, high]), n_seq))
    assert u.stats()["folds"] == 2
    u.close()


# ------------------------------------------------------------------------------------------------- C: state across folds
@pytest.mark.parametrize("n_seq,seqids", [(5, (0, 1, 2, 3)), (5, (2,)), (300, (0, 7, 255, 256, 299))])
def test_one_handle_through_growth_shrinking_and_its_own_spans(n_seq, seqids):
    """n_seq = 5: five sort passes, the result of the sort lands in the second buffer; 300: six, in the first."""
    assert 4 + cd.seqid_sort_passes(n_seq) == (5 if n_seq == 5 else 6)
    rng = np.random.default_rng(n_seq + len(seqids))

    def some(n, lo, hi):
        s = rng.integers(lo, hi, n)
        return cd.rows_of(rng.choice(seqids, n), s, s + rng.integers(1, 40, n))

    u, rows = engine.RegionUnion(n_seq), np.zeros((0, 3), np.uint32)

    def step(new):
        nonlocal rows
        rows = np.concatenate([rows, new])
        u.add(new)
        u.finish()
        want = cd.merge_rows(rows, n_seq)
        _assert_spans(u.spans(), want)
        return want

    step(some(10, 1000, 200000))
    assert len(step(some(5000, 1000, 200000))[1]) > 2000  # the capacity grows; the ten rows' spans are carried along
    step(np.array([[seqids[0], 500, 300000]], np.uint32))  # one row covering everything of its seqid
    want = step(cd.rows_of(np.array(seqids[1:], np.int64), np.full(len(seqids) - 1, 500), np.full(len(seqids) - 1, 300000)))
    assert u.n_spans == len(seqids) and want[1].tolist() == [500] * len(seqids)  # one span per seqid (one span in all: seqids == (2,))
    want = step(cd.rows_of(seqids[-1], np.array([300000, 300002, 400000]), np.array([300001, 300010, U32_MAX])))
    assert u.n_spans == len(seqids) + 2  # [300000, 300001) touches the big span, the other two are new
    folds = u.stats()["folds"]
    o, us, ue, _ = u.spans()
    u.add_spans(o, us, ue)  # its own spans: nothing may change
    u.finish()
    _assert_spans(u.spans(), want)
    assert u.stats()["folds"] == folds + 1 and u.stats()["rows"] == len(rows) + len(us)
    u.close()


def test_segment_buffers_regrow_between_calls():
    n_seq, rows = 3, cd.sort_plan_rows(3, "all_bytes", n=3000)
    u = _union(n_seq, rows)
    want = cd.merge_rows(rows, n_seq)
    rng = np.random.default_rng(3)
    for n in (10, 1000, 3, 0):
        q, a = rng.integers(0, n_seq, n), rng.integers(0, U32_MAX, n)
        b = np.minimum(a + rng.choice([1, 1 << 20, 1 << 31], n), U32_MAX)
        got = u.segments_covered(q, a, b)
        assert got.dtype == np.uint32 and np.array_equal(got, cd.covered(want, q, a, b))
    u.close()


# ------------------------------------------------------------------------------------------------------ D: the fold split
def test_one_add_of_more_than_a_fold():
    """8 Mi + 1025 rows in one add: two folds.  The one large case -- nothing else reaches gffx_hip_union_add_host's split."""
    rows = cd.fold_split_rows()
    assert len(rows) == cd.UNION_FOLD + 1025
    u = _union(3, rows)
    st = u.stats()
    assert st["folds"] == 2 and st["rows"] == len(rows)
    want = cd.merge_rows(rows, 3)
    assert u.n_spans == len(want[1]) < 1000
    _assert_spans(u.spans(), want)
    u.close()


# ----------------------------------------------------------------------------------------------- E: k_segments_covered
def _covered_both_ways(n_seq, rows, q, a, b):
    """RegionUnion.segments_covered (U built on the device) and the one-shot entry (U built on the host) == the definition."""
    spans = cd.merge_rows(rows, n_seq)
    want = cd.covered(spans, q, a, b)
    u = _union(n_seq, rows)
    _assert_spans(u.spans(), spans)
    got = u.segments_covered(q, a, b)
    u.close()
    bad = np.nonzero(got != want)[0]
    assert got.dtype == np.uint32 and not len(bad), (len(bad), [(int(q[i]), int(a[i]), int(b[i]), int(got[i]), int(want[i])) for i in bad[:5]])
    one = engine.segments_covered(q, a, b, rows, n_seq)
    bad = np.nonzero(one != want)[0]
    assert one.dtype == np.uint32 and not len(bad), (len(bad), [(int(q[i]), int(a[i]), int(b[i]), int(one[i]), int(want[i])) for i in bad[:5]])
    return want


@pytest.mark.parametrize("name", cd.DIRECTORY_CASES)
def test_directory_rule_and_span_edges(name):
    """Every pair of probe points (each span's start and end, every bin edge, each +- 1, 0 and 0xFFFFFFFF) as a segment."""
    n_seq, rows = cd.directory_case(name)
    spans = cd.merge_rows(rows, n_seq)
    q, a, b = cd.probe_segments(spans, n_seq)
    want = _covered_both_ways(n_seq, cd.place(rows, 2), q, a, b)
    assert int(want.max()) > 0
    if name == "starts_on_bin_edges":  # the documented rule gives 16 Mi-wide bins, and every start sits on one's edge
        shift, nb = cd.directory_rule(spans[1])
        assert (shift, nb) == (24, 14) and (spans[1] % (1 << shift) == 0).all() and len(set((spans[1] >> shift).tolist())) < nb
    if name == "more_than_2_31_bases":
        i = np.nonzero((q == 1) & (a == 0) & (b == U32_MAX))[0]
        assert len(i) == 1 and want[i[0]] == (1 << 32) - 11
    if name == "empty_first_bins":  # segments before the first span
        assert (want[(q == 1) & (b <= (1 << 30) + 5)] == 0).all() and np.count_nonzero((q == 1) & (b <= (1 << 30) + 5) & (a < b)) > 20
    if name == "spread_to_the_top":
        assert np.count_nonzero((b.astype(np.int64) - a.astype(np.int64)) > 1 << 31) > 1000  # segments wider than 2^31


@pytest.mark.parametrize("n_seg", [1, 255, 256, 257])
def test_many_seqids_and_block_edges_of_the_segment_count(n_seg):
    n_seq, with_spans = 65537, (0, 255, 65535, 65536)
    rng = np.random.default_rng(n_seg)
    s = rng.integers(0, U32_MAX - 5000, 400)
    rows = cd.rows_of(rng.choice(with_spans, 400), s, s + rng.integers(1, 5000, 400))
    q = rng.choice(with_spans + (1, 254, 256, 65534), n_seg)
    q[-1] = 65536
    a = rng.integers(0, U32_MAX, n_seg)
    b = np.minimum(a + rng.choice([1, 1 << 26, 1 << 31, U32_MAX], n_seg), U32_MAX)
    a[-1], b[-1] = 0, U32_MAX
    want = _covered_both_ways(n_seq, rows, q, a, b)
    assert (want[~np.isin(q, with_spans)] == 0).all() and want[-1] > 0
