"""The pileup's second consumer (gffx_hip_pileup_meta_*, engine.Pileup.meta_set / meta): the column totals and the features x
columns matrix of `gffx meta` == the sparse definition of tests/_meta_definition.py, bit for bit: on the hand example, at the
column counts where the wave's 63-column steps and the limit lie, at the feature counts around the kernel's tile, on seqids
without rows or without features, however the rows are grouped into adds or spread over handles, beside the pileup's segments,
against the explicit-segment route that existed before, and under the mirror law."""
import numpy as np
import pytest

import _meta_definition as md
import _pileup_definition as pd
from gffx_amd import engine

pytestmark = pytest.mark.gpu

E = engine._ffi.GffxHipError
BIG = md.U32_MAX


def _lay(t):
    return engine.MetaLayout(*t)


def _rows(seed, n, n_seq=3, span=60000, on=None):
    rng = np.random.default_rng(seed)
    r = np.empty((n, 3), np.uint32)
    r[:, 0] = rng.choice(on if on is not None else np.arange(n_seq), n)
    r[:, 1] = rng.integers(0, span, n)
    r[:, 2] = r[:, 1] + rng.choice([1, 30, 150, 2000], n) + rng.integers(0, 50, n)
    return r


def _feats(seed, n, n_seq=3, span=60000, on=None):
    rng = np.random.default_rng(500 + seed)
    f = np.empty((n, 4), np.uint32)
    f[:, 0] = rng.choice(on if on is not None else np.arange(n_seq), n)
    f[:, 1] = rng.integers(0, span, n)
    f[:, 2] = f[:, 1] + rng.choice([1, 2, 90, 1500, 20000], n)
    f[:, 3] = rng.integers(0, 2, n)
    return f


def _check(n_seq, rows, feats, lay, seq_len=None, pieces=None, matrix=True):
    """One pileup without segments: totals and matrix against the sparse definition."""
    feats = np.asarray(feats, np.uint32).reshape(-1, 4)
    want = md.sparse(n_seq, rows, feats, lay, seq_len)
    want_cols = md.totals(want, md.lens(feats, lay, seq_len))
    p = engine.Pileup(n_seq, [], [], [])
    assert p.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(lay), seq_len, keep_matrix=matrix) == md.columns(lay)
    for piece in (pieces if pieces is not None else [rows]):
        p.add(piece)
    got = p.meta(matrix=matrix)
    p.close()
    for g, w in zip(got[:3], want_cols):
        assert g.dtype == np.uint64 and np.array_equal(g, w), (np.nonzero(g != w)[0][:10], g[:8], w[:8])
    if matrix:
        assert got[3].shape == want.shape and np.array_equal(got[3], want), np.argwhere(got[3] != want)[:10]
    return got


@pytest.mark.parametrize("name", sorted(md.HAND))
def test_the_hand_example(name):
    lay, seq_len, bases, width, col_bases, col_len, col_features = md.HAND[name]
    cb, cl, cf, m = _check(md.HAND_N_SEQ, md.HAND_ROWS, md.HAND_FEATS, lay, seq_len)
    assert (m.tolist(), cb.tolist(), cl.tolist(), cf.tolist()) == (bases, col_bases, col_len, col_features)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 129, "cap"])
@pytest.mark.parametrize("mode", ["point", "scaled"])
def test_column_counts_at_the_wave_steps_and_the_limit(B, mode):
    cap = engine.meta_constants()[0]
    B = cap if B == "cap" else B
    rows = _rows(B % 97, 3000)
    feats = _feats(B % 97, 40)
    if mode == "point":
        lay = md.point(3 * (B // 2), 3 * (B - B // 2), 3, md.CENTER)
    else:
        lay = md.scaled(2 * (B // 3), 2 * (B // 3), 2, B - 2 * (B // 3))
    assert md.columns(lay) == B
    _check(3, rows, feats, lay)


def test_more_columns_than_the_limit_are_refused_and_the_handle_stays_usable():
    cap = engine.meta_constants()[0]
    rows, feats = _rows(1, 500), _feats(1, 10)
    p = engine.Pileup(3, [0], [0], [60000])
    for bad in (md.point(cap + 1, 0, 1), md.scaled(0, 0, 1, cap + 1), md.point(4, 4, 0), md.point(3, 4, 2), md.point(0, 0, 1), md.scaled(2, 2, 2, 0),
                md.point(4, 4, 2, 3), (2, 0, 4, 4, 2, 2)):
        with pytest.raises(E) as ei:
            p.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(bad))
        assert ei.value.code == -1
    for q, s, e in (([3], [1], [2]), ([0], [5], [5]), ([0], [9], [2])):  # a seqid out of range, an empty and an inverted feature
        with pytest.raises(E) as ei:
            p.meta_set(q, s, e, [0], _lay(md.point(4, 4, 2)))
        assert ei.value.code == -1
    with pytest.raises(E):
        p.meta()  # no features yet
    lay = md.point(cap, 0, 1)
    p.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(lay))
    p.add(rows)
    want = md.sparse(3, rows, feats, lay)
    assert np.array_equal(p.meta()[0], want.sum(0, dtype=np.uint64))
    with pytest.raises(E):
        p.meta(matrix=True)  # not kept
    assert np.array_equal(p.bases(), pd.brute(rows, [0], [0], [60000]))
    p.close()


@pytest.mark.parametrize("count", ["0", "1", "3", "tile - 1", "tile", "tile + 1", "5 * tile + 1"])
def test_feature_counts_around_the_tile(count):
    n = eval(count, {"tile": engine.meta_constants()[1]})
    rows = _rows(7, 4000)
    feats = _feats(n, n)
    for lay in (md.point(200, 200, 20), md.scaled(40, 40, 20, 11)):
        _check(3, rows, feats, lay)


def test_seqids_without_rows_without_features_and_mixed_inside_a_block():
    n_seq = 5
    rows = _rows(11, 5000, n_seq=n_seq, on=[0, 1, 3])  # 2 and 4: no rows
    feats = _feats(11, 150, n_seq=n_seq, on=[0, 2, 3, 4])  # 1: rows and no features; neighbours in the array lie on different seqids
    assert len(set(feats[:8, 0].tolist())) > 1
    cb, cl, cf, m = _check(n_seq, rows, feats, md.point(500, 500, 50))
    assert not m[np.isin(feats[:, 0], [2, 4])].any() and m[feats[:, 0] == 0].any() and m[feats[:, 0] == 3].any()
    # no rows at all: the lengths are there, the bases are 0
    cb, cl, cf = _check(n_seq, np.zeros((0, 3), np.uint32), feats, md.scaled(100, 100, 50, 9), matrix=False)
    assert not cb.any() and cl.all() and cf.all()


def test_features_out_of_coordinate_order_and_sorted_give_the_same_rows():
    rows = _rows(12, 6000)
    feats = _feats(12, 200)
    lay = md.scaled(300, 300, 30, 25)
    shuffled = _check(3, rows, feats, lay)
    order = np.lexsort((feats[:, 1], feats[:, 0]))
    by_coordinate = _check(3, rows, feats[order], lay)
    assert np.array_equal(shuffled[3][order], by_coordinate[3]) and np.array_equal(shuffled[0], by_coordinate[0])


def test_equal_starts_equal_ends_and_the_extremes():
    k = np.arange(300, dtype=np.uint32)
    rows = np.concatenate([np.stack([0 * k, 1000 + 0 * k, 1001 + k], axis=1), np.stack([0 * k, 2000 + k, 2500 + 0 * k], axis=1)]).astype(np.uint32)
    feats = np.array([(0, 1000, 1001, 0), (0, 1000, 1300, 1), (0, 999, 1000, 0), (0, 2400, 2500, 1), (0, 2500, 2501, 0), (0, 1001, 2499, 1)], np.uint32)
    for lay in (md.point(10, 10, 1), md.point(300, 300, 100, md.TES), md.scaled(3, 3, 1, 50)):
        _check(1, rows, feats, lay)
    # coordinates 0 and 2^32 - 1, with and without a length
    rows = np.array([(0, 0, BIG), (0, 0, 1), (0, BIG - 1, BIG), (0, BIG - 50, BIG), (0, 3, 4_000_000_000), (1, 0, 5)], np.uint32)
    feats = np.array([(0, 0, BIG, 0), (0, 0, BIG, 1), (0, 0, 1, 0), (0, 0, 1, 1), (0, BIG - 1, BIG, 0), (0, BIG - 1, BIG, 1), (0, BIG - 40, BIG, 1), (1, 0, 9, 0),
                      (0, 2 ** 31 - 3, BIG, 1)], np.uint32)
    for lay in (md.point(100, 100, 10), md.point(20, 20, 10, md.CENTER), md.scaled(20, 20, 10, 6), md.scaled(0, 0, 1, 1000)):
        _check(2, rows, feats, lay)
        _check(2, rows, feats, lay, seq_len=[BIG - 7, 4])


def test_column_totals_above_32_bits():
    rows = np.array([(0, 0, BIG)] * 5 + [(0, 10, 20)], np.uint32)
    feats = np.array([(0, 0, BIG, 0), (0, 0, BIG, 1), (0, 100, BIG - 100, 0)], np.uint32)
    cb, _, _, m = _check(1, rows, feats, md.scaled(0, 0, 1, 4))
    assert int(cb.min()) > 2 ** 32 and int(m.min()) > 2 ** 32


def test_one_add_many_adds_a_second_fold_and_two_handles():
    n = 9000
    rows, feats = _rows(21, n), _feats(21, 130)
    lay = md.point(400, 200, 20, md.TES)
    one = _check(3, rows, feats, lay)
    many = _check(3, rows, feats, lay, pieces=[rows[:1], rows[1:5001], rows[5001:5002], rows[5002:]])
    want = md.sparse(3, rows, feats, lay)
    h1, h2 = engine.Pileup(3, [], [], []), engine.Pileup(3, [], [], [])
    for h in (h1, h2):
        h.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(lay), keep_matrix=True)
    h1.add(rows[:2777]), h2.add(rows[2777:])
    a, b = h1.meta(matrix=True), h2.meta(matrix=True)
    h1.close(), h2.close()
    assert np.array_equal(a[3] + b[3], want) and np.array_equal(a[0] + b[0], one[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(many[3], want) and np.array_equal(many[0], one[0])


def test_more_rows_than_one_fold_through_one_add():
    n = engine.PILEUP_FOLD + 1
    rng = np.random.default_rng(5)
    rows = np.empty((n, 3), np.uint32)
    rows[:, 0] = rng.integers(0, 2, n)
    rows[:, 1] = rng.integers(0, 3_000_000_000, n)
    rows[:, 2] = rows[:, 1] + rng.integers(1, 2000, n)
    rows[-1] = (1, 77, 4_000_000_000)  # the one row of the second fold
    feats = np.array([(0, 1_000_000_000, 1_000_300_000, 0), (1, 2_000_000_000, 2_000_000_500, 1), (1, 70, 90, 0), (2, 5, 9, 1), (1, 3_999_999_990, 4_000_000_010, 1)],
                     np.uint32)
    lay = md.scaled(3000, 3000, 1000, 5)
    p = engine.Pileup(3, [], [], [])
    p.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(lay), keep_matrix=True)
    p.add(rows)
    got = p.meta(matrix=True)
    assert p.stats()["folds"] == 2 and p.meta_ms() > 0
    p.close()
    want = md.sparse(3, rows, feats, lay)
    assert np.array_equal(got[3], want) and np.array_equal(got[0], want.sum(0, dtype=np.uint64)) and want[2].any() and want[4].any()


def test_segments_and_meta_side_by_side_reset_and_the_explicit_segment_route():
    rows, other = _rows(31, 5000), _rows(32, 2500)
    feats = _feats(31, 90)
    lay = md.scaled(200, 100, 50, 13)
    seq_len = [60500, 61000, 59000]
    q, a, b = md.segments(feats, lay, seq_len)
    # the route that existed before: a pileup over the G x B explicit clamped columns
    explicit = engine.Pileup(3, q, a, b)
    explicit.add(rows)
    before = explicit.bases()
    # ... which the same handle still gives with features beside its segments, and which is the matrix
    explicit.reset()
    explicit.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(lay), seq_len, keep_matrix=True)
    explicit.add(rows)
    assert np.array_equal(explicit.bases(), before)
    cb, cl, cf, m = explicit.meta(matrix=True)
    assert np.array_equal(m.ravel(), before) and np.array_equal(m, md.sparse(3, rows, feats, lay, seq_len))
    assert np.array_equal(cl, (b - a).astype(np.uint64).reshape(len(feats), -1).sum(0, dtype=np.uint64))
    # without the matrix: the same column totals
    lean = engine.Pileup(3, [], [], [])
    lean.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], _lay(lay), seq_len)
    lean.add(rows)
    assert all(np.array_equal(x, y) for x, y in zip(lean.meta(), (cb, cl, cf)))
    lean.close()
    # reset: bases and matrix back to zero, lengths and features stay; then other rows
    explicit.reset()
    zb, zl, zf, zm = explicit.meta(matrix=True)
    assert not zb.any() and not zm.any() and not explicit.bases().any() and np.array_equal(zl, cl) and np.array_equal(zf, cf)
    explicit.add(other)
    assert np.array_equal(explicit.meta(matrix=True)[3], md.sparse(3, other, feats, lay, seq_len))
    assert np.array_equal(explicit.bases(), pd.closed_form(other, q, a, b))
    # new features replace the old ones and start from zero
    few = feats[:3]
    explicit.meta_set(few[:, 0], few[:, 1], few[:, 2], few[:, 3], _lay(md.point(40, 40, 20)), keep_matrix=True)
    assert not explicit.meta(matrix=True)[3].any()
    explicit.add(rows)
    assert np.array_equal(explicit.meta(matrix=True)[3], md.sparse(3, rows, few, md.point(40, 40, 20)))
    explicit.close()


@pytest.mark.parametrize("near_zero", [False, True])
def test_the_mirror_law_on_the_device(near_zero):
    C_ = 200000
    rows = _rows(41, 3000, span=3000 if near_zero else 60000)
    feats = _feats(41, 70, span=3000 if near_zero else 60000)
    feats[:, 1] += 0 if near_zero else 5000
    feats[:, 2] += 0 if near_zero else 5000
    m_rows, m_feats = md.mirror(rows, feats, C_)
    for lay in (md.point(1000, 500, 100), md.point(300, 300, 30, md.CENTER), md.scaled(600, 300, 100, 17)):
        here = _check(3, rows, feats, lay)
        there = _check(3, m_rows, m_feats, lay, seq_len=[C_] * 3)
        assert np.array_equal(here[3], there[3]) and np.array_equal(here[1], there[1])
        cut = (md.lens(feats, lay) < np.diff(np.array([md.offsets(lay, int(e) - int(s)) for _, s, e, _ in feats]), axis=1)).any()
        assert cut == near_zero
