"""The device pileup (gffx_hip_pileup_*, engine.Pileup): the bases the rows lay on every segment == the brute-force sum of
tests/_pileup_definition.py, at the row counts where the kernels change path (a wave, a block, a sort tile, a prefix-sum
tile, a fold), at the three sort plans, however the rows are grouped into adds or spread over handles, and against the
union builder's covered bases on the same rows.  Everything is an integer and compared for equality."""
import numpy as np
import pytest

import _pileup_definition as pd
from gffx_amd import engine

pytestmark = pytest.mark.gpu

E = engine._ffi.GffxHipError
N_SEQ = 3


def _rows(seed, n, n_seq=N_SEQ, span=20000, on=None):
    """n rows with start < end; seqids drawn from `on` (default: all but the last, which stays without rows)."""
    rng = np.random.default_rng(seed)
    r = np.empty((n, 3), np.uint32)
    r[:, 0] = rng.choice(on if on is not None else np.arange(max(n_seq - 1, 1)), n)
    r[:, 1] = rng.integers(0, span, n)
    r[:, 2] = r[:, 1] + rng.choice([1, 30, 500, 4000], n) + rng.integers(0, 50, n)
    if n > 3:  # a touching pair, a duplicate, equal starts
        r[1] = (r[0, 0], r[0, 2], r[0, 2] + 10)
        r[2] = r[0]
        r[3] = (r[0, 0], r[0, 1], r[0, 2] + 7)
    return r


def _segs(seed, n, rows, n_seq=N_SEQ, span=20000, on=None):
    rng = np.random.default_rng(1000 + seed)
    q = rng.choice(on if on is not None else np.arange(n_seq), n).astype(np.uint32)
    a = rng.integers(0, span + 3000, n).astype(np.uint32)
    b = (a + rng.choice([0, 1, 100, 5000, 30000], n)).astype(np.uint32)
    k = min(n, len(rows))
    if k:  # segments that are rows, and ones that touch a row at either end
        q[:k], a[:k], b[:k] = rows[:k, 0], rows[:k, 1], rows[:k, 2]
    for j in range(min(n, len(rows)) // 3):
        if j % 2:
            a[j], b[j] = rows[j, 2], rows[j, 2] + 9
        elif rows[j, 1] >= 9:
            a[j], b[j] = rows[j, 1] - 9, rows[j, 1]
    return q, a, b


def _check(rows, n_seq, q, a, b, pieces=None):
    want = pd.brute(rows, q, a, b)
    p = engine.Pileup(n_seq, q, a, b)
    for piece in (pieces if pieces is not None else [rows]):
        p.add(piece)
    got = p.bases()
    st = p.stats()
    p.close()
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert st["rows"] == len(rows)
    return got, st


def _row_counts():
    tile = engine.PILEUP_SCAN_TILE
    return [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, tile - 1, tile, tile + 1, 2 * tile + 1]


@pytest.mark.parametrize("i", range(14))
def test_row_counts_at_the_kernels_edges(i):
    n = _row_counts()[i]
    rows = _rows(i, n)
    q, a, b = _segs(i, 300, rows)
    _, st = _check(rows, N_SEQ, q, a, b)
    assert st["folds"] == 1


@pytest.mark.parametrize("per_seq", [(0, 0, 0), (1, 0, 0), (2, 1, 0), (1, 2, 1), (2, 2, 2), (0, 0, 2)])
def test_zero_one_and_two_rows_per_seqid(per_seq):
    rows = np.array([(c, 100 + 40 * k, 100 + 40 * k + 70) for c, n in enumerate(per_seq) for k in range(n)], np.uint32).reshape(-1, 3)
    q = np.repeat(np.arange(3, dtype=np.uint32), 4)
    a = np.tile(np.array([0, 100, 139, 170], np.uint32), 3)
    b = np.tile(np.array([101, 170, 141, 400], np.uint32), 3)
    got, st = _check(rows, 3, q, a, b)
    assert st["folds"] == (1 if len(rows) else 0)
    if per_seq == (2, 1, 0):
        assert got.tolist() == [1, 100, 3, 40, 1, 70, 2, 0, 0, 0, 0, 0]


def test_more_rows_than_one_fold_through_one_add():
    n = engine.PILEUP_FOLD + 1
    rng = np.random.default_rng(5)
    rows = np.empty((n, 3), np.uint32)
    rows[:, 0] = rng.integers(0, 2, n)
    rows[:, 1] = rng.integers(0, 3_000_000_000, n)  # (sums of 2^22 such starts pass 2^53: u64, not doubles)
    rows[:, 2] = rows[:, 1] + rng.integers(1, 2000, n)
    rows[-1] = (1, 77, 4_000_000_000)  # the one row of the second fold
    q = np.array([0, 1, 1, 2, 0, 1], np.uint32)
    a = np.array([0, 0, 1_000_000_000, 0, 2_999_999_999, 78], np.uint32)
    b = np.array([3_000_002_000, pd.U32_MAX, 1_000_500_000, pd.U32_MAX, 3_000_000_001, 79], np.uint32)
    _, st = _check(rows, 3, q, a, b)
    assert st["folds"] == 2


@pytest.mark.parametrize("n_seg", [0, 1, 255, 256, 257])
def test_segment_counts_at_the_block_edge(n_seg):
    rows = _rows(20 + n_seg, 1000)
    q, a, b = _segs(n_seg, n_seg, rows)
    _check(rows, N_SEQ, q, a, b)


@pytest.mark.parametrize("n_seq", [1, 2, 256, 257, 65537])
def test_the_three_sort_plans_with_work_on_the_last_seqid(n_seq):
    on = np.unique([0, n_seq // 2, n_seq - 1])
    rows = _rows(n_seq, 6000, n_seq=n_seq, on=on)
    rows[5:40, 0] = n_seq - 1
    q, a, b = _segs(n_seq, 400, rows, n_seq=n_seq, on=np.unique([0, n_seq // 3, n_seq // 2, n_seq - 1]))
    q[-3:] = n_seq - 1
    got, _ = _check(rows, n_seq, q, a, b)
    assert got[q == n_seq - 1].sum() > 0


@pytest.mark.parametrize("name", sorted(pd.HAND))
def test_the_hand_shapes(name):
    n_seq, rows, (q, a, b) = pd.HAND[name]
    _check(np.ascontiguousarray(rows, dtype=np.uint32), n_seq, q, a, b)


def test_additivity_over_adds_stores_and_handles():
    n = 10000
    rows = _rows(31, n)
    q, a, b = _segs(31, 700, rows)
    want = pd.brute(rows, q, a, b)
    one, _ = _check(rows, N_SEQ, q, a, b)
    three, st = _check(rows, N_SEQ, q, a, b, pieces=[rows[:1], rows[1:6001], rows[6001:]])
    assert st["folds"] == 3
    # from both slots of a region store; slot 1 in two parts, the second starting at a row that is no multiple of four
    store = engine.RegionStore(0, 6000, False)
    p = engine.Pileup(N_SEQ, q, a, b)
    store.staging(0)[:6000] = rows[:6000]
    store.append(0, 6000)
    p.add_store(store, 0, 0, 6000)
    store.staging(1)[:4000] = rows[6000:]
    store.append(1, 4000)
    p.add_store(store, 1, 0, 1001)
    p.add_store(store, 1, 1001, 2999)
    with pytest.raises(E) as ei:
        p.add_store(store, 1, 1, 4000)  # beyond the last append from buffer 1
    assert ei.value.code == -1
    stored = p.bases()
    store.wait_staging(0), store.wait_staging(1)
    p.close(), store.close()
    # two handles, each with a share of the rows, summed
    h1, h2 = engine.Pileup(N_SEQ, q, a, b), engine.Pileup(N_SEQ, q, a, b)
    h1.add(rows[:3333]), h2.add(rows[3333:])
    summed = h1.bases() + h2.bases()
    h1.close(), h2.close()
    for got in (one, three, stored, summed):
        assert got.dtype == np.uint64 and np.array_equal(got, want)


def test_running_totals_and_reset():
    rows = _rows(41, 3000)
    other = _rows(42, 2000)
    q, a, b = _segs(41, 300, rows)
    p = engine.Pileup(N_SEQ, q, a, b)
    assert not p.bases().any()
    p.add(rows[:1200])
    first = p.bases()
    assert np.array_equal(first, pd.brute(rows[:1200], q, a, b)) and np.array_equal(p.bases(), first)  # read twice
    p.add(rows[1200:])
    assert np.array_equal(p.bases(), pd.brute(rows, q, a, b))
    p.reset()
    assert not p.bases().any()
    p.add(other)
    assert np.array_equal(p.bases(), pd.brute(other, q, a, b))
    st = p.stats()
    assert st["rows"] == 5000 and st["folds"] == 3 and st["kernel_ms"] > 0
    assert abs(st["kernel_ms"] - (st["keys_ms"] + st["sorts_ms"] + st["scan_ms"] + st["segments_ms"])) < 1e-6
    p.close()
    for call in (lambda: p.add(other), p.bases, p.reset, p.stats):
        with pytest.raises(E) as ei:  # use after close: the handle is gone, the call is refused
            call()
        assert ei.value.code == -1


@pytest.mark.parametrize("bad", [np.array([[0, 1, 5], [3, 1, 2]], np.uint32), np.array([[1, 7, 7]], np.uint32),
                                 np.array([[0, 9, 3]], np.uint32), np.array([[1, 7, 7], [5, 1, 2]], np.uint32)])
def test_refusals_match_the_union_builders_and_stick(bad):
    ok = np.array([[0, 1, 5], [2, 3, 9]], np.uint32)
    u = engine.RegionUnion(3)
    with pytest.raises(E) as want:
        u.add(bad)
    u.close()
    p = engine.Pileup(3, [0, 2], [0, 0], [100, 100])
    p.add(ok)
    with pytest.raises(E) as ei:
        p.add(bad)
    assert ei.value.code == want.value.code and ei.value.code in (-1, -5)
    for call in (lambda: p.add(ok), p.bases, p.reset):  # the object only reports the error again
        with pytest.raises(E) as again:
            call()
        assert again.value.code == ei.value.code
    p.close()
    p = engine.Pileup(3, [0, 2], [0, 0], [100, 100])  # ... and a fresh one is not affected
    p.add(ok)
    assert p.bases().tolist() == [4, 6]
    p.close()
    with pytest.raises(E) as ei:
        engine.Pileup(3, [3], [0], [1])
    assert ei.value.code == -1


def test_covered_bases_never_exceed_the_pileup():
    rows = _rows(51, 600, span=400000)
    q, a, b = _segs(51, 2000, rows, span=400000)
    u = engine.RegionUnion(N_SEQ)
    u.add(rows)
    u.finish()
    covered = u.segments_covered(q, a, b).astype(np.uint64)
    u.close()
    bases, _ = _check(rows, N_SEQ, q, a, b)
    assert np.all(covered <= bases) and np.any(covered < bases) and np.any((covered == bases) & (bases > 0))
    # rows of a seqid that do not overlap one another (tiled end to end, and with gaps): covered == bases everywhere
    rng = np.random.default_rng(52)
    parts = []
    for c in range(2):
        edges = np.cumsum(rng.integers(1, 300, 3001))
        keep = rng.random(3000) < 0.7
        parts.append(np.stack([np.full(3000, c), edges[:-1], edges[1:]], axis=1)[keep])
    flat = np.ascontiguousarray(rng.permutation(np.concatenate(parts)), dtype=np.uint32)
    q, a, b = _segs(53, 1500, flat, span=450000)
    u = engine.RegionUnion(N_SEQ)
    u.add(flat)
    u.finish()
    covered = u.segments_covered(q, a, b).astype(np.uint64)
    u.close()
    bases, _ = _check(flat, N_SEQ, q, a, b)
    assert np.array_equal(covered, bases) and bases.sum() > 0
