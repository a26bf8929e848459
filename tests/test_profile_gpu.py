"""The device depth profile (gffx_hip_profile_*, engine.DepthProfile): the canonical points == the sparse sweep of
tests/_profile_definition.py, at the row counts where the kernels change path (a thread, a wave, a scan tile, the carry
kernel's step, a fold), with runs of equal keys longer than a tile and seqid changes at tile edges, at the three sort plans,
however the rows are grouped into adds, stores or handles; the spans "depth >= T" against the definition and, at T = 1,
against the union builder; sum of depth x overlap against the device pileup; the refusals.  Everything is an integer and
compared for equality."""
import numpy as np
import pytest

import _profile_definition as pf
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


def _points(rows, n_seq, pieces=None):
    """(points, stats) of a fresh profile given the rows in `pieces` (default: one add)."""
    p = engine.DepthProfile(n_seq)
    for piece in (pieces if pieces is not None else [rows]):
        p.add(piece)
    p.finish()
    got, st = p.points(), p.stats()
    assert p.n_points == len(got[1])
    p.close()
    return got, st


def _check(rows, n_seq, pieces=None, want=None):
    want = pf.sweep_np(rows, n_seq) if want is None else want
    got, st = _points(rows, n_seq, pieces)
    assert pf.same(got, want), [np.nonzero(a != b)[0][:5] if a.shape == b.shape else (a.shape, b.shape) for a, b in zip(got, want)]
    assert st["rows"] == len(rows)
    return got, st


def _row_counts():
    tile = engine.PROFILE_SCAN_TILE
    # 2 x rows events: 128 tiles hold 256 tiles' worth of events, so the tile sums cross the carry kernel's step of 256 once
    return [1, 2, 63, 64, 65, tile // 2 - 1, tile // 2, tile // 2 + 1, tile - 1, tile, tile + 1, 2 * tile + 1, 128 * tile - 1, 128 * tile + 1]


@pytest.mark.parametrize("i", range(14))
def test_row_counts_at_the_kernels_edges(i):
    n = _row_counts()[i]
    rows = _rows(i, n, span=20000 if n < 50000 else 4_000_000)
    want = pf.sweep_np(rows, N_SEQ)
    if n <= 3000:
        assert pf.same(want, pf.sweep(rows, N_SEQ))
    _, st = _check(rows, N_SEQ, want=want)
    assert st["folds"] == 1


@pytest.mark.parametrize("name", sorted(pf.HAND))
def test_the_hand_shapes(name):
    n_seq, rows = pf.HAND[name]
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    got, _ = _check(rows, n_seq, want=pf.sweep(rows, n_seq))
    if name in pf.BY_HAND:
        assert pf.same(got, pf.hand_points(name))


def test_more_rows_than_one_fold_through_one_add():
    n = engine.PROFILE_FOLD + 1
    rng = np.random.default_rng(5)
    rows = np.empty((n, 3), np.uint32)
    rows[:, 0] = rng.integers(0, 2, n)
    rows[:, 1] = rng.integers(0, 3_000_000_000, n)
    rows[:, 2] = rows[:, 1] + rng.integers(1, 2000, n)
    rows[-1] = (1, 77, 4_000_000_000)  # the one row of the second fold lies over every carried point of seqid 1
    got, st = _check(rows, 3)
    assert st["folds"] == 2 and len(got[1]) > n


def test_a_run_of_equal_keys_longer_than_a_tile():
    tile = engine.PROFILE_SCAN_TILE
    k = np.arange(3 * tile, dtype=np.uint32)
    rows = np.stack([0 * k + 1, 500 + 0 * k, 501 + k % 7], axis=1).astype(np.uint32)  # 3 tiles of equal starts, a few distinct ends
    rows = np.concatenate([np.array([[0, 10, 20], [1, 400, 500], [1, 100, 600]], np.uint32), rows, np.array([[2, 5, 6]], np.uint32)])
    got, _ = _check(rows, 3, want=pf.sweep(rows, 3))
    assert int(got[2].max()) == 3 * tile + 1
    # ... and 3 x tile equal rows: the starts are one run, the ends another, two points in all
    same = np.tile(np.array([[0, 7, 9]], np.uint32), (3 * tile, 1))
    got, _ = _check(same, 1)
    assert [x.tolist() for x in got] == [[0, 2], [7, 9], [3 * tile, 0]]


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_a_seqid_change_at_a_tile_edge(shift):
    # Seqid 0 gets exactly tile + shift records in the second fold.  Rows bring two records each; an odd count needs carried
    # points, which bring one each: the rows [0, 10) and [0, 20) leave three (0: 2, 10: 1, 20: 0).
    tile = engine.PROFILE_SCAN_TILE
    first = np.array([[0, 0, 10], [0, 0, 20]] if shift else [[1, 0, 5]], np.uint32)
    carried = 3 if shift else 0
    n0 = (tile + shift - carried) // 2
    assert 2 * n0 + carried == tile + shift
    i = np.arange(n0, dtype=np.uint32)
    a = np.stack([0 * i, 100 + 10 * i, 100 + 10 * i + 15], axis=1)  # overlapping neighbours: every record is a point
    b = np.stack([0 * i + 1, 100 + 7 * i, 100 + 7 * i + 3], axis=1)
    second = np.ascontiguousarray(np.concatenate([b, a]), dtype=np.uint32)
    rows = np.concatenate([first, second])
    _, st = _check(rows, 2, pieces=[first, second], want=pf.sweep(rows, 2))
    assert st["folds"] == 2


@pytest.mark.parametrize("n_seq", [1, 256, 257, 65537])
def test_the_three_sort_plans_with_rows_on_the_first_and_the_last_seqid(n_seq):
    on = np.unique([0, n_seq // 2, n_seq - 1])
    rows = _rows(n_seq, 6000, n_seq=n_seq, on=on)
    rows[5:40, 0] = n_seq - 1
    rows[40:60, 0] = 0
    got, _ = _check(rows, n_seq, want=pf.sweep(rows, n_seq))
    assert got[0][1] > 0 and got[0][n_seq] > got[0][n_seq - 1]


def test_any_grouping_gives_the_same_points():
    n = 10000
    rows = _rows(31, n)
    want = pf.sweep(rows, N_SEQ)
    one, _ = _check(rows, N_SEQ, want=want)
    three, st = _check(rows, N_SEQ, pieces=[rows[:1], rows[1:6001], rows[6001:]], want=want)
    assert st["folds"] == 3
    shuffled, _ = _check(rows[np.random.default_rng(1).permutation(n)], N_SEQ, want=want)
    # from both slots of a region store; slot 1 in two parts, the second starting at a row that is no multiple of four
    store = engine.RegionStore(0, 6000, False)
    p = engine.DepthProfile(N_SEQ)
    store.staging(0)[:6000] = rows[:6000]
    store.append(0, 6000)
    p.add_store(store, 0, 0, 6000)
    p.finish()
    assert pf.same(p.points(), pf.sweep(rows[:6000], N_SEQ))  # after every step
    store.staging(1)[:4000] = rows[6000:]
    store.append(1, 4000)
    p.add_store(store, 1, 0, 1001)
    p.finish()
    assert pf.same(p.points(), pf.sweep(rows[:7001], N_SEQ))
    p.add_store(store, 1, 1001, 2999)
    with pytest.raises(E) as ei:
        p.add_store(store, 1, 1, 4000)  # beyond the last append from buffer 1: a refused argument, the profile stays usable
    assert ei.value.code == -1
    p.finish()
    stored = p.points()
    store.wait_staging(0), store.wait_staging(1)
    p.close(), store.close()
    # two handles, each with a share of the rows, merged with add_points (either way round, and into an empty one)
    h1, h2, h3 = engine.DepthProfile(N_SEQ), engine.DepthProfile(N_SEQ), engine.DepthProfile(N_SEQ)
    h1.add(rows[:3333]), h2.add(rows[3333:])
    h1.finish(), h2.finish()
    p1, p2 = h1.points(), h2.points()
    assert pf.same(p1, pf.sweep(rows[:3333], N_SEQ)) and pf.same(p2, pf.sweep(rows[3333:], N_SEQ))
    h1.add_points(*p2)
    h1.finish()
    merged = h1.points()
    h3.add_points(*p2)
    h3.finish()
    assert pf.same(h3.points(), p2)
    h3.add_points(*p1)
    h3.finish()
    merged_other_way = h3.points()
    h3.add_points(np.zeros(N_SEQ + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))  # no points: nothing changes
    h3.finish()
    assert pf.same(h3.points(), want)
    h1.close(), h2.close(), h3.close()
    for got in (one, three, shuffled, stored, merged, merged_other_way):
        assert pf.same(got, want)


def test_reset_and_finishing_again():
    rows, other = _rows(41, 3000), _rows(42, 2000)
    p = engine.DepthProfile(N_SEQ)
    p.finish()
    assert p.n_points == 0 and [len(x) for x in p.points()] == [N_SEQ + 1, 0, 0]
    for _ in range(2):  # reset, then the same again
        p.add(rows[:1200])
        p.finish()
        p.finish()
        assert pf.same(p.points(), pf.sweep(rows[:1200], N_SEQ)) and pf.same(p.points(), p.points())
        p.add(rows[1200:])  # finish -> add -> finish
        with pytest.raises(E) as ei:
            p.points()
        assert ei.value.code == -6
        p.finish()
        assert pf.same(p.points(), pf.sweep(rows, N_SEQ))
        p.reset()
        with pytest.raises(E) as ei:
            p.points()
        assert ei.value.code == -6
        p.finish()
        assert p.n_points == 0 and int(p.points()[0][-1]) == 0
    p.add(other)
    p.finish()
    assert pf.same(p.points(), pf.sweep(other, N_SEQ))
    st = p.stats()
    assert st["rows"] == 8000 and st["folds"] == 5 and st["kernel_ms"] > 0
    assert abs(st["kernel_ms"] - (st["events_ms"] + st["sort_ms"] + st["scan_ms"] + st["points_ms"])) < 1e-6
    p.close()
    for call in (lambda: p.add(other), p.finish, p.points, p.reset, p.stats, lambda: p.union_at_least(1)):
        with pytest.raises(E) as ei:  # use after close: the handle is gone, the call is refused
            call()
        assert ei.value.code == -1


def _segments(points, n_seq):
    """Segments that begin and end on points, inside runs and outside every run, plus an empty and an inverted one."""
    q, a, b = [], [], []
    p_off, pos, _ = points
    for c in range(n_seq):
        ps = [int(x) for x in pos[int(p_off[c]):int(p_off[c + 1])]][:60]
        for lo, hi in zip(ps, ps[1:]):
            for s, e in ((lo, hi), (lo, min(hi + 3, pf.U32_MAX)), (max(lo - 2, 0), hi), (lo + (hi - lo) // 2, hi), (lo, lo), (hi, lo)):
                q.append(c), a.append(s), b.append(e)
        q.append(c), a.append(0), b.append(pf.U32_MAX)
        q.append(c), a.append(3_000_000_000), b.append(3_000_000_100)  # outside every run
    return np.array(q, np.uint32), np.array(a, np.uint32), np.array(b, np.uint32)


@pytest.mark.parametrize("name", ["random", "nested", "cancelling", "equal_starts", "seqid_without_rows", "extremes", "many_spans"])
def test_thresholds_against_the_definition_and_the_union(name):
    if name == "random":
        n_seq, rows = N_SEQ, _rows(61, 5000)
    elif name == "many_spans":  # more spans than one tile of points, on two seqids: the span kernels' scan and carry
        i = np.arange(3 * engine.PROFILE_SCAN_TILE, dtype=np.uint32)
        n_seq, rows = 3, np.concatenate([np.stack([i % 2 * 2, 10 * i, 10 * i + 4], axis=1), np.stack([i % 2 * 2, 10 * i + 2, 10 * i + 7], axis=1)]).astype(np.uint32)
    else:
        n_seq, rows = pf.HAND[name]
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    want = pf.sweep_np(rows, n_seq)
    p = engine.DepthProfile(n_seq)
    with pytest.raises(E) as ei:
        p.union_at_least(1)  # before finish
    assert ei.value.code == -6
    p.add(rows)
    p.finish()
    assert pf.same(p.points(), want)
    q, a, b = _segments(want, n_seq)
    top = pf.max_depth(want)
    for T in sorted({1, 2, top, top + 1}):
        u = p.union_at_least(T)
        spans = pf.spans_at_least(want, T)
        got = u.spans()
        assert u.n_spans == len(spans[1]) and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, spans)), T
        if T == top + 1:
            assert u.n_spans == 0
        assert np.array_equal(u.segments_covered(q, a, b).astype(np.uint64), pf.covered_at_least(want, T, q, a, b)), T
        if T == 1:  # the union builder on the same rows: u_off, us, ue, pb
            ru = engine.RegionUnion(n_seq)
            ru.add(rows)
            ru.finish()
            assert all(np.array_equal(g, w) for g, w in zip(got, ru.spans()))
            assert np.array_equal(u.segments_covered(q, a, b), ru.segments_covered(q, a, b))
            ru.close()
        u.close()
    with pytest.raises(E) as ei:
        p.union_at_least(0)
    assert ei.value.code == -1
    u = p.union_at_least(1)  # T == 0 was a refused argument: the profile is as usable as before
    assert u.n_spans == len(pf.spans_at_least(want, 1)[1])
    p.close()
    assert u.n_spans == len(pf.spans_at_least(want, 1)[1])  # the union is the caller's and outlives the profile
    u.close()


def test_depth_times_overlap_is_the_pileup():
    rows = _rows(71, 4000)
    points, _ = _check(rows, N_SEQ)
    q, a, b = _segments(points, N_SEQ)
    pile = engine.Pileup(N_SEQ, q, a, b)
    pile.add(rows)
    bases = pile.bases()
    pile.close()
    p_off, pos, dep = points
    got = np.zeros(len(q), np.uint64)
    for c in range(N_SEQ):
        lo, hi = int(p_off[c]), int(p_off[c + 1])
        if hi - lo < 2:
            continue
        s, e, d = pos[lo:hi - 1].astype(np.int64), pos[lo + 1:hi].astype(np.int64), dep[lo:hi - 1].astype(np.int64)
        for i in np.nonzero(q == c)[0]:
            got[i] = (d * np.clip(np.minimum(e, int(b[i])) - np.maximum(s, int(a[i])), 0, None)).sum()
    assert np.array_equal(got, bases) and bases.sum() > 0


@pytest.mark.parametrize("bad,code", [(np.array([[1, 7, 7]], np.uint32), -1), (np.array([[0, 9, 3]], np.uint32), -1),
                                      (np.array([[0, 1, 5], [3, 1, 2]], np.uint32), -5), (np.array([[1, 7, 7], [5, 1, 2]], np.uint32), -5)])
def test_refused_rows_match_the_union_builders_and_stick(bad, code):
    ok = np.array([[0, 1, 5], [2, 3, 9]], np.uint32)
    u = engine.RegionUnion(3)
    with pytest.raises(E) as want:
        u.add(bad)
    u.close()
    p = engine.DepthProfile(3)
    p.add(ok)
    with pytest.raises(E) as ei:
        p.add(bad)
    assert ei.value.code == want.value.code == code  # (range first when both are there)
    for call in (lambda: p.add(ok), p.finish, p.points, p.reset, lambda: p.union_at_least(1)):  # the object only reports the error again
        with pytest.raises(E) as again:
            call()
        assert again.value.code == code
    p.close()
    p = engine.DepthProfile(3)  # ... and a fresh one is not affected
    p.add(ok)
    p.finish()
    assert [x.tolist() for x in p.points()] == [[0, 2, 2, 4], [1, 5, 3, 9], [1, 0, 1, 0]]
    p.close()


NOT_CANONICAL = {
    "positions_not_ascending": ([0, 3, 3], [5, 4, 9], [1, 2, 0]),
    "equal_positions": ([0, 3, 3], [5, 5, 9], [1, 2, 0]),
    "last_depth_not_0": ([0, 2, 2], [5, 9], [1, 2]),
    "last_depth_not_0_before_another_seqid": ([0, 1, 3], [5, 5, 9], [1, 1, 0]),
    "first_depth_0": ([0, 2, 2], [5, 9], [0, 0]),
    "first_depth_0_on_the_second_seqid": ([0, 2, 4], [5, 9, 1, 3], [1, 0, 0, 0]),
    "two_equal_depths": ([0, 3, 3], [5, 7, 9], [2, 2, 0]),
    "p_off_not_monotone": ([0, 2, 1], [5, 9], [1, 0]),
    "p_off_not_from_0": ([1, 2, 2], [5, 9], [1, 0]),
}


@pytest.mark.parametrize("name", sorted(NOT_CANONICAL))
def test_points_that_are_not_canonical_are_refused(name):
    p_off, pos, dep = NOT_CANONICAL[name]
    p = engine.DepthProfile(2)
    p.add(np.array([[0, 1, 5]], np.uint32))
    h = engine._ffi
    o, a, b = np.array(p_off, np.uint64), np.array(pos, np.uint32), np.array(dep, np.uint32)
    rc = h.lib().gffx_hip_profile_add_points(p._h, o.ctypes.data_as(h.u64p), a.ctypes.data_as(h.u32p), b.ctypes.data_as(h.u32p))
    assert rc == -1 and b"gffx_hip_profile_add_points" in h.lib().gffx_hip_last_error()
    with pytest.raises(E) as ei:  # refused points are data, not an argument: the object has failed
        p.finish()
    assert ei.value.code == -1
    p.close()


def test_a_refused_argument_leaves_the_profile_usable():
    rows = np.array([[0, 1, 5], [1, 3, 9]], np.uint32)
    p = engine.DepthProfile(2)
    p.add(rows)
    L, h = engine._ffi.lib(), engine._ffi
    assert L.gffx_hip_profile_add_host(p._h, None, 3) == -1  # NULL rows
    assert L.gffx_hip_profile_add_points(p._h, None, None, None) == -1
    out = h.vp()
    assert L.gffx_hip_profile_union_at_least(p._h, 1, None) == -1
    p.finish()
    assert L.gffx_hip_profile_union_at_least(p._h, 0, h.C.byref(out)) == -1 and not out.value
    # every pointer of copy_points may be NULL
    assert L.gffx_hip_profile_copy_points(p._h, None, None, None) == 0
    assert [x.tolist() for x in p.points()] == [[0, 2, 4], [1, 5, 3, 9], [1, 0, 1, 0]]
    p.add(np.zeros((0, 3), np.uint32))  # no rows: nothing happens, the profile stays finished
    assert [x.tolist() for x in p.points()] == [[0, 2, 4], [1, 5, 3, 9], [1, 0, 1, 0]]
    p.close()
