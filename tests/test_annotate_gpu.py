"""The class map on the device through the C-ABI (engine.ClassMap): points, running sums, counts and class bytes are compared
bit for bit with the sparse restatement of the definition (tests/_annotate_definition.py), at the edges of every launch shape:
event counts around the scan tile, runs of equal keys and seqid changes at a tile edge, the sort's one, two and three seqid
bytes, 1 to 32 layers, any grouping of the rows, region counts around the wave and the block, both ways to hand regions in,
and the refusals."""
import numpy as np
import pytest

import _annotate_definition as ad
from gffx_amd import engine
from gffx_amd._ffi import GffxHipError

pytestmark = pytest.mark.gpu


def build(n_seq, T, rows, calls=None):
    m = engine.ClassMap(n_seq, T)
    rows = np.asarray(rows, np.uint32).reshape(-1, 4)
    for part in (calls if calls is not None else [rows]):
        m.add_rows(part)
    m.finish()
    return m


def device(n_seq, T, rows, regions, calls=None):
    m = build(n_seq, T, rows, calls)
    p_off, pos, cls = m.points()
    counts, best = m.run(regions)
    out = (p_off, pos, cls, m.bases(), counts, best)
    m.close()
    return out


def check(n_seq, T, rows, regions=None, calls=None):
    regions = ad.probe_regions(n_seq, T, rows) if regions is None else np.asarray(regions, np.uint32).reshape(-1, 3)
    want = ad.sparse(n_seq, T, rows, regions)
    got = device(n_seq, T, rows, regions, calls)
    for name, g, w in zip(("p_off", "pos", "cls", "cb", "counts", "class"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    return want


def test_the_hand_example():
    got = device(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ad.HAND_REGIONS)
    assert ad.same(got, ad.hand())
    check(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS)


def _event_counts():
    S, _, _ = engine._classmap_constants()
    # (a span gives two events, so an event count is even: the odd counts 1, S - 1, S + 1 and 2 S + 1 are taken from both sides)
    return sorted({2, S - 2, S, S + 2, 2 * S, 2 * S + 2})


def test_event_counts_around_the_scan_tile():
    for n in _event_counts():
        rows = ad.events_case(n, T=3)
        want = check(1, 3, rows)
        assert len(want[1]) >= n // 2  # every row is a span of its own


def test_runs_and_seqid_borders_at_a_tile_edge():
    S, _, _ = engine._classmap_constants()
    # 32 layers toggle at one position: the run of 32 equal keys lies across the edge between tile 0 and tile 1
    lead = ad.events_case(S - 16, T=32)  # S - 16 events before position P, all far below it
    P = 1 << 20
    run = np.array([[k, 0, P, P + 100 + k] for k in range(32)], np.uint32)
    check(1, 32, np.concatenate([lead, run]))
    # a close and an open of every layer at P: the tile's events cancel to mask 0 there and no point is written at P
    both = np.array([[k, 0, P - 50, P] for k in range(32)] + [[k, 0, P, P + 50] for k in range(32)], np.uint32)
    want = check(1, 32, np.concatenate([lead, both]))
    assert P not in want[1].tolist()
    # the seqid changes exactly at the tile edge: seqid 0 holds S events, seqid 1 the rest
    a, b = ad.events_case(S, T=2, seq=0), ad.events_case(S + 2, T=2, seq=1)
    check(2, 2, np.concatenate([a, b]))
    # a tile whose events cancel to mask 0 under a mask that is not 0: two long rows of layers 0 and 2 open first, S - 2 events
    # of layer 1 fill tile 0, and tile 1 holds S / 2 whole rows of layer 1.  The class is 0 all the way: two points
    i = np.arange(S - 1, dtype=np.int64)
    inner = np.stack([np.full(S - 1, 1), np.zeros(S - 1, np.int64), 10 + 7 * i, 13 + 7 * i], 1).astype(np.uint32)
    cover = np.array([[0, 0, 0, 1 << 20], [2, 0, 1, 1 << 20]], np.uint32)
    want = check(1, 3, np.concatenate([inner, cover]))
    assert want[1].tolist() == [0, 1 << 20] and want[2].tolist() == [0, 3]


@pytest.mark.parametrize("n_seq", [1, 257, 65537])
def test_the_sort_plan_by_seqid_bytes(n_seq):
    seqs = sorted({0, n_seq - 1, min(255, n_seq - 1), min(256, n_seq - 1), min(65536, n_seq - 1)})
    rng = np.random.default_rng(n_seq)
    rows = []
    for c in seqs:
        s = rng.integers(0, 1 << 31, 300)
        rows.append(np.stack([rng.integers(0, 5, 300), np.full(300, c), s, s + 1 + rng.integers(0, 1 << 20, 300)], 1))
    rows = np.concatenate(rows).astype(np.uint32)
    rows = rows[rng.permutation(len(rows))]
    check(n_seq, 5, rows)


@pytest.mark.parametrize("T", [1, 2, 5, 32])
def test_layer_counts_and_a_layer_without_rows(T):
    rng = np.random.default_rng(T)
    n = 400
    s = rng.integers(0, 20000, n)
    layer = rng.integers(0, T, n)
    if T > 1:
        layer[layer == T // 2] = 0  # layer T / 2 has no rows
    rows = np.stack([layer, rng.integers(0, 3, n), s, s + 1 + rng.integers(0, 300, n)], 1).astype(np.uint32)
    regions = np.stack([rng.integers(0, 3, 200), rng.integers(0, 21000, 200), rng.integers(0, 21000, 200)], 1).astype(np.uint32)
    want = check(3, T, rows, np.concatenate([regions, ad.probe_regions(3, T, rows)]))
    if T > 1:
        assert not want[4][:, T // 2].any()


def test_coordinates_at_both_ends_of_32_bits():
    rows = np.array([[1, 0, 0, 1], [0, 0, ad.U32_MAX - 1, ad.U32_MAX], [1, 0, 5, ad.U32_MAX], [0, 1, 0, ad.U32_MAX]], np.uint32)
    want = check(3, 2, rows)  # (seqid 2 has no points)
    assert want[3].max() >= (1 << 32)  # the running sums need their 64 bits


def test_the_grouping_of_the_rows_does_not_matter():
    n_seq, T, rows, regions = ad.random_case(7, n=120)
    rng = np.random.default_rng(3)
    one = check(n_seq, T, rows, regions)
    for calls in ([r[None, :] for r in rows], [rows[rng.permutation(len(rows))]], [np.repeat(rows, 2, 0)], [rows[:50], rows[50:51], rows[51:]]):
        got = device(n_seq, T, rows, regions, calls)
        assert ad.same(got, one)


def test_region_counts_around_the_wave_and_the_block():
    _, B, _ = engine._classmap_constants()
    n_seq, T, rows, _ = ad.random_case(11, n=100)
    rng = np.random.default_rng(5)
    m = build(n_seq, T, rows)
    for nq in sorted({0, 1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7}):  # (the kernel does not chunk: one thread per region, any grid)
        regions = np.stack([rng.integers(0, n_seq, nq), rng.integers(0, 320, nq), rng.integers(0, 320, nq)], 1).astype(np.uint32)
        want = ad.sparse(n_seq, T, rows, regions)
        counts, best = m.run(regions)
        assert counts.shape == (nq, T + 1) and np.array_equal(counts, want[4]) and np.array_equal(best, want[5])
    m.close()


def test_run_host_against_run_store():
    n_seq, T, rows, _ = ad.random_case(13, n=100)
    regions = ad.probe_regions(n_seq, T, rows)[:300]
    want = ad.sparse(n_seq, T, rows, regions)
    m = build(n_seq, T, rows)
    store = engine.RegionStore(0, len(regions) + 8, False)
    store.staging(1)[:len(regions)] = regions
    store.append(1, len(regions))
    counts, best = m.run_store(store, 1, 0, len(regions))
    assert np.array_equal(counts, want[4]) and np.array_equal(best, want[5])
    counts, best = m.run_store(store, 1, 5, 100)  # a slice that starts at an odd row
    assert np.array_equal(counts, want[4][5:105]) and np.array_equal(best, want[5][5:105])
    host = m.run(regions)
    assert np.array_equal(host[0], want[4]) and np.array_equal(host[1], want[5])
    with pytest.raises(GffxHipError) as e:
        m.run_store(store, 1, 0, len(regions) + 1)
    assert e.value.code == ad.E_INVALID
    assert np.array_equal(m.run(regions)[0], want[4])  # a refused argument leaves the object usable
    assert m.last_kernel_ms() > 0 and m.stage_ms()["sort_ms"] > 0
    store.close()
    m.close()


def test_a_region_on_a_seqid_out_of_range_is_refused_and_the_object_stays():
    m = build(2, 3, ad.HAND_ROWS)
    regions = ad.HAND_REGIONS.copy()
    regions[4, 0] = 2
    with pytest.raises(GffxHipError) as e:
        m.run(regions)
    assert e.value.code == ad.E_CHR_RANGE
    counts, best = m.run(ad.HAND_REGIONS)
    assert np.array_equal(counts, np.array(ad.HAND_COUNTS, np.uint32)) and best.tolist() == ad.HAND_CLASS
    m.close()


def test_a_run_before_finish_is_refused():
    m = engine.ClassMap(2, 3)
    m.add_rows(ad.HAND_ROWS)
    with pytest.raises(GffxHipError) as e:
        m.run(ad.HAND_REGIONS)
    assert e.value.code == ad.E_STATE
    with pytest.raises(GffxHipError) as e:
        m.points()
    assert e.value.code == ad.E_STATE
    m.finish()
    assert m.run(ad.HAND_REGIONS)[1].tolist() == ad.HAND_CLASS
    m.add_rows([[0, 1, 100, 200]])  # more rows: the map is stale until the next finish
    with pytest.raises(GffxHipError) as e:
        m.run(ad.HAND_REGIONS)
    assert e.value.code == ad.E_STATE
    m.finish()
    assert m.n_points == len(ad.HAND_POS) + 2
    m.close()


@pytest.mark.parametrize("bad,code", [([3, 0, 1, 2], ad.E_CHR_RANGE), ([0, 2, 1, 2], ad.E_CHR_RANGE), ([0, 0, 2, 2], ad.E_INVALID),
                                      ([0, 0, 3, 2], ad.E_INVALID), ([3, 0, 3, 2], ad.E_CHR_RANGE)])
def test_refused_rows_are_sticky(bad, code):
    m = engine.ClassMap(2, 3)
    m.add_rows(ad.HAND_ROWS)
    with pytest.raises(GffxHipError) as e:
        m.add_rows(np.concatenate([ad.HAND_ROWS, np.array([bad], np.uint32)]))
    assert e.value.code == code
    for call in (lambda: m.add_rows(ad.HAND_ROWS), m.finish, lambda: m.run(ad.HAND_REGIONS), m.points, m.bases):
        with pytest.raises(GffxHipError) as e:
            call()
        assert e.value.code == code and "failed earlier" in str(e.value)
    m.close()


def test_a_map_without_rows():
    m = engine.ClassMap(3, 4)
    m.finish()
    assert m.n_points == 0 and m.points()[0].tolist() == [0, 0, 0, 0] and m.bases().shape == (4, 0)
    counts, best = m.run([[0, 5, 25], [2, 0, ad.U32_MAX], [1, 9, 3]])
    assert counts.tolist() == [[0, 0, 0, 0, 20], [0, 0, 0, 0, ad.U32_MAX], [0, 0, 0, 0, 0]] and best.tolist() == [4, 4, 4]
    m.close()
