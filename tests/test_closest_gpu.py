"""The device side of `gffx closest` (gffx_hip_closest_*, engine.Closest) against the brute-force definition of
tests/_closest_definition.py: the end table against a stable sort, the hand cases and a random set under all six flag
combinations through _run_host and _run_store, the region counts where the launch changes shape, pair buffers that must grow,
more seqids than the LDS staging holds, a seqid out of range, and handles that are reused.  Everything is an integer and
compared for equality."""
import numpy as np
import pytest

import _closest_definition as cd
from gffx_amd import engine

pytestmark = pytest.mark.gpu

E = engine._ffi.GffxHipError
META_LDS_SEQIDS = 24 * 1024 // 16  # kMetaLdsBytes / 16 (device/gffx_device.hpp)


def _index(n_seq, roots, device=0):
    co, s, e, f = cd.index_arrays(n_seq, roots)
    return engine.TreeIndexData.from_roots(co, s, e, f, device=device)


def _same(got, want, what=""):
    counts, offsets, triples, gaps = got
    w_counts, w_offsets, w_triples, w_gaps = want[:4]
    assert counts.dtype == np.uint32 and offsets.dtype == np.uint64 and triples.dtype == np.uint32 and gaps.dtype == np.uint32
    assert np.array_equal(counts, w_counts), (what, np.nonzero(counts != w_counts)[0][:10])
    assert np.array_equal(offsets, w_offsets), what
    assert triples.shape == w_triples.shape and np.array_equal(triples, w_triples), (what, np.nonzero((triples != w_triples).any(axis=1))[0][:10])
    live = w_counts > 0  # (a gap is undefined where the count is 0)
    assert np.array_equal(gaps[live], w_gaps[live]), what


def _via_store(cl, regions, combo, device=0):
    regions = np.asarray(regions, np.uint32).reshape(-1, 3)
    store = engine.RegionStore(0, max(len(regions), 1) + 5, False, device)
    # (rows in front of the ones asked for: `first` is honoured)
    store.staging(1)[:3] = [[0, 1, 2]] * 3
    store.staging(1)[3:3 + len(regions)] = regions
    store.append(1, 3 + len(regions))
    got = cl.run_store(store, 1, 3, len(regions), *combo)
    store.close()
    return got


@pytest.fixture(scope="module")
def random_world():
    n_seq, roots, regions = cd.random_world()
    return n_seq, roots, regions, {combo: cd.brute(n_seq, roots, regions, *combo) for combo in cd.COMBOS}


@pytest.mark.parametrize("name", sorted(cd.HAND))
def test_the_end_table_is_a_stable_sort(name):
    n_seq, roots, _ = cd.HAND[name]
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, 8)
    e_end, e_pos = cl.end_table()
    w_end, w_pos = cd.end_table(n_seq, roots)
    assert np.array_equal(e_end, w_end) and np.array_equal(e_pos, w_pos)
    cl.close()
    ix.close()


@pytest.mark.parametrize("n_seq", [1, 255, 256, 257, 300, 70000])
def test_the_end_table_at_the_sort_plans(n_seq):
    # one, two and three seqid bytes in the sort plan; more than one sort tile of roots; many equal ends
    rng = np.random.default_rng(n_seq)
    n = 9000
    roots = np.empty((n, 3), np.uint32)
    roots[:, 0] = rng.integers(0, n_seq, n)
    roots[:3, 0] = [0, n_seq - 1, n_seq // 2]
    roots[:, 1] = rng.integers(0, 1 << 20, n)
    roots[:, 2] = roots[:, 1] + rng.choice([0, 5, 5, 1000, 1 << 24], n)
    roots[n // 2:, 2] = (roots[n // 2:, 2] >> 12) << 12
    roots[n // 2:, 1] = np.minimum(roots[n // 2:, 1], roots[n // 2:, 2])
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, 8)
    e_end, e_pos = cl.end_table()
    w_end, w_pos = cd.end_table(n_seq, roots)
    assert np.array_equal(e_end, w_end) and np.array_equal(e_pos, w_pos)
    assert cl.stats()["build_ms"] > 0
    cl.close()
    ix.close()


@pytest.mark.parametrize("name", sorted(cd.HAND))
def test_the_hand_cases(name):
    n_seq, roots, regions = cd.HAND[name]
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, len(regions))
    for combo in cd.COMBOS:
        want = cd.brute(n_seq, roots, regions, *combo)
        _same(cl.run(regions, *combo), want, (name, combo, "host"))
        _same(_via_store(cl, regions, combo), want, (name, combo, "store"))
        if (name, combo) in cd.BY_HAND or name == "table":
            counts, offsets, triples, gaps = cl.run(regions, *combo)
            dist = engine.closest_distances(regions, counts, triples, gaps)
            rows = [[(int(triples[k, 0]), int(dist[k])) for k in range(int(offsets[i]), int(offsets[i + 1]))] for i in range(len(counts))]
            if name == "table":
                assert [[(cd.TABLE_NAMES[f], d) for f, d in row] for row in rows] == cd.TABLE_BY_HAND[combo]
            else:
                assert rows == cd.BY_HAND[(name, combo)]
    cl.close()
    ix.close()


@pytest.mark.parametrize("combo", cd.COMBOS, ids=lambda c: "%s-%s" % ("ignore" if c[0] else "default", c[1]))
def test_the_random_set(random_world, combo):
    n_seq, roots, regions, want = random_world
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, len(regions))
    _same(cl.run(regions, *combo), want[combo], (combo, "host"))
    blocks, chunk = cl.last_grid()
    assert blocks == -(-len(regions) // 256) and chunk == 256
    _same(_via_store(cl, regions, combo), want[combo], (combo, "store"))
    assert cl.last_kernel_ms() > 0
    cl.close()
    ix.close()


@pytest.mark.parametrize("nq", [0, 1, 255, 256, 257, 769])
def test_region_counts_at_the_launch_edges(random_world, nq):
    n_seq, roots, regions, want = random_world
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, 1024)
    for combo in ((False, "both"), (True, "left")):
        w = cd.brute(n_seq, roots, regions[:nq], *combo)
        got = cl.run(regions[:nq], *combo)
        _same(got, w, (nq, combo))
        blocks, chunk = cl.last_grid()
        assert blocks == -(-nq // 256)
        if nq == 769:  # four blocks, and the earlier ones have pairs: the last block's base is a sum over three partial sums
            assert blocks >= 3 and chunk == 256
            assert int(got[1][256]) > 0 and int(got[1][512]) > int(got[1][256]) and int(got[1][768]) > int(got[1][512])
    with pytest.raises(E) as ei:
        cl.run(regions[:1025])
    assert ei.value.code == -1
    _same(cl.run(regions[:5]), cd.brute(n_seq, roots, regions[:5]), "after a refused argument")
    cl.close()
    ix.close()


def test_a_chunk_of_more_than_one_tile_per_block():
    # more than 2048 tiles of 256 regions: a block serves two tiles and carries its base from one to the next
    n_seq, roots, _ = cd.random_world()
    rng = np.random.default_rng(5)
    nq = 2048 * 256 + 300
    regions = np.empty((nq, 3), np.uint32)
    regions[:, 0] = rng.integers(0, n_seq, nq)
    regions[:, 1] = rng.integers(0, 9000, nq)
    regions[:, 2] = regions[:, 1] + rng.choice([1, 50, 700], nq)
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, nq)
    got = cl.run(regions)
    blocks, chunk = cl.last_grid()
    assert chunk == 512 and blocks == -(-nq // 512)
    pick = np.r_[0:600, nq - 900:nq]
    w = cd.brute(n_seq, roots, regions[pick])
    counts, offsets, triples, gaps = got
    assert np.array_equal(counts[pick], w[0]) and np.array_equal(gaps[pick][w[0] > 0], w[3][w[0] > 0])
    assert np.array_equal(offsets[1:], np.cumsum(counts.astype(np.uint64))) and offsets[0] == 0
    tail = triples[int(offsets[nq - 900]):]
    assert np.array_equal(tail, w[2][int(w[1][600]):])
    cl.close()
    ix.close()


def test_a_batch_without_answers_and_one_that_grows_the_pair_buffer():
    n_seq, roots, _ = cd.HAND["forty_roots_with_one_start"]
    ix = _index(n_seq + 1, roots)  # (seqid 2 has no roots)
    nq = 300
    cl = engine.Closest(ix, nq)    # room for nq pairs at first
    nothing = np.tile(np.array([[2, 10, 20]], np.uint32), (nq, 1))
    nothing[::3] = [0, 50, 50]      # ... and empty regions
    nothing[1::3] = [0, 30000, 30001]
    counts, offsets, triples, gaps = cl.run(nothing, False, "right")
    assert not counts.any() and not offsets.any() and triples.shape == (0, 3) and len(offsets) == nq + 1
    assert cl.stats()["grows"] == 0
    ties = np.tile(np.array([[0, 4000, 5000]], np.uint32), (nq, 1))
    ties[:, 1] += np.arange(nq, dtype=np.uint32)
    want = cd.brute(n_seq + 1, roots, ties)
    assert want[0].tolist() == [40] * nq
    _same(cl.run(ties), want, "ties")
    assert cl.stats()["grows"] == 1
    _same(cl.run(ties, True, "right"), cd.brute(n_seq + 1, roots, ties, True, "right"), "the grown buffer again")
    assert cl.stats()["grows"] == 1
    cl.close()
    ix.close()


def test_more_seqids_than_the_lds_staging_holds():
    n_seq = META_LDS_SEQIDS + 1
    rng = np.random.default_rng(11)
    on = np.array([0, 1, 700, n_seq - 2, n_seq - 1])
    roots = np.empty((200, 3), np.uint32)
    roots[:, 0] = rng.choice(on, 200)
    roots[:, 1] = rng.integers(0, 50, 200) * 100
    roots[:, 2] = roots[:, 1] + rng.choice([1, 30, 100, 900], 200)
    regions = np.empty((700, 3), np.uint32)
    regions[:, 0] = rng.choice(np.r_[on, 5, 1000], 700)
    regions[:, 1] = rng.integers(0, 6000, 700)
    regions[:, 2] = regions[:, 1] + rng.choice([1, 9, 250], 700)
    for n in (n_seq - 1, n_seq):  # the last count that is staged, the first that is not
        r = roots.copy()
        q = regions.copy()
        r[:, 0] = np.minimum(r[:, 0], n - 1)
        q[:, 0] = np.minimum(q[:, 0], n - 1)
        ix = _index(n, r)
        cl = engine.Closest(ix, len(q))
        for combo in cd.COMBOS:
            _same(cl.run(q, *combo), cd.brute(n, r, q, *combo), (n, combo))
        cl.close()
        ix.close()


def test_a_seqid_out_of_range_and_two_runs_with_different_flags(random_world):
    n_seq, roots, regions, want = random_world
    ix = _index(n_seq, roots)
    cl = engine.Closest(ix, len(regions))
    bad = regions[:600].copy()
    bad[577, 0] = n_seq
    with pytest.raises(E) as ei:
        cl.run(bad)
    assert ei.value.code == -5 and b"chr >=" in str(ei.value).encode()
    with pytest.raises(E) as ei:  # the run is void: nothing to read
        engine.check(engine.lib().gffx_hip_closest_wait(cl._h))
    assert ei.value.code == -6
    with pytest.raises(E) as ei:
        cl.run(regions, flags=6)
    assert ei.value.code == -1
    # ... and the handle goes on: two runs with different flags, then the first again
    a, b = (False, "both"), (True, "right")
    _same(cl.run(regions, *a), want[a], a)
    _same(cl.run(regions, *b), want[b], b)
    _same(cl.run(regions, *a), want[a], a)
    cl.close()
    ix.close()


@pytest.mark.skipif(engine.device_count() < 2, reason="needs a second device")
def test_a_handle_on_a_cloned_index(random_world):
    n_seq, roots, regions, want = random_world
    ix = _index(n_seq, roots)
    ix1 = ix.clone(1)
    cl = engine.Closest(ix1, len(regions))
    combo = (True, "both")
    _same(cl.run(regions, *combo), want[combo], "clone")
    _same(_via_store(cl, regions, combo, device=1), want[combo], "clone, store")
    store0 = engine.RegionStore(0, 16, False, 0)
    store0.append(0, 4)
    with pytest.raises(E) as ei:
        cl.run_store(store0, 0, 0, 4)
    assert ei.value.code == -1
    store0.close()
    cl.close()
    ix1.close()
    ix.close()
