"""The permutation totals on the device through the C-ABI (engine.ClassMap.perm_*): both matrices and the unplaced count are
compared bit for bit with the definition in Python integers (tests/_enrich_definition.py) -- the hand-written example, region
counts around the wave and the block, permutation counts around the group of rows a block walks, 1 to 32 layers, every region
in one class and regions over all 33, the length and width edges, any split into runs with its first_row, both ways to hand
regions in -- and the refusals."""
import numpy as np
import pytest

import _annotate_definition as ad
import _enrich_definition as ed
from gffx_amd import engine
from gffx_amd._ffi import GffxHipError

pytestmark = pytest.mark.gpu


def build(n_seq, T, rows):
    m = engine.ClassMap(n_seq, T)
    m.add_rows(np.asarray(rows, np.uint32).reshape(-1, 4))
    m.finish()
    return m


def device(m, seq_len, regions, n_perm, seed, first_row=0):
    m.perm_begin(seq_len, n_perm, seed)
    m.perm_run(regions, first_row)
    return m.perm_totals()


def check(case, n_perm, seed, fast=True):
    n_seq, T, rows, seq_len, regions = case
    m = build(n_seq, T, rows)
    got = device(m, seq_len, regions, n_perm, seed)
    m.close()
    want = ed.totals(n_seq, T, rows, seq_len, regions, n_perm, seed, fast=fast)
    assert got[0].dtype == np.uint64 and got[0].shape == (n_perm + 1, T + 1) and ed.same(got, want)
    return want


@pytest.fixture(scope="module")
def shared():
    """One map of ~2000 points over three seqids, 3000 regions, and the definition's totals of 40 permutations of them."""
    n_seq, T, rows, seq_len, regions = ed.random_case(101, T=5, n=1500, size=200000, nq=3000, width=60)
    want = ed.totals(n_seq, T, rows, seq_len, regions, 40, 77, fast=True)
    m = build(n_seq, T, rows)
    yield dict(case=(n_seq, T, rows, seq_len, regions), want=want, map=m)
    m.close()


def test_the_hand_example():
    m = build(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS)
    for seed in (0, 12345):
        assert ed.same(device(m, ed.HAND_LEN, ed.HAND_REGIONS, ed.HAND_N_PERM, seed), ed.hand())
    m.close()
    check((ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, [700, 20], ed.HAND_REGIONS), 9, 3, fast=False)


def test_the_largest_case(shared):
    n_seq, T, rows, seq_len, regions = shared["case"]
    got = device(shared["map"], seq_len, regions, 40, 77)
    assert ed.same(got, shared["want"])
    B, R, unplaced = got
    assert unplaced > 0 and np.all(R.sum(1) == len(regions)) and len({int(v) for v in B.sum(1)}) == 1
    assert len({tuple(r) for r in B[1:].tolist()}) == 40  # forty different permutations
    assert shared["map"].perm_last_kernel_ms() > 0


def test_region_counts_around_the_wave_and_the_block(shared):
    _, block = engine._enrich_constants()
    n_seq, T, rows, seq_len, regions = shared["case"]
    m = shared["map"]
    for nq in sorted({0, 1, 63, 64, 65, 255, 256, 257, 2 * block + 1}):
        want = ed.totals(n_seq, T, rows, seq_len, regions[:nq], 3, 5, fast=True)
        assert ed.same(device(m, seq_len, regions[:nq], 3, 5), want), nq


def test_permutation_counts_around_the_group(shared):
    G, _ = engine._enrich_constants()
    n_seq, T, rows, seq_len, regions = shared["case"]
    m = shared["map"]
    want = ed.totals(n_seq, T, rows, seq_len, regions[:300], 2 * G + 1, 9, fast=True)
    for n_perm in sorted({0, 1, G - 1, G, G + 1, 2 * G + 1}):
        got = device(m, seq_len, regions[:300], n_perm, 9)
        # (row p depends on p, the seed and the region's row only: fewer permutations are the first rows of more)
        assert ed.same(got, (want[0][:n_perm + 1], want[1][:n_perm + 1], want[2])), n_perm


@pytest.mark.parametrize("T", [1, 5, 32])
def test_layer_counts(T):
    check(ed.random_case(40 + T, T=T, n=300, nq=400), 5, T)


def test_every_region_in_one_class_and_regions_over_all_33():
    # one class: layer 0 covers every seqid wholly, so every base of every placed region is of class 0
    n_seq, T, rows, seq_len, regions = ed.random_case(50, T=32, n=100, nq=600)
    cover = np.array([[0, c, 0, int(seq_len[c])] for c in range(n_seq)], np.uint32)
    regions = regions[regions[:, 2] <= seq_len[regions[:, 0]]]
    B, R, _ = check((n_seq, T, np.concatenate([rows, cover]), seq_len, regions), 4, 6)
    assert not B[:, 1:].any() and not R[:, 1:T].any() and (B[:, 0] > 0).all()
    # all 33: stripes of 10 bases, layer k on [100 k, 100 k + 10) of every period of 3300, one-base regions
    rows = np.array([[k, 0, 3300 * j + 100 * k, 3300 * j + 100 * k + 10] for j in range(30) for k in range(32)], np.uint32)
    regions = np.array([[0, x, x + 1] for x in range(0, 99000, 7)][:1024], np.uint32)
    B, R, _ = check((1, 32, rows, [99000], regions), 6, 8)
    assert (R[0] > 0).all() and (B[0] > 0).all()


def test_the_length_and_width_edges():
    want = check(ed.edge_case(), 17, 2)
    assert want[2] == 4
    B, _, _ = check(ed.big_totals_case(), 3, 4)
    assert int(B[0, 0]) == 8 << 31


def test_any_split_into_runs_with_its_first_row(shared):
    n_seq, T, rows, seq_len, regions = shared["case"]
    m = shared["map"]
    m.perm_begin(seq_len, 40, 77)
    for first, last in ((0, 1), (1, 8), (8, len(regions))):
        m.perm_run(regions[first:last], first)
    assert ed.same(m.perm_totals(), shared["want"])
    # first_row counts: the same runs numbered from 0 each give other permutations, and the same observed row
    few = regions[:200]
    parts = [few[:1], few[1:8], few[8:]]
    m.perm_begin(seq_len, 5, 77)
    for part in parts:
        m.perm_run(part, 0)
    got = m.perm_totals()
    right = ed.totals(n_seq, T, rows, seq_len, few, 5, 77, fast=True)
    wrong = ed.totals(n_seq, T, rows, seq_len, parts[0], 5, 77, fast=True)
    for part in parts[1:]:
        wrong = ed.add(wrong, ed.totals(n_seq, T, rows, seq_len, part, 5, 77, fast=True))
    assert ed.same(got, wrong) and not ed.same(got, right) and np.array_equal(got[0][0], right[0][0]) and np.array_equal(got[1][0], right[1][0])


def test_a_run_cut_into_several_launches(shared, monkeypatch):
    """GFFX_HIP_PERM_LAUNCH_BLOCKS (read by perm_begin) caps the blocks of one launch of k_classmap_permute: a run then takes
    several launches, each from a later tile on, and the totals are the same bits."""
    G, block = engine._enrich_constants()
    n_seq, T, rows, seq_len, regions = shared["case"]
    m = shared["map"]
    tiles = -(-len(regions) // block)
    assert tiles >= 12 and -(-41 // G) > 3
    monkeypatch.setenv("GFFX_HIP_PERM_LAUNCH_BLOCKS", "3")  # fewer than the row groups of 40 permutations: one tile per launch
    assert ed.same(device(m, seq_len, regions, 40, 77), shared["want"])
    monkeypatch.setenv("GFFX_HIP_PERM_LAUNCH_BLOCKS", str(5 * -(-41 // G) + 1))  # five tiles per launch, the last launch shorter
    assert ed.same(device(m, seq_len, regions, 40, 77), shared["want"])
    m.perm_begin(seq_len, 40, 77)  # ... and with runs that do not begin at row 0
    monkeypatch.delenv("GFFX_HIP_PERM_LAUNCH_BLOCKS")  # (the cap of a begin holds for its runs)
    m.perm_run(regions[:700], 0)
    m.perm_run(regions[700:], 700)
    assert ed.same(m.perm_totals(), shared["want"])
    want = ed.totals(n_seq, T, rows, seq_len, regions[:2 * block + 1], 0, 5, fast=True)
    monkeypatch.setenv("GFFX_HIP_PERM_LAUNCH_BLOCKS", "2")  # one row group: two tiles per launch, three tiles
    assert ed.same(device(m, seq_len, regions[:2 * block + 1], 0, 5), want)
    monkeypatch.setenv("GFFX_HIP_PERM_LAUNCH_BLOCKS", "0")  # out of range: the default
    assert ed.same(device(m, seq_len, regions[:2 * block + 1], 0, 5), want)


def test_host_rows_against_the_store(shared):
    n_seq, T, rows, seq_len, regions = shared["case"]
    m = shared["map"]
    store = engine.RegionStore(0, len(regions) + 8, False)
    store.staging(1)[:len(regions)] = regions
    store.append(1, len(regions))
    m.perm_begin(seq_len, 40, 77)
    m.perm_run_store(store, 1, 0, len(regions), 0)
    assert ed.same(m.perm_totals(), shared["want"])
    m.perm_begin(seq_len, 40, 77)
    m.perm_run_store(store, 1, 0, 5, 0)  # a slice, then the rest from an odd row on
    m.perm_run_store(store, 1, 5, len(regions) - 5, 5)
    assert ed.same(m.perm_totals(), shared["want"])
    with pytest.raises(GffxHipError) as e:
        m.perm_run_store(store, 1, 0, len(regions) + 1, 0)
    assert e.value.code == ad.E_INVALID
    assert ed.same(m.perm_totals(), shared["want"])  # a refused argument adds nothing
    store.close()


def test_perm_begin_twice_resets_the_totals(shared):
    n_seq, T, rows, seq_len, regions = shared["case"]
    m = shared["map"]
    first = device(m, seq_len, regions[:500], 4, 1)
    m.perm_run(regions[:500], 0)  # the totals add up over runs ...
    twice = m.perm_totals()
    assert np.array_equal(twice[0], 2 * first[0]) and np.array_equal(twice[1], 2 * first[1]) and twice[2] == 2 * first[2]
    assert ed.same(device(m, seq_len, regions[:500], 4, 1), first)  # ... and begin starts over
    m.perm_begin(seq_len, 2, 1)
    B, R, unplaced = m.perm_totals()  # nothing run: zeros of the new shape
    assert B.shape == (3, T + 1) and not B.any() and not R.any() and unplaced == 0


def test_annotate_on_the_same_handle_keeps_its_counts():
    m = build(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS)
    counts, best = m.run(ad.HAND_REGIONS)
    assert ed.same(device(m, ed.HAND_LEN, ed.HAND_REGIONS, 2, 0), ed.hand())
    again = np.zeros_like(counts)
    from gffx_amd._ffi import check as ffi_check, lib, u32p
    ffi_check(lib().gffx_hip_classmap_copy_counts(m._h, again.ctypes.data_as(u32p)))  # the counts of the run before perm_run, still there
    assert np.array_equal(again, counts) and np.array_equal(counts, np.array(ad.HAND_COUNTS, np.uint32)) and best.tolist() == ad.HAND_CLASS
    assert m.run(ad.HAND_REGIONS)[1].tolist() == ad.HAND_CLASS
    assert ed.same(m.perm_totals(), ed.hand())  # ... and a run of annotate leaves the totals alone
    m.close()


def test_the_refusals():
    m = engine.ClassMap(ad.HAND_N_SEQ, ad.HAND_T)
    m.add_rows(ad.HAND_ROWS)
    with pytest.raises(GffxHipError) as e:
        m.perm_begin(ed.HAND_LEN, 2, 0)  # before finish
    assert e.value.code == ad.E_STATE
    m.finish()
    with pytest.raises(GffxHipError) as e:
        m.perm_run(ed.HAND_REGIONS, 0)  # before perm_begin
    assert e.value.code == ad.E_STATE
    with pytest.raises(GffxHipError) as e:
        m.perm_totals()
    assert e.value.code == ad.E_STATE
    with pytest.raises(GffxHipError) as e:
        m.perm_begin(ed.HAND_LEN, ed.MAX_PERMS + 1, 0)
    assert e.value.code == ad.E_INVALID
    with pytest.raises(GffxHipError) as e:
        m.perm_run(ed.HAND_REGIONS, 0)  # a refused begin opens nothing
    assert e.value.code == ad.E_STATE
    # ... and leaves totals that are open as they are, shape included
    assert ed.same(device(m, ed.HAND_LEN, ed.HAND_REGIONS, 2, 0), ed.hand())
    with pytest.raises(GffxHipError) as e:
        m.perm_begin(ed.HAND_LEN, ed.MAX_PERMS + 1, 0)
    assert e.value.code == ad.E_INVALID
    assert ed.same(m.perm_totals(), ed.hand())
    # a row on a seqid out of range voids its run -- and only its run -- and the handle stays usable
    m.perm_begin(ed.HAND_LEN, 2, 0)
    m.perm_run(ed.HAND_REGIONS[:3], 0)
    bad = ed.HAND_REGIONS.copy()
    bad[4, 0] = 2
    m.perm_run(bad, 0)
    m.perm_run(ed.HAND_REGIONS[3:], 3)
    with pytest.raises(GffxHipError) as e:
        m.perm_totals()
    assert e.value.code == ad.E_CHR_RANGE
    assert ed.same(m.perm_totals(), ed.hand())  # reported once; the two good runs stand
    assert ed.same(device(m, ed.HAND_LEN, ed.HAND_REGIONS, 2, 0), ed.hand())
    # new rows make the map stale: the totals go with it
    m.add_rows([[0, 1, 100, 200]])
    with pytest.raises(GffxHipError) as e:
        m.perm_run(ed.HAND_REGIONS, 0)
    assert e.value.code == ad.E_STATE
    m.finish()
    with pytest.raises(GffxHipError) as e:
        m.perm_run(ed.HAND_REGIONS, 0)
    assert e.value.code == ad.E_STATE
    m.close()
