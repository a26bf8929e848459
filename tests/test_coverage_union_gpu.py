"""The device-side union builder (gffx_hip_union_*): its spans == a numpy restatement of merge_intervals
(commands/coverage.rs:92-109: sort by start, merge while s <= current end), however the rows are grouped into adds or
exchanged between handles; its covered bases == the definition and == the one-shot gffx_hip_segments_covered."""
import numpy as np
import pytest

from gffx_amd import engine

pytestmark = pytest.mark.gpu


def _merge_definition(rows, n_seq):
    """(u_off, us, ue, pb) of the rows: per seqid sort by start, merge while s <= current end; pb = covered bases of the
    seqid's spans before this one."""
    u_off, us, ue, pb = [0], [], [], []
    for c in range(n_seq):
        r = rows[rows[:, 0] == c]
        r = r[np.argsort(r[:, 1], kind="stable")]
        acc, cur = 0, None
        for s, e in zip(r[:, 1].tolist(), r[:, 2].tolist()):
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
    return (np.array(u_off, np.uint64), np.array(us, np.uint32), np.array(ue, np.uint32), np.array(pb, np.uint64))


def _numpy_covered(seg_seq, seg_start, seg_end, regions, n_seq):
    out = np.zeros(len(seg_seq), np.uint32)
    for c in range(n_seq):
        r = regions[regions[:, 0] == c]
        if not len(r):
            continue
        hi = int(r[:, 2].max())
        mask = np.zeros(hi + 1, np.int32)  # difference array over the seqid's bases
        np.add.at(mask, r[:, 1], 1)
        np.add.at(mask, r[:, 2], -1)
        covered = np.concatenate([[0], np.cumsum(np.cumsum(mask)[:hi] > 0)])  # covered[x] = covered bases in [0, x)
        for i in np.nonzero(seg_seq == c)[0]:
            a, b = min(int(seg_start[i]), hi), min(int(seg_end[i]), hi)
            out[i] = covered[b] - covered[a] if b > a else 0
    return out


def _build(rows, n_seq, chunks=None):
    u = engine.RegionUnion(n_seq)
    for piece in (chunks if chunks is not None else [rows]):
        u.add(piece)
    u.finish()
    return u


def _assert_spans(got, want):
    for g, w, name in zip(got, want, ("u_off", "us", "ue", "pb")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


def _random_rows(seed, nq, n_seq=5, span=2_000_000):
    rng = np.random.default_rng(seed)
    rows = np.empty((nq, 3), np.uint32)
    rows[:, 0] = rng.integers(0, n_seq - 1, nq)  # the last seqid has no rows at all
    rows[:, 1] = rng.integers(0, span, nq)
    rows[:, 2] = rows[:, 1] + rng.choice([1, 30, 500, 40000], nq) + rng.integers(0, 50, nq)
    if nq > 3:  # touching, nested and duplicate rows
        rows[1] = (rows[0, 0], rows[0, 2], rows[0, 2] + 10)
        rows[2] = (rows[0, 0], rows[0, 1] + 0, max(int(rows[0, 1]) + 1, int(rows[0, 2]) - 1))
        rows[3] = rows[0]
    return rows


@pytest.mark.parametrize("seed,nq", [(0, 1), (1, 400), (2, 20000), (3, 300000)])
def test_spans_equal_the_definition(seed, nq):
    rows = _random_rows(seed, nq)
    u = _build(rows, 5)
    want = _merge_definition(rows, 5)
    assert u.n_spans == len(want[1])
    _assert_spans(u.spans(), want)
    assert u.stats()["rows"] == nq and u.stats()["folds"] >= 1


def _case(name):
    rng = np.random.default_rng(11)
    if name == "touching_and_nested":
        return 3, np.array([[0, 10, 20], [0, 20, 30], [0, 31, 40], [0, 5, 100], [0, 50, 60], [1, 7, 9], [1, 9, 11],
                            [1, 0, 7], [2, 4000000000, 4294967295], [2, 1, 4000000000]], np.uint32)
    if name == "duplicates":
        return 2, np.repeat(np.array([[0, 100, 200], [1, 5, 6], [0, 150, 300]], np.uint32), 700, axis=0)
    if name == "a_seqid_without_rows":
        return 4, np.array([[0, 1, 2], [3, 1, 2], [3, 5, 9], [0, 2, 3]], np.uint32)
    if name == "one_row":
        return 3, np.array([[1, 17, 18]], np.uint32)
    if name == "one_seqid":
        r = _random_rows(5, 50000, n_seq=2)
        return 2, r
    if name == "300_seqids":  # more seqids than one radix digit holds
        n = 40000
        r = np.empty((n, 3), np.uint32)
        r[:, 0] = rng.integers(0, 300, n)
        r[:, 1] = rng.integers(0, 100000, n)
        r[:, 2] = r[:, 1] + rng.integers(1, 40, n)
        return 300, r
    r = _random_rows(6, 30000)
    order = np.lexsort((r[:, 1], r[:, 0]))
    return 5, (r[order] if name == "sorted" else r[order[::-1]])


@pytest.mark.parametrize("name", ["touching_and_nested", "duplicates", "a_seqid_without_rows", "one_row", "one_seqid", "300_seqids",
                                  "sorted", "reverse_sorted"])
def test_spans_of_special_shapes(name):
    n_seq, rows = _case(name)
    rows = np.ascontiguousarray(rows)
    _assert_spans(_build(rows, n_seq).spans(), _merge_definition(rows, n_seq))


def test_an_empty_union_is_queryable():
    u = engine.RegionUnion(3)
    u.add(np.zeros((0, 3), np.uint32))
    u.finish()
    o, us, ue, pb = u.spans()
    assert o.tolist() == [0, 0, 0, 0] and len(us) == len(ue) == len(pb) == 0
    assert u.segments_covered([0, 2], [5, 5], [9, 9]).tolist() == [0, 0]


@pytest.mark.parametrize("seed,nq", [(7, 5000), (8, 120000)])
def test_grouping_does_not_matter(seed, nq):
    rows = _random_rows(seed, nq)
    want = _merge_definition(rows, 5)
    one = _build(rows, 5).spans()
    _assert_spans(one, want)
    cuts = np.sort(np.random.default_rng(seed).integers(0, nq, 6))
    cuts[0] = 0  # (an empty first chunk)
    seven = _build(rows, 5, np.split(rows, cuts)).spans()
    _assert_spans(seven, one)
    # two handles, each with a share of the rows, merged through add_spans -- in both directions
    a, b = _build(rows[: nq // 3], 5), _build(rows[nq // 3:], 5)
    bo, bs, be, _ = b.spans()
    ao, as_, ae, _ = a.spans()
    a.add_spans(bo, bs, be)
    a.finish()
    _assert_spans(a.spans(), one)
    b.add_spans(ao, as_, ae)
    b.finish()
    _assert_spans(b.spans(), one)


def test_one_row_at_a_time():
    rows = _random_rows(9, 60, n_seq=3, span=3000)
    u = engine.RegionUnion(3)
    for r in rows:
        u.add(r[None, :])
    u.finish()
    _assert_spans(u.spans(), _merge_definition(rows, 3))
    _assert_spans(u.spans(), _build(rows, 3).spans())


@pytest.mark.parametrize("seed,nq,nseg", [(0, 1, 50), (1, 400, 3000), (2, 20000, 50000), (3, 300000, 200000)])
def test_covered_bases_equal_the_definition_and_the_one_shot_entry(seed, nq, nseg):
    rng = np.random.default_rng(seed)
    n_seq, span = 5, 2_000_000
    regions = _random_rows(seed, nq)
    seg_seq = rng.integers(0, n_seq, nseg).astype(np.uint32)
    seg_start = rng.integers(0, span + 50000, nseg).astype(np.uint32)
    seg_end = (seg_start + rng.choice([1, 100, 5000, 300000], nseg)).astype(np.uint32)
    seg_seq[0], seg_start[0], seg_end[0] = regions[0]  # a segment equal to a row
    seg_end[1] = seg_start[1]  # an empty segment
    seg_seq[2], seg_start[2], seg_end[2] = 0, span + 100000, span + 100050  # beyond the last span
    u = _build(regions, n_seq, np.array_split(regions, 3))
    got = u.segments_covered(seg_seq, seg_start, seg_end)
    assert np.array_equal(got, _numpy_covered(seg_seq, seg_start, seg_end, regions, n_seq))
    assert np.array_equal(got, engine.segments_covered(seg_seq, seg_start, seg_end, regions, n_seq))
    assert got[1] == 0 and got[2] == 0


def test_errors_are_reported_and_a_valid_build_follows():
    E = engine._ffi.GffxHipError
    ok = np.array([[0, 1, 5], [2, 3, 9]], np.uint32)
    u = engine.RegionUnion(3)
    with pytest.raises(E) as ei:
        u.add(np.array([[0, 1, 5], [3, 1, 2]], np.uint32))  # seqid 3 of 3
    assert ei.value.code == -5
    with pytest.raises(E):  # the object only reports the error again
        u.finish()
    u.close()
    u = engine.RegionUnion(3)
    u.add(ok)
    with pytest.raises(E) as ei:
        u.add(np.array([[1, 7, 7]], np.uint32))  # start >= end
        u.finish()
    assert ei.value.code == -1
    u.close()
    u = engine.RegionUnion(3)
    with pytest.raises(E) as ei:  # not finished yet
        u.spans()
    assert ei.value.code == -6
    u.close()
    for call in (lambda: u.add(ok), u.finish, u.spans, lambda: u.segments_covered([0], [1], [2])):
        with pytest.raises(E) as ei:  # use after destroy: the handle is gone, the call is refused
            call()
        assert ei.value.code == -1
    assert u.n_spans == 0
    u = _build(ok, 3)
    assert u.spans()[1].tolist() == [1, 3] and u.segments_covered([2, 1], [0, 0], [100, 100]).tolist() == [6, 0]
    with pytest.raises(E) as ei:
        u.segments_covered([3], [0], [1])
    assert ei.value.code == -5
