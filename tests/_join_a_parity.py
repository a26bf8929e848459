"""The Join A parity check shared by the GPU suites (tests/test_join_a_gpu.py, tests/test_knob_edges_gpu.py): one batch, every output
of the engine -- counts, triples, root_fids, offsets, segment bases, per-query segments, unique roots, emission records -- compared
with the oracle's."""
import numpy as np

from gffx_amd import engine
from oracle import binding as ob

FLAGS = engine.OUT_FIDS | engine.OUT_TRIPLES | engine.OUT_ROOT_BITMAP | engine.OUT_OFFSETS


def _sorted_rows(t):
    t = np.asarray(t, dtype=np.uint32).reshape(-1, 3)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def _check(roots, regions, mode, invert, soa=False, strategy=engine.STRATEGY_AUTO, knobs=None, reserve=0, ix=None, oix=None):
    """One batch over `regions`, every output of the engine against the oracle.  knobs: {name: value} set on the batch before its
    first run (the partitioned strategy sizes its chunks on its first pass); reserve: reserve_hits before it (a small one forces the
    capacity replay at the wait); ix / oix: an index and its oracle built once by the caller (else from `roots`)."""
    co, s, e, f = roots["chr_offsets"], roots["start"], roots["end"], roots["fid"]
    own_ix = ix is None
    if oix is None:
        oix = ob.OracleIndex.from_roots(co, s, e, f)
    want_t, want_c = oix.query_features(regions, int(mode), invert)
    if own_ix:
        ix = engine.TreeIndexData.from_roots(co, s, e, f)
    b = engine.QueryBatch(ix, max(len(regions), 1))
    for name, value in (knobs or {}).items():
        b.set_option(name, value)
    if reserve:
        b.reserve_hits(reserve)
    if soa:
        b.set_regions_soa(regions[:, 0], regions[:, 1], regions[:, 2])
    else:
        b.set_regions(regions)
    b.run(mode, invert, FLAGS, strategy)
    b.wait()
    assert b.total_hits == len(want_t)
    got_c = b.counts()
    assert np.array_equal(got_c, want_c)
    got_t = b.triples()
    assert np.array_equal(_sorted_rows(got_t), _sorted_rows(want_t))
    assert np.array_equal(b.fids(), got_t[:, 0])
    off = b.offsets()
    assert int(off[-1]) == len(want_t)
    if strategy == engine.STRATEGY_DIRECT:  # direct: CSR in input order
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(want_c.astype(np.uint64))]).astype(np.uint64))
    else:  # partitioned (or AUTO): every query's segment is given explicitly; the segments tile [0, pairs)
        nz = want_c > 0
        seg_lo, seg_hi = off[:-1][nz], off[:-1][nz] + want_c[nz]
        order = np.argsort(seg_lo)
        assert len(seg_lo) == 0 or (seg_lo[order][0] == 0 and seg_hi[order][-1] == len(want_t)
                                    and np.array_equal(seg_hi[order][:-1], seg_lo[order][1:]))
    # pairs of query i are exactly the oracle's pairs of query i (their order inside a query is free)
    for qi in np.random.default_rng(0).choice(len(regions), size=min(200, len(regions)), replace=False):
        seg = got_t[int(off[qi]):int(off[qi]) + int(got_c[qi])]
        one_t, _ = oix.query_features(regions[qi:qi + 1], int(mode), invert)
        assert np.array_equal(_sorted_rows(seg), _sorted_rows(one_t))
    assert np.array_equal(b.unique_roots(), np.unique(want_t[:, 0]))
    # a root_fid-only pass (what bench.py and `depth` run: its own emit path in the one-kernel strategies):
    # the (query, root_fid) pairs of EVERY query
    b.run(mode, invert, engine.OUT_FIDS | engine.OUT_OFFSETS, strategy)
    b.wait()
    c2, off2, f2 = b.counts(), b.offsets(), b.fids()
    assert np.array_equal(c2, want_c) and len(f2) == len(want_t)
    wc = want_c.astype(np.int64)
    qid = np.repeat(np.arange(len(regions), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    got_pairs = np.stack([qid, f2[off2[:-1].astype(np.int64)[qid] + within].astype(np.int64)], axis=1)
    by_chr = np.argsort(regions[:, 0], kind="stable")  # the oracle walks seqid after seqid, regions in input order
    want_pairs = np.stack([np.repeat(by_chr, wc[by_chr]), want_t[:, 0].astype(np.int64)], axis=1)
    order = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(order(got_pairs), order(want_pairs))
    if strategy in (engine.STRATEGY_AUTO, engine.STRATEGY_WINDOWS):
        # the pass bench.py times: counts + root_fids + ONE segment base per group of 256 regions (no per-region offsets);
        # a consumer derives a region's segment from the group's base and the counts before it
        b.run(mode, invert, engine.OUT_FIDS | engine.OUT_SEGBASE, strategy)
        b.wait()
        c3, f3, sb = b.counts(), b.fids(), b.segbase()
        assert np.array_equal(c3, want_c) and len(f3) == len(want_t) and len(sb) == (len(regions) + 255) // 256
        off3 = b.offsets_from_segbase(c3).astype(np.int64)
        got3 = np.stack([qid, f3[off3[qid] + within].astype(np.int64)], axis=1)
        assert np.array_equal(order(got3), order(want_pairs))
        gtot = np.add.reduceat(wc, np.arange(0, len(wc), 256)) if len(wc) else np.zeros(0, np.int64)
        nzg = gtot > 0  # the groups' runs tile [0, pairs)
        lo, hi = sb.astype(np.int64)[nzg], sb.astype(np.int64)[nzg] + gtot[nzg]
        o3 = np.argsort(lo)
        assert len(lo) == 0 or (lo[o3][0] == 0 and hi[o3][-1] == len(want_t) and np.array_equal(hi[o3][:-1], lo[o3][1:]))
    b.run(mode, invert, FLAGS, strategy)  # (back to the full pass for the records below; segment order is per pass)
    b.wait()
    off = b.offsets()
    # the same results as {input row, count, offset} records in emission order
    rows, rc, ro = b.query_records()
    assert np.array_equal(np.sort(rows), np.arange(len(regions), dtype=np.uint32))
    assert np.array_equal(rc, want_c[rows]) and np.array_equal(ro, off[:-1][rows])
    b.close()
    if own_ix:
        ix.close()
    return len(want_t)
