"""The two levels of the window index's coverage filter on the device: every windows-strategy launch stages the finest level that
fits its LDS beside the split bitmap, the seqid records and its strips (engine_windows.hip: run_windows_pass), and whichever level
it takes, the results are the oracle's -- counts, per-region root_fids, segment bases / per-region offsets, and the unique roots of
a root pass; every mode, inverted or not, at 512 and 1024 threads.

Three indexes over the same 1200 roots on three long seqids (1.45 Gbp: both levels are budget-limited, so they differ):
  fine    GFFX_HIP_WIN_FILTER_KB=2, _FINE_KB=8: cells of 2^17 and 2^15 bp; the 5.5 KB fine bitmap fits every launch; the batch takes
          the fine level wherever it fits (GFFX_HIP_WIN_FILTER=2) -> level 2
  coarse  the same index, the batch held to the coarse level (GFFX_HIP_WIN_FILTER=1) -> level 1
  tight   the defaults (24 KB; the fine level at most 48 KB), GFFX_HIP_WIN_FILTER=2: cells of 2^13 and 2^12 bp; the 44 KB fine bitmap fits a 1024-thread
          pair pass without per-region offsets and every root pass, but NOT a 512-thread pair pass (80 KB, 41 KB of them strips)
          nor a 1024-thread one with offsets parked beside the strips: those fall back to the coarse level (they do not shed a
          table for it)
The regions: rows around the roots, rows whose first and last base lie in one coarse cell but in two fine ones, rows across a
coarse boundary (the cells nest: no row lies in one fine cell and two coarse ones), rows inside one fine cell, rows of exactly
16384 bases (the widest the lines answer) and one base more, rows past the last root, empty and reversed rows -- and a row with a
seqid out of range, which is an error at every level.
"""
import os

import numpy as np
import pytest

from gffx_amd import engine, synth
from gffx_amd.engine import OverlapMode
from oracle import binding as ob

pytestmark = pytest.mark.gpu

CHROMS = [("a", 700_000_000), ("b", 500_000_000), ("c", 250_000_000)]
SIZES = [1, 63, 257, 5000]
WMAX = 16384
CONFIGS = {"fine": ({"GFFX_HIP_WIN_FILTER_KB": "2", "GFFX_HIP_WIN_FILTER_FINE_KB": "8"}, 2),
           "coarse": ({"GFFX_HIP_WIN_FILTER_KB": "2", "GFFX_HIP_WIN_FILTER_FINE_KB": "8"}, 1),
           "tight": ({}, 2)}


def _special_rows(roots):
    rows = []
    co, st, en = roots["chr_offsets"], roots["start"].astype(np.int64), roots["end"].astype(np.int64)
    for c in range(len(CHROMS)):
        lo, hi = int(co[c]), int(co[c + 1])
        for j in (lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3):
            s, e = int(st[j]), int(en[j])
            for csh, fsh in ((13, 12), (17, 15)):
                fb = ((s >> fsh) + 1) << fsh  # a fine boundary that is no coarse one: one coarse cell, two fine ones
                if fb % (1 << csh) == 0:
                    fb += 1 << fsh
                cb = ((s >> csh) + 1) << csh  # a coarse boundary: two cells at both levels
                rows += [(c, fb - 50, fb + 50), (c, cb - 50, cb + 50), (c, fb + 10, fb + 20), (c, fb - 1, fb), (c, fb, fb + 1)]
            rows += [(c, max(0, s + 1 - WMAX), max(0, s + 1 - WMAX) + WMAX), (c, e - 1, e - 1 + WMAX), (c, max(0, s - 100), max(0, s - 100) + WMAX + 1),
                     (c, s, e), (c, s, s), (c, s + 10, s), (c, e, e + 1), (c, max(0, s - 1), s)]
        last = int(en[lo:hi].max())
        rows += [(c, last, last + 100), (c, last + 1000, last + 5000), (c, 4_000_000_000, 4_000_000_100), (c, 0, 1)]
    return np.array(rows, dtype=np.uint32)


def _regions(roots, n):
    sp = _special_rows(roots)
    rng = np.random.default_rng(11)
    st = roots["start"].astype(np.int64)
    co = roots["chr_offsets"]
    j = rng.integers(0, len(st), 5000)
    c = np.searchsorted(co, j, side="right") - 1
    s = np.maximum(0, st[j] + rng.integers(-20_000, 20_000, 5000))
    w = rng.integers(1, 12_000, 5000)
    near = np.stack([c, s, s + w], axis=1).astype(np.uint32)
    far = synth.synth_bed(1000, seed=12, chroms=CHROMS, edge_frac=0.1, roots=roots)
    near[::5][: len(far)] = far  # every fifth row anywhere on the seqids (most of them far from every root)
    rows = np.concatenate([sp[:1], near[:40], sp[1:], near[40:]])  # (63 rows hold a few of the special ones, 257 all of them)
    assert len(sp) < 200
    return np.ascontiguousarray(rows[:n])


class _World:
    def __init__(self):
        self.roots = synth.gencode_like_roots(1200, seed=5, chroms=CHROMS)
        r = self.roots
        self.oix = ob.OracleIndex.from_roots(r["chr_offsets"], r["start"], r["end"], r["fid"])
        self.regions = {n: _regions(r, n) for n in SIZES}
        self.ix, self.want = {}, {}
        for name in ("fine", "tight"):
            env = CONFIGS[name][0]
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)  # (the index builders' knobs are read when the index is created)
            try:
                self.ix[name] = engine.TreeIndexData.from_roots(r["chr_offsets"], r["start"], r["end"], r["fid"])
            finally:
                for k, v in saved.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        self.ix["coarse"] = self.ix["fine"]

    def oracle(self, n, mode, invert):
        """the oracle's answer, computed once per (regions, mode, invert) and shared by the three configurations"""
        key = (n, int(mode), invert)
        if key not in self.want:
            regions = self.regions[n]
            t, c = self.oix.query_features(regions, int(mode), invert)
            wc = c.astype(np.int64)
            by_chr = np.argsort(regions[:, 0], kind="stable")  # the oracle walks seqid after seqid, regions in input order
            pairs = np.stack([np.repeat(by_chr, wc[by_chr]), t[:, 0].astype(np.int64)], axis=1)
            self.want[key] = (c, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))], np.unique(t[:, 0]))
        return self.want[key]


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.ix["fine"].close()
    w.ix["tight"].close()


def _pairs_of(b, counts, off):
    wc = counts.astype(np.int64)
    qid = np.repeat(np.arange(len(wc), dtype=np.int64), wc)
    within = np.arange(len(qid), dtype=np.int64) - np.repeat(np.cumsum(wc) - wc, wc)
    got = np.stack([qid, b.fids()[off.astype(np.int64)[qid] + within].astype(np.int64)], axis=1)
    return got[np.lexsort((got[:, 1], got[:, 0]))]


def _expected_level(config, threads, kind):
    if config != "tight":
        return 2 if config == "fine" else 1
    return 2 if kind == "roots" or (kind == "segbase" and threads == 1024) else 1


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("mode", list(OverlapMode))
def test_every_filter_level_answers_like_the_oracle(world, mode, invert, config):
    ix = world.ix[config]
    assert ix.options() == {k: int(v) for k, v in CONFIGS[config][0].items()}
    runs = mode != OverlapMode.Overlap or not invert  # (Overlap inverted keeps nothing: no kernel runs)
    for threads in (512, 1024):
        b = engine.QueryBatch(ix, max(SIZES))
        b.set_option("WIN_THREADS", threads)
        b.set_option("WIN_WIDE", 0)  # (the narrow form for every batch, whatever its sample of widths says: the mixed form reads no filter)
        b.set_option("WIN_FILTER", CONFIGS[config][1])
        for n in SIZES:
            want_c, want_pairs, want_roots = world.oracle(n, mode, invert)
            b.set_regions(world.regions[n])
            for kind, flags in (("segbase", engine.OUT_FIDS | engine.OUT_SEGBASE), ("offsets", engine.OUT_FIDS | engine.OUT_OFFSETS)):
                b.run(mode, invert, flags, engine.STRATEGY_WINDOWS)
                b.wait()
                c = b.counts()
                assert np.array_equal(c, want_c), (threads, n, kind)
                assert b.total_hits == len(want_pairs)
                off = b.offsets_from_segbase(c) if kind == "segbase" else b.offsets()[:-1]
                assert np.array_equal(_pairs_of(b, c, off), want_pairs), (threads, n, kind)
                if runs:
                    assert (b.block_threads, b.filter_level) == (threads, _expected_level(config, threads, kind)), (threads, n, kind)
            b.run(mode, invert, engine.OUT_ROOT_BITMAP | engine.OUT_NO_COUNTS, engine.STRATEGY_WINDOWS)
            b.wait()
            assert np.array_equal(b.unique_roots(), want_roots), (threads, n)
            if runs:
                assert b.filter_level == _expected_level(config, threads, "roots"), (threads, n)
        b.close()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_a_seqid_out_of_range_is_an_error_at_every_level(world, config):
    regions = world.regions[257].copy()
    regions[100, 0] = len(CHROMS)
    b = engine.QueryBatch(world.ix[config], len(regions))
    b.set_option("WIN_WIDE", 0)
    b.set_option("WIN_FILTER", CONFIGS[config][1])
    b.set_regions(regions)
    with pytest.raises(engine._ffi.GffxHipError) as ei:
        b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_SEGBASE, engine.STRATEGY_WINDOWS)
        b.wait()
    assert ei.value.code == -5
    b.close()


def test_the_engines_choice_by_rounds_per_block(world):
    """left to the engine (GFFX_HIP_WIN_FILTER=0) a launch takes the fine level only when its blocks run four rounds or more -- the
    larger bitmap is staged once per block --: a small launch takes the coarse one, 4 Mi regions alone at 1024 threads the fine one"""
    b = engine.QueryBatch(world.ix["fine"], 1 << 22)
    b.set_option("WIN_WIDE", 0)
    b.set_regions(world.regions[5000])
    b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_SEGBASE, engine.STRATEGY_WINDOWS)
    b.wait()
    want_c = world.oracle(5000, OverlapMode.Overlap, False)[0]
    assert b.filter_level == 1 and np.array_equal(b.counts(), want_c)
    reps = (1 << 22) // 4096
    b.set_regions(np.ascontiguousarray(np.tile(world.regions[5000][:4096], (reps, 1))))
    b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_SEGBASE, engine.STRATEGY_WINDOWS)
    b.wait()
    assert (b.block_threads, b.filter_level) == (1024, 2) and np.array_equal(b.counts(), np.tile(want_c[:4096], reps))
    b.set_regions(np.ascontiguousarray(np.tile(world.regions[5000][:4096], (reps - 1, 1))))
    b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_SEGBASE, engine.STRATEGY_WINDOWS)
    b.wait()
    assert (b.block_threads, b.filter_level) == (1024, 1) and np.array_equal(b.counts(), np.tile(want_c[:4096], reps - 1))
    b.close()


def test_a_cloned_index_carries_both_levels(world):
    """gffx_hip_index_clone copies the fine bitmap and its seqid records with the rest (here onto the same device)"""
    ix = world.ix["fine"].clone(0)
    n = 5000
    want_c, want_pairs, _ = world.oracle(n, OverlapMode.Overlap, False)
    b = engine.QueryBatch(ix, n)
    b.set_option("WIN_WIDE", 0)
    b.set_option("WIN_FILTER", 2)
    b.set_regions(world.regions[n])
    b.run(OverlapMode.Overlap, False, engine.OUT_FIDS | engine.OUT_SEGBASE, engine.STRATEGY_WINDOWS)
    b.wait()
    c = b.counts()
    assert np.array_equal(c, want_c) and b.filter_level == 2
    assert np.array_equal(_pairs_of(b, c, b.offsets_from_segbase(c)), want_pairs)
    b.close()
    ix.close()
