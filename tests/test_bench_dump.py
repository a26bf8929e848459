"""bench.py --dump-outputs: the files hold every region's pairs in a form that does not depend on where the engine put the segments
(CPU), stay under the size cap with a fixed sample, and on the GPU hold what the oracle computes for the bench's seeded workload,
whatever --steps is."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scattered(counts, per_region, seed):
    """The pair buffer of a pass that placed the segments in a random order and each segment's pairs in a random order."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(counts))
    starts = np.zeros(len(counts), dtype=np.uint64)
    buf, at = [], 0
    for q in order:
        starts[q] = at
        buf.append(rng.permutation(per_region[q]))
        at += counts[q]
    return starts, np.concatenate(buf).astype(np.uint32)


def _load(d, names):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in names}


def test_dump_does_not_depend_on_segment_placement(tmp_path):
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 6, 3000).astype(np.uint32)
    per_region = [rng.integers(0, 60000, c) for c in counts]
    names = ("rows", "counts", "fids")
    got = []
    for seed in (1, 2):
        starts, fids = _scattered(counts, per_region, seed)
        files = bench.dump_outputs(str(tmp_path / str(seed)), counts, starts, fids)
        assert files == {"rows": [3000], "counts": [3000], "fids": [int(counts.sum())]}
        got.append(_load(str(tmp_path / str(seed)), names))
    for n in names:
        assert got[0][n].dtype == np.float64 and np.array_equal(got[0][n], got[1][n]), n
    want = np.concatenate([np.sort(p) for p in per_region])
    assert np.array_equal(got[0]["rows"], np.arange(3000)) and np.array_equal(got[0]["counts"], counts)
    assert np.array_equal(got[0]["fids"], want)


def test_dump_triples_sorted_inside_each_region(tmp_path):
    counts = np.array([2, 0, 3], dtype=np.uint32)
    starts = np.array([3, 0, 0], dtype=np.uint64)  # region 2's segment first
    trip = np.array([[9, 5, 6], [1, 7, 8], [9, 1, 2], [4, 4, 4], [2, 2, 2]], dtype=np.uint32)
    assert bench.dump_outputs(str(tmp_path), counts, starts, trip)["triples"] == [5, 3]
    got = np.load(str(tmp_path / "triples.npy"))
    assert np.array_equal(got, [[2, 2, 2], [4, 4, 4], [1, 7, 8], [9, 1, 2], [9, 5, 6]])


def test_dump_counts_only_pass(tmp_path):
    counts = np.array([1, 2, 3], dtype=np.uint32)
    assert bench.dump_outputs(str(tmp_path), counts, None, None) == {"rows": [3], "counts": [3]}
    assert sorted(os.listdir(tmp_path)) == ["counts.npy", "rows.npy"]


def test_dump_over_budget_is_a_fixed_sample(tmp_path):
    rng = np.random.default_rng(6)
    counts = rng.integers(0, 40, 20000).astype(np.uint32)
    per_region = [rng.integers(0, 60000, c) for c in counts]
    budget = 400_000
    samples = []
    for seed in (1, 2):  # a different placement of the same results: the same sample
        starts, fids = _scattered(counts, per_region, seed)
        d = str(tmp_path / str(seed))
        bench.dump_outputs(d, counts, starts, fids, budget=budget)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= budget
        samples.append(_load(d, ("rows", "counts", "fids")))
    s = samples[0]
    rows = s["rows"].astype(np.int64)
    assert 0 < len(rows) < len(counts) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, samples[1]["rows"]) and np.array_equal(s["fids"], samples[1]["fids"])
    assert np.array_equal(s["counts"], counts[rows])
    assert np.array_equal(s["fids"], np.concatenate([np.sort(per_region[q]) for q in rows]))


def _bench_dump(d, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--quick", "--steps", str(steps), "--warmup", "1",
                        "--repeats", "1", "--no-traffic", "--no-cpu-baseline", "--dump-outputs", d],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = json.loads(r.stdout)
    assert line["steps"] == steps and line["dump_outputs"]["dir"] == d
    return line


@pytest.mark.gpu
def test_bench_dump_matches_oracle_and_steps(tmp_path):
    from gffx_amd import synth
    from oracle import binding as ob

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench_dump(a, 1)
    _bench_dump(b, 3)
    names = ("rows", "counts", "fids")
    da, db = _load(a, names), _load(b, names)
    for n in names:  # the same inputs whatever the number of steps, and the same results
        assert np.array_equal(da[n], db[n]), n
    # the headline's workload (configs[1]) through the oracle
    roots = synth.gencode_like_roots(63000, seed=42)
    regions = synth.synth_bed(1_000_000, seed=1001)
    oix = ob.OracleIndex.from_roots(roots["chr_offsets"], roots["start"], roots["end"], roots["fid"])
    want, want_c = oix.query_features(regions, 2, False)
    assert line["config"]["kept_pairs_total"] == len(want)
    assert np.array_equal(da["rows"], np.arange(len(regions))) and np.array_equal(da["counts"], want_c)
    by_chr = np.argsort(regions[:, 0], kind="stable")  # the oracle's triples: regions by seqid, input order inside one
    rid = np.repeat(by_chr, want_c[by_chr].astype(np.int64))
    assert np.array_equal(da["fids"], want[np.lexsort((want[:, 0], rid)), 0])
