"""Measures `gffx closest` on the GENCODE-shaped synthetic index and 1 M synthetic regions that bench.py uses
(synth.gencode_like_roots(63000, seed=42), synth.synth_bed(1_000_000, seed=1001)).

Protocol.  Kernel times are HIP-event times of the handle's two kernels (gffx_hip_closest_last_kernel_ms: k_closest_count +
k_closest_emit; the host's wait between them, which sizes the pair buffer, is outside the events): one warm-up run per flag
combination, then --repeats timed runs; median and min .. max.  Beside them, on the same batch:
    direct sibling   the DIRECT strategy's Overlap pass with GFFX_OUT_TRIPLES | GFFX_OUT_OFFSETS (k_join_count + k_join_emit,
                     the same launch structure), their HIP-event times under the batch's profiling
    one host core    tools/closest_check.cpp built -O2 (`make closest_host_baseline`): device/closest_core.hpp over the same
                     roots and regions, the answer loop only, pinned to one core
    end table        HIP-event time of the build at gffx_hip_closest_create (keys kernel, device sort, unpack), one per handle
    CLI wall clock   `gffx closest -b` on a 1 M-row BED beside `gffx intersect -b -e` on the same file (index built before,
                     page cache warm, best of two)
Algorithm bytes per region: 12 in + 4 (count) + 4 (gap) + 8 (offset) + 12 per answered root out; over the median time as a
share of 8 TB/s -- the kernels are bound by the latency of dependent gathers, not by that figure.
Nothing here is a pass/fail number.  Prints a text table (kept as profiles/closest.txt) and one JSON line.
Usage: python tools/closest_bench.py [--genes 63000] [--regions 1000000] [--repeats 7] [--dir DIR] [--no-cli]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
HBM_BPS = 8e12
COMBOS = [(ig, side) for ig in (False, True) for side in ("both", "left", "right")]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def host_baseline(d, roots, regions, flags):
    exe = os.path.join(ROOT, "gffx_amd", "bin", "closest_host_baseline")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "closest_host_baseline"], stdout=subprocess.DEVNULL)
    path = os.path.join(d, "vectors.txt")
    co = roots["chr_offsets"]
    seq = np.repeat(np.arange(len(co) - 1, dtype=np.int64), np.diff(co.astype(np.int64)))
    with open(path, "w") as f:
        f.write("n_seq %d\n" % (len(co) - 1))
        np.savetxt(f, np.stack([seq, roots["start"].astype(np.int64), roots["end"].astype(np.int64)], axis=1), fmt="root %d %d %d")
        q = np.concatenate([np.full((len(regions), 1), flags, np.int64), regions.astype(np.int64)], axis=1)
        np.savetxt(f, q, fmt="q %d %d %d %d")
    out = subprocess.run(["taskset", "-c", "0", exe, "--time", path], check=True, capture_output=True, text=True).stdout.split()
    return {"pairs": int(out[1]), "ms": float(out[3])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one, removed)")
    ap.add_argument("--no-cli", action="store_true", help="skip the CLI wall clocks (they write and index a GFF3 file)")
    a = ap.parse_args()
    assert a.repeats >= 5, "the protocol asks for at least 5 timed runs"
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="closest_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import engine, synth
    if engine.device_count() < 1:
        raise SystemExit("closest_bench needs an MI355X: no HIP device visible (nothing is measured on the CPU)")
    roots = synth.gencode_like_roots(a.genes, seed=42)
    regions = synth.synth_bed(a.regions, seed=1001)
    nq = len(regions)
    engine.warmup(0)
    ix = engine.TreeIndexData.from_roots(roots["chr_offsets"], roots["start"], roots["end"], roots["fid"], roots["names"])
    res = {"roots": int(ix.n_roots), "seqids": int(ix.n_chr), "regions": nq, "repeats": a.repeats}

    builds = []
    for rep in range(a.repeats + 1):
        cl = engine.Closest(ix, nq)
        if rep:
            builds.append(cl.stats()["build_ms"])
        if rep < a.repeats:
            cl.close()
    res["end_table_build_ms"] = spread(builds)

    res["combos"] = {}
    for ig, side in COMBOS:
        times, pairs, over = [], 0, 0
        for rep in range(a.repeats + 1):
            counts, offsets, triples, gaps = cl.run(regions, ig, side)
            if rep:
                times.append(cl.last_kernel_ms())
            pairs = int(offsets[-1])
            over = int(((gaps == 0) & (counts > 0)).sum())
        t = spread(times)
        nbytes = 28 * nq + 12 * pairs
        res["combos"]["%s/%s" % ("ignore" if ig else "default", side)] = {
            "kernel_ms": t, "answered_roots": pairs, "regions_answered_by_overlaps": over, "regions_without_answer": int((counts == 0).sum()),
            "algorithm_bytes": nbytes, "share_of_8TBps_pct": round(nbytes / (t["median"] * 1e-3) / HBM_BPS * 100, 3),
            "ns_per_region": round(1e6 * t["median"] / nq, 3)}
    res["pair_buffer_grows"] = cl.stats()["grows"]

    # the fair sibling: the DIRECT strategy's Overlap pass with triples and offsets, the same batch, the same launch structure
    b = engine.QueryBatch(ix, nq)
    b.set_regions(regions)
    flags = engine.OUT_TRIPLES | engine.OUT_OFFSETS
    b.run(engine.OverlapMode.Overlap, False, flags, engine.STRATEGY_DIRECT)
    b.wait()
    times = []
    for rep in range(a.repeats):
        b.set_profiling(True)
        b.reset_profile()
        b.run(engine.OverlapMode.Overlap, False, flags, engine.STRATEGY_DIRECT)
        b.wait()
        b.set_profiling(False)
        times.append(b.kernel_ms(engine.K_JOIN_COUNT)[0] + b.kernel_ms(engine.K_JOIN_EMIT)[0])
    res["direct_overlap_triples"] = {"kernel_ms": spread(times), "pairs": int(b.total_hits)}
    b.close()

    res["host_one_core"] = {"default/both": host_baseline(a.dir, roots, regions, 0), "ignore/both": host_baseline(a.dir, roots, regions, 1)}
    assert res["host_one_core"]["default/both"]["pairs"] == res["combos"]["default/both"]["answered_roots"], "host and device count different answers"
    assert res["host_one_core"]["ignore/both"]["pairs"] == res["combos"]["ignore/both"]["answered_roots"], "host and device count different answers"
    cl.close()

    if not a.no_cli:
        synth.build_synth_text()
        gff, bed = os.path.join(a.dir, "anno.gff"), os.path.join(a.dir, "q.bed")
        synth.write_gff3_fast(gff, roots)
        synth.write_bed_fast(bed, regions, roots["names"])
        subprocess.run([GFFX, "index", "-i", gff], check=True, capture_output=True)
        res["cli_s"] = {}
        for label, cmd in (("closest -b", ["closest", "-i", gff, "-b", bed]), ("closest -b --ignore-overlaps", ["closest", "-i", gff, "-b", bed, "--ignore-overlaps"]),
                           ("intersect -b -e", ["intersect", "-i", gff, "-b", bed, "-e"])):
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                subprocess.run([GFFX] + cmd + ["-o", os.path.join(a.dir, "out.txt")], check=True, capture_output=True)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            res["cli_s"][label] = round(best, 3)
            res.setdefault("cli_out_MB", {})[label] = round(os.path.getsize(os.path.join(a.dir, "out.txt")) / 1e6, 1)

    print("gffx closest: %d regions x %d roots on %d seqids; one warm-up, then %d timed runs, median [min .. max]" % (nq, res["roots"], res["seqids"], a.repeats))
    e = res["end_table_build_ms"]
    print("end table build (k_closest_keys + device sort + k_closest_unpack)   %.3f ms [%.3f .. %.3f]" % (e["median"], e["min"], e["max"]))
    for name, o in res["combos"].items():
        t = o["kernel_ms"]
        print("%-14s k_closest_count + k_closest_emit  %.3f ms [%.3f .. %.3f]  %.2f ns/region  %d answered roots (%d regions by overlaps, %d without answer)"
              "  algorithm bytes %.1f MB = %s %% of 8 TB/s" % (name, t["median"], t["min"], t["max"], o["ns_per_region"], o["answered_roots"],
                                                             o["regions_answered_by_overlaps"], o["regions_without_answer"], o["algorithm_bytes"] / 1e6,
                                                             o["share_of_8TBps_pct"]))
    d = res["direct_overlap_triples"]
    print("direct sibling k_join_count + k_join_emit (Overlap, triples + offsets)  %.3f ms [%.3f .. %.3f]  %d pairs"
          % (d["kernel_ms"]["median"], d["kernel_ms"]["min"], d["kernel_ms"]["max"], d["pairs"]))
    for name, h in res["host_one_core"].items():
        print("one host core, closest_core.hpp -O2, %-13s %.1f ms (%d answered roots)" % (name, h["ms"], h["pairs"]))
    for label, s in res.get("cli_s", {}).items():
        print("CLI wall clock  gffx %-30s %.3f s  (%.1f MB out)" % (label, s, res["cli_out_MB"][label]))
    print("pair buffer grown %d time(s) over all runs" % res["pair_buffer_grows"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
