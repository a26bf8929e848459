"""Measures `gffx enrich` on the workload of tools/annotate_bench.py: the GENCODE-shaped synthetic annotation
(synth.gencode_like_roots(63000, seed=5): 3.56 M lines), five layers (CDS, five_prime_UTR, exon, mRNA, gene) and 1 M synthetic
regions (synth.synth_bed(1_000_000, seed=1001)); a seqid's length is the largest end of its rows and regions.

Protocol.  One warm-up, then --repeats timed runs; median and min .. max, all from HIP events on the object's stream.
    k_classmap_permute   gffx_hip_classmap_perm_last_kernel_ms of one perm_run over all regions (the range check and the
                     permute launches), for every N of --perms; per placement = time / (regions x (N + 1))
    (a) the route without it   k_classmap_regions (gffx_hip_classmap_last_kernel_ms) over regions placed on the host, once per
                     permutation, --route-perms permutations per timed run: its KERNEL time only -- not the placement on the
                     host, not the copies of the regions in and of (T + 1) x 4 + 1 bytes per region out, not the sums on the
                     host -- which is generous to it.  Per region = time / (regions x permutations).  Its counts, summed on the
                     host, must equal the rows of the new kernel's matrices (compared).
    (b) one host core  tools/enrich_check.cpp built -O2 (`make enrich_host_baseline`): device/enrich_core.hpp over the same
                     points, sums and regions, --host-perms permutations, pinned to one core; the figure for N = 1000 is that
                     time SCALED linearly by rows (said so where it is printed)
    CLI wall clock   `gffx enrich -n <largest N>` beside `gffx annotate` on the same 1 M-row BED (index built before, page
                     cache warm, best of two)
Nothing here is a pass/fail number.  Prints a text table (kept as profiles/enrich.txt) and one JSON line.
Usage: python tools/enrich_bench.py [--genes 63000] [--regions 1000000] [--perms 100,1000] [--repeats 5] [--dir DIR] [--no-cli] [--no-host]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
GOLD = np.uint64(0x9E3779B97F4A7C15)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def show(s):
    return "%.3f ms [%.3f .. %.3f]" % (s["median"], s["min"], s["max"])


def mix64(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def place_on_host(regions, seq_len, p, seed):
    """Row p of the definition (device/enrich_core.hpp) in numpy's wrapping 64-bit arithmetic."""
    with np.errstate(over="ignore"):
        key = mix64(np.array([seed], np.uint64) + GOLD * np.uint64(p))
        r = mix64(key + GOLD * (np.arange(len(regions), dtype=np.uint64) + np.uint64(1)))
        qs, qe = regions[:, 1].astype(np.uint64), regions[:, 2].astype(np.uint64)
        L = seq_len[regions[:, 0]].astype(np.uint64)
        w = np.where(qe > qs, qe - qs, 0).astype(np.uint64)
        movable = (qe > qs) & (w <= L)
        span = np.where(movable, L - w + np.uint64(1), np.uint64(1))
        # the high half of r x span for span < 2^32, from two 32-bit halves of r
        hi = ((r >> np.uint64(32)) * span + (((r & np.uint64(0xFFFFFFFF)) * span) >> np.uint64(32))) >> np.uint64(32)
    out = regions.copy()
    out[movable, 1] = hi[movable].astype(np.uint32)
    out[movable, 2] = (hi[movable] + w[movable]).astype(np.uint32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--perms", default="100,1000")
    ap.add_argument("--route-perms", type=int, default=8)
    ap.add_argument("--host-perms", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one, removed)")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="enrich_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from annotate_bench import LAYERS, layer_rows
    from gffx_amd import engine, synth
    if engine.device_count() < 1:
        raise SystemExit("enrich_bench needs an MI355X: no HIP device visible (nothing is measured on the CPU)")
    perms = [int(x) for x in a.perms.split(",")]
    synth.build_synth_text()
    roots = synth.gencode_like_roots(a.genes, seed=5)
    names = list(roots["names"])
    n_seq, T = len(names), len(LAYERS)
    gff, bed = os.path.join(a.dir, "anno.gff"), os.path.join(a.dir, "q.bed")
    synth.write_gff3_fast(gff, roots, seed=5)
    regions = synth.synth_bed(a.regions, seed=1001)
    nq = len(regions)
    rows = layer_rows(gff, names)
    seq_len = np.zeros(n_seq, np.uint32)
    np.maximum.at(seq_len, rows[:, 1], rows[:, 3])
    np.maximum.at(seq_len, regions[:, 0], regions[:, 2])
    engine.warmup(0)
    m = engine.ClassMap(n_seq, T)
    m.add_rows(rows)
    m.finish()
    G, block = engine._enrich_constants()
    res = {"layer_rows": len(rows), "seqids": n_seq, "layers": LAYERS, "regions": nq, "points": m.n_points, "repeats": a.repeats, "seed": a.seed,
           "rows_per_block": G, "regions_per_block": block}

    res["k_classmap_permute_ms"], res["ns_per_placement"], totals = {}, {}, {}
    for N in perms:
        kern = []
        for rep in range(a.repeats + 1):
            m.perm_begin(seq_len, N, a.seed)
            m.perm_run(regions, 0)
            totals[N] = m.perm_totals()
            if rep:
                kern.append(m.perm_last_kernel_ms())
        res["k_classmap_permute_ms"][str(N)] = spread(kern)
        res["ns_per_placement"][str(N)] = {k: round(1e6 * v / (nq * (N + 1)), 4) for k, v in spread(kern).items()}
    res["unplaced"] = totals[perms[0]][2]
    for N in perms[1:]:  # (row p does not depend on N)
        assert np.array_equal(totals[N][0][:perms[0] + 1], totals[perms[0]][0]), "the rows of two N disagree"

    # (a) k_classmap_regions once per permutation over host-placed regions: its kernel time, and its sums against the matrices
    B, R, _ = totals[perms[0]]
    route = []
    for rep in range(a.repeats + 1):
        ms = 0.0
        for p in range(1, a.route_perms + 1):
            counts, cls = m.run(place_on_host(regions, seq_len, p, a.seed))
            ms += m.last_kernel_ms()
            if rep == 0:
                assert np.array_equal(counts.sum(0, dtype=np.uint64), B[p]) and np.array_equal(np.bincount(cls, minlength=T + 1).astype(np.uint64), R[p]), \
                    "the two routes disagree on row %d" % p
        if rep:
            route.append(ms)
    res["route_k_classmap_regions_ms"] = spread(route)
    res["route_perms"] = a.route_perms
    res["route_ns_per_region"] = {k: round(1e6 * v / (nq * a.route_perms), 4) for k, v in spread(route).items()}

    if not a.no_host:
        exe = os.path.join(ROOT, "gffx_amd", "bin", "enrich_host_baseline")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "enrich_host_baseline"], stdout=subprocess.DEVNULL)
        p_off, pos, cls = m.points()
        cb = m.bases()
        seq = np.repeat(np.arange(n_seq), np.diff(p_off.astype(np.int64)))
        path = os.path.join(a.dir, "case.txt")
        with open(path, "w") as f:
            f.write("n_seq %d\nlayers %d\nperms %d\nseed %d\n" % (n_seq, T, a.host_perms, a.seed))
            np.savetxt(f, np.stack([np.arange(n_seq), seq_len.astype(np.int64)], 1), fmt="len %d %d")
            np.savetxt(f, np.stack([seq, pos.astype(np.int64), cls.astype(np.int64)], 1), fmt="p %d %d %d")
            np.savetxt(f, np.concatenate([np.arange(len(pos))[:, None], cb.T.astype(np.int64)], 1), fmt="cb" + " %d" * (T + 1))
            np.savetxt(f, regions.astype(np.int64), fmt="q %d %d %d")
        out = subprocess.run(["taskset", "-c", "0", exe, "--time", path], check=True, capture_output=True, text=True).stdout.split()
        ms = float(out[5])
        res["host_one_core"] = {"perms": a.host_perms, "ms": ms, "ns_per_placement": round(1e6 * ms / (nq * (a.host_perms + 1)), 2),
                                "scaled_to": {str(N): round(ms * (N + 1) / (a.host_perms + 1) / 1e3, 1) for N in perms}}
    m.close()

    if not a.no_cli:
        synth.write_bed_fast(bed, regions, roots["names"])
        subprocess.run([GFFX, "index", "-i", gff], check=True, capture_output=True)
        genome = os.path.join(a.dir, "genome.txt")
        with open(genome, "w") as f:
            f.write("".join("%s\t%d\n" % (n, L) for n, L in zip(names, seq_len.tolist())))
        res["cli_s"] = {}
        big = max(perms)
        for label, cmd in (("enrich -b -n %d -g -T %s" % (big, ",".join(LAYERS)), ["enrich", "-i", gff, "-b", bed, "-T", ",".join(LAYERS), "-n", str(big), "-g", genome,
                                                                                  "--seed", str(a.seed)]),
                           ("annotate -b -T " + ",".join(LAYERS), ["annotate", "-i", gff, "-b", bed, "-T", ",".join(LAYERS)])):
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                subprocess.run([GFFX] + cmd + ["-o", os.path.join(a.dir, "out.txt")], check=True, capture_output=True)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            res["cli_s"][label] = round(best, 3)

    print("gffx enrich: %d regions, %d layer rows on %d seqids, %d layers (%s), %d points, %d unplaced; %d rows x %d regions per block; one warm-up, then %d timed "
          "runs, median [min .. max], HIP events" % (nq, res["layer_rows"], n_seq, T, ",".join(LAYERS), res["points"], res["unplaced"], G, block, a.repeats))
    for N in perms:
        s, n = res["k_classmap_permute_ms"][str(N)], res["ns_per_placement"][str(N)]
        print("k_classmap_permute  N = %-5d %s  %.4f ns/placement [%.4f .. %.4f]" % (N, show(s), n["median"], n["min"], n["max"]))
    n = res["route_ns_per_region"]
    print("(a) k_classmap_regions x %d permutations placed on the host, kernel time only  %s  %.4f ns/region [%.4f .. %.4f]"
          % (a.route_perms, show(res["route_k_classmap_regions_ms"]), n["median"], n["min"], n["max"]))
    if "host_one_core" in res:
        h = res["host_one_core"]
        print("(b) one host core, enrich_core.hpp -O2, N = %d: %.1f ms, %.2f ns/placement; SCALED linearly by rows: %s"
              % (h["perms"], h["ms"], h["ns_per_placement"], ", ".join("N = %s: %s s" % kv for kv in h["scaled_to"].items())))
    for label, sec in res.get("cli_s", {}).items():
        print("CLI wall clock  gffx %-70s %.3f s" % (label, sec))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
