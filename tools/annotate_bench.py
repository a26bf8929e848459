"""Measures `gffx annotate` on the GENCODE-shaped synthetic annotation (synth.gencode_like_roots(63000, seed=5) written by
synth.write_gff3_fast: 3.56 M lines of types gene, mRNA, exon, CDS) and 1 M synthetic regions (synth.synth_bed(1_000_000,
seed=1001)), five layers: CDS, five_prime_UTR (no line carries it: an empty layer), exon, mRNA, gene.

Protocol.  One warm-up, then --repeats timed runs; median and min .. max.
    build            HIP-event times of the class map's stages (gffx_hip_classmap_stage_ms: union, toggles, sort, scan, points,
                     bases), a fresh object per run, all rows in one call
    k_classmap_regions   HIP-event time of the kernel (gffx_hip_classmap_last_kernel_ms), and the wall clock of the whole
                     run_host call (regions in, counts and class bytes out) beside it
    T-pass route     the same counts from code that exists without this command: T cumulative unions (layers 0 .. k) and one
                     gffx_hip_union_segments_covered per union, bases_k = covered_k - covered_{k-1}.  That entry point copies
                     its segments in and its answer out and exposes no event time, so its figure is the WALL CLOCK of the T
                     calls, to be read beside the wall clock of run_host, not beside the kernel time.  The counts are compared.
    one host core    tools/classmap_check.cpp built -O2 (`make classmap_host_baseline`): device/classmap_core.hpp's region rule
                     over the same points and regions, the answer loop only, pinned to one core
    CLI wall clock   `gffx annotate -b` beside `gffx closest -b` on the same 1 M-row BED (index built before, page cache warm,
                     best of two)
Nothing here is a pass/fail number.  Prints a text table (kept as profiles/annotate.txt) and one JSON line.
Usage: python tools/annotate_bench.py [--genes 63000] [--regions 1000000] [--repeats 7] [--dir DIR] [--no-cli] [--no-host]"""
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
LAYERS = ["CDS", "five_prime_UTR", "exon", "mRNA", "gene"]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def show(s):
    return "%.3f ms [%.3f .. %.3f]" % (s["median"], s["min"], s["max"])


def layer_rows(gff, names):
    """(layer, seqid, start - 1, end) of every line whose type is a layer, as the command takes them."""
    seq_of = {n.encode(): i for i, n in enumerate(names)}
    layer_of = {n.encode(): i for i, n in enumerate(LAYERS)}
    out = []
    with open(gff, "rb") as f:
        for line in f:
            if line[:1] == b"#":
                continue
            p = line.split(b"\t", 5)
            k = layer_of.get(p[2])
            if k is not None:
                out.append((k, seq_of[p[0]], int(p[3]) - 1, int(p[4])))
    return np.array(out, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one, removed)")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="annotate_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import engine, synth
    if engine.device_count() < 1:
        raise SystemExit("annotate_bench needs an MI355X: no HIP device visible (nothing is measured on the CPU)")
    synth.build_synth_text()
    roots = synth.gencode_like_roots(a.genes, seed=5)
    names = list(roots["names"])
    n_seq, T = len(names), len(LAYERS)
    gff, bed = os.path.join(a.dir, "anno.gff"), os.path.join(a.dir, "q.bed")
    synth.write_gff3_fast(gff, roots, seed=5)
    regions = synth.synth_bed(a.regions, seed=1001)
    nq = len(regions)
    rows = layer_rows(gff, names)
    engine.warmup(0)
    res = {"lines": sum(1 for _ in open(gff, "rb")), "layer_rows": len(rows), "rows_per_layer": np.bincount(rows[:, 0], minlength=T).tolist(),
           "seqids": n_seq, "layers": LAYERS, "regions": nq, "repeats": a.repeats}

    stages = {}
    m = None
    for rep in range(a.repeats + 1):
        if m is not None:
            m.close()
        m = engine.ClassMap(n_seq, T)
        m.add_rows(rows)
        m.finish()
        if rep:
            for k, v in m.stage_ms().items():
                stages.setdefault(k, []).append(v)
    res["build_ms"] = {k: spread(v) for k, v in stages.items()}
    res["build_total_ms"] = spread([sum(v[i] for v in stages.values()) for i in range(a.repeats)])
    res["points"] = m.n_points

    kern, wall = [], []
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        counts, cls = m.run(regions)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            kern.append(m.last_kernel_ms())
            wall.append(dt)
    res["k_classmap_regions_ms"] = spread(kern)
    res["run_host_wall_ms"] = spread(wall)
    res["ns_per_region"] = round(1e6 * res["k_classmap_regions_ms"]["median"] / nq, 3)
    res["class_histogram"] = np.bincount(cls, minlength=T + 1).tolist()

    # the T-pass route: cumulative unions, one segments_covered per layer
    unions = []
    for k in range(T):
        u = engine.RegionUnion(n_seq)
        part = rows[rows[:, 0] <= k]
        if len(part):
            u.add(np.ascontiguousarray(part[:, 1:]))
        u.finish()
        unions.append(u)
    ok = regions[:, 1] < regions[:, 2]
    q, s, e = (np.ascontiguousarray(regions[:, i]) for i in range(3))
    e = np.where(ok, e, s).astype(np.uint32)  # (an inverted row covers nothing)
    tpass = []
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        cov = [u.segments_covered(q, s, e) for u in unions]
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            tpass.append(dt)
    res["t_pass_wall_ms"] = spread(tpass)
    prev = np.zeros(nq, np.int64)
    for k in range(T):
        assert np.array_equal(cov[k].astype(np.int64) - prev, counts[:, k].astype(np.int64)), "the two routes disagree on layer %d" % k
        prev = cov[k].astype(np.int64)
    for u in unions:
        u.close()

    if not a.no_host:
        exe = os.path.join(ROOT, "gffx_amd", "bin", "classmap_host_baseline")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "classmap_host_baseline"], stdout=subprocess.DEVNULL)
        path = os.path.join(a.dir, "case.txt")
        with open(path, "w") as f:
            f.write("n_seq %d\nlayers %d\n" % (n_seq, T))
            np.savetxt(f, rows.astype(np.int64), fmt="row %d %d %d %d")
            np.savetxt(f, regions.astype(np.int64), fmt="q %d %d %d")
        out = subprocess.run(["taskset", "-c", "0", exe, "--time", path], check=True, capture_output=True, text=True).stdout.split()
        res["host_one_core"] = {"points": int(out[1]), "ms": float(out[5])}
        assert res["host_one_core"]["points"] == res["points"], "host and device build different maps"
    m.close()

    if not a.no_cli:
        synth.write_bed_fast(bed, regions, roots["names"])
        subprocess.run([GFFX, "index", "-i", gff], check=True, capture_output=True)
        res["cli_s"] = {}
        for label, cmd in (("annotate -b -T " + ",".join(LAYERS), ["annotate", "-i", gff, "-b", bed, "-T", ",".join(LAYERS)]),
                           ("closest -b", ["closest", "-i", gff, "-b", bed])):
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                subprocess.run([GFFX] + cmd + ["-o", os.path.join(a.dir, "out.txt")], check=True, capture_output=True)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            res["cli_s"][label] = round(best, 3)
            res.setdefault("cli_out_MB", {})[label] = round(os.path.getsize(os.path.join(a.dir, "out.txt")) / 1e6, 1)

    print("gffx annotate: %d regions, %d layer rows of %d lines on %d seqids, %d layers (%s), %d points; one warm-up, then %d timed runs, median [min .. max]"
          % (nq, res["layer_rows"], res["lines"], n_seq, T, ",".join(LAYERS), res["points"], a.repeats))
    print("rows per layer %s; regions per class (the last is none) %s" % (res["rows_per_layer"], res["class_histogram"]))
    for k, v in res["build_ms"].items():
        print("build  %-11s %s" % (k[:-3], show(v)))
    print("build  total       %s" % show(res["build_total_ms"]))
    print("k_classmap_regions (HIP events)              %s  %.2f ns/region" % (show(res["k_classmap_regions_ms"]), res["ns_per_region"]))
    print("run_host wall clock (copies in and out)      %s" % show(res["run_host_wall_ms"]))
    print("T-pass route, %d x gffx_hip_union_segments_covered, wall clock (copies in and out)  %s" % (T, show(res["t_pass_wall_ms"])))
    if "host_one_core" in res:
        print("one host core, classmap_core.hpp -O2, region rule   %.1f ms" % res["host_one_core"]["ms"])
    for label, sec in res.get("cli_s", {}).items():
        print("CLI wall clock  gffx %-60s %.3f s  (%.1f MB out)" % (label, sec, res["cli_out_MB"][label]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
