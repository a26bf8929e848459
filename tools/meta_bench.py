"""Measures `gffx meta` at scale: the GENCODE-shaped index of bench.py (63 002 roots; the features are the gene lines of the
synthetic text, strands included) and a seeded BED of N rows (width U[100, 10 000] over GRCh38-shaped chromosomes).

Per fold of 4 Mi rows, HIP events, the median of --reps folds after a warm-up fold:
  k_pileup_meta           point mode (UP = DOWN = 2000, BIN = 10: 400 columns) and scaled mode (UP = DOWN = 1000, BIN = 10, M = 100:
                          300 columns), each with and without the features x columns matrix
  the explicit route      what existed before: a Pileup over the G x B explicit clamped columns (k_pileup_segments), then the
                          totals copied back and the columns summed on the host; its column sums must equal the fused kernel's
  one host core           the definition through device/meta_core.hpp (bin/meta_host_baseline, `make meta_host_baseline`) on a
                          sample of the features against the same fold, scaled to all features: the evaluation of the bases
                          alone (no formatting, no widths inside the timed window)
and the wall clock of `gffx meta` beside `gffx coverage --mean-depth` on the same BED file (--runs each, all listed).
One JSON object on stdout.  The files are kept in --dir between runs.
Usage: python tools/meta_bench.py [--rows 10000000] [--genes 63000] [--seed 5] [--reps 5] [--runs 3] [--sample 10000] [--dir DIR]
                                  [--skip-cli] [--skip-explicit] [--skip-host]"""
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

U32_MAX = 2 ** 32 - 1


def gene_lines(gff, names):
    """(seq, start - 1, end, minus) of the gene lines, in file order."""
    num = {n.encode(): i for i, n in enumerate(names)}
    out = []
    with open(gff, "rb") as f:
        for ln in f:
            if ln[:1] == b"#":
                continue
            c = ln.split(b"\t", 7)
            if len(c) > 6 and c[2] == b"gene":
                out.append((num[c[0]], int(c[3]) - 1, int(c[4]), 1 if c[6] == b"-" else 0))
    return np.array(out, dtype=np.uint32).reshape(-1, 4)


def explicit_columns(feats, lay):
    """The G x B clamped columns of tests/_meta_definition.py, in numpy int64 (no length: the clamp is at 0 and 2^32 - 1)."""
    mode, anchor, up, down, bin_, m = lay
    s, e, minus = feats[:, 1].astype(np.int64)[:, None], feats[:, 2].astype(np.int64)[:, None], feats[:, 3].astype(bool)[:, None]
    L = e - s
    if mode == 0:
        a0 = (0 * L, L, L // 2)[anchor]
        t = a0 - up + np.arange((up + down) // bin_ + 1, dtype=np.int64)[None, :] * bin_
    else:
        t = np.concatenate([-up + np.arange(up // bin_, dtype=np.int64)[None, :] * bin_ + 0 * L, (np.arange(m + 1, dtype=np.int64)[None, :] * L) // m,
                            L + np.arange(1, down // bin_ + 1, dtype=np.int64)[None, :] * bin_], axis=1)
    g = np.clip(np.where(minus, e - t, s + t), 0, U32_MAX)
    a = np.where(minus, g[:, 1:], g[:, :-1]).astype(np.uint32)
    b = np.where(minus, g[:, :-1], g[:, 1:]).astype(np.uint32)
    q = np.repeat(feats[:, 0], a.shape[1]).astype(np.uint32)
    return q, a.ravel(), b.ravel()


def median_of_folds(add_fold, read_ms, reps):
    """ms per fold: the differences of a running HIP-event total over reps folds, after one warm-up fold."""
    add_fold()
    seen, per = read_ms(), []
    for _ in range(reps):
        add_fold()
        now = read_ms()
        per.append(now - seen)
        seen = now
    return {"median_ms": round(statistics.median(per), 4), "folds_ms": [round(x, 4) for x in per]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sample", type=int, default=10000, help="features of the one-core host run")
    ap.add_argument("--dir", default=None, help="directory for the files (default: a temporary one, removed)")
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--skip-explicit", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="meta_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from coverage_bench import write_bed
    from gffx_amd import engine, synth
    gffx = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
    roots = synth.gencode_like_roots(a.genes, seed=a.seed)
    names = roots["names"]
    gff = os.path.join(a.dir, "genes_%d_%d.gff" % (a.genes, a.seed))
    if not os.path.exists(gff + ".gof"):
        synth.write_gff3_fast(gff, roots, seed=a.seed)
        subprocess.check_call([gffx, "index", "-i", gff])
    bed = os.path.join(a.dir, "rows_%d_%d.bed" % (a.rows, a.seed))
    if not os.path.exists(bed):
        write_bed(bed, a.rows, a.seed + 1, names, synth)
    feats = gene_lines(gff, names)
    G, n_seq = len(feats), len(names)
    fold = min(engine.PILEUP_FOLD, a.rows)
    rows = synth.synth_bed(fold, seed=a.seed + 1)  # (the first piece of the file's rows)
    rows = np.ascontiguousarray(rows[rows[:, 1] < rows[:, 2]])
    res = {"features": G, "minus": int(feats[:, 3].sum()), "fold_rows": len(rows), "reps": a.reps, "configs": {}}
    layouts = {"point_2000_2000_10": (0, 0, 2000, 2000, 10, 0), "scaled_1000_1000_10_100": (1, 0, 1000, 1000, 10, 100)}
    for name, lay in layouts.items():
        cfg = {"columns": engine.MetaLayout(*lay).columns}
        totals = {}
        for keep in (False, True):
            p = engine.Pileup(n_seq, [], [], [])
            p.meta_set(feats[:, 0], feats[:, 1], feats[:, 2], feats[:, 3], engine.MetaLayout(*lay), keep_matrix=keep)
            m = median_of_folds(lambda: p.add(rows), p.meta_ms, a.reps)
            st = p.stats()
            m["fold_without_meta_ms"] = round(st["kernel_ms"] / st["folds"], 4)  # keys, sorts, prefix sums (no segments here)
            m["boundaries_per_fold"] = G * (cfg["columns"] + 1)
            totals[keep] = p.meta()[0] // np.uint64(a.reps + 1)
            p.close()
            cfg["k_pileup_meta_matrix" if keep else "k_pileup_meta"] = m
        assert np.array_equal(totals[False], totals[True])
        if not a.skip_explicit:
            t0 = time.perf_counter()
            q, lo, hi = explicit_columns(feats, lay)
            build_s = time.perf_counter() - t0
            p = engine.Pileup(n_seq, q, lo, hi)
            m = median_of_folds(lambda: p.add(rows), lambda: p.stats()["segments_ms"], a.reps)
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                sums = p.bases().reshape(G, -1).sum(0, dtype=np.uint64)
                host.append(round((time.perf_counter() - t0) * 1e3, 3))
            p.close()
            assert np.array_equal(sums // np.uint64(a.reps + 1), totals[False]), "the explicit route and the fused kernel disagree"
            m.update(segments=len(q), build_segments_host_s=round(build_s, 3), copy_and_column_sums_host_ms=host)
            cfg["explicit_k_pileup_segments"] = m
        if not a.skip_host:
            tool = os.path.join(ROOT, "gffx_amd", "bin", "meta_host_baseline")
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "meta_host_baseline"], stdout=subprocess.DEVNULL)
            pick = np.sort(np.random.default_rng(a.seed).choice(G, min(a.sample, G), replace=False))
            case = os.path.join(a.dir, "host_case.txt")
            with open(case, "w") as f:
                f.write("n_seq %d\nlayout %d %d %d %d %d %d\n" % ((n_seq,) + lay))
                np.savetxt(f, rows, fmt="row %d %d %d")
                np.savetxt(f, feats[pick], fmt="feat %d %d %d %d")
            takes, geometry = [], []
            for _ in range(3):
                r = subprocess.run([tool, case], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, check=True)
                timed = dict(ln.split() for ln in r.stderr.decode().splitlines() if ln.startswith(("ms ", "geometry_ms ")))
                takes.append(float(timed["ms"]))  # the bases alone: boundaries, searches, differences, column sums; nothing is formatted inside
                geometry.append(float(timed["geometry_ms"]))
            ms = statistics.median(takes)
            cfg["one_host_core"] = {"sample": len(pick), "sample_ms": round(ms, 3), "takes_ms": takes, "all_features_ms": round(ms * G / len(pick), 1),
                                    "sample_geometry_ms": statistics.median(geometry)}
            os.remove(case)
        res["configs"][name] = cfg
        sys.stderr.write("%s: %s\n" % (name, json.dumps(cfg)))
    if not a.skip_cli:
        out = os.path.join(a.dir, "out.tsv")
        cmds = {"meta_point": [gffx, "meta", "-i", gff, "-s", bed, "-o", out],
                "meta_scaled": [gffx, "meta", "-i", gff, "-s", bed, "-o", out, "--scale", "100", "-u", "1000", "-d", "1000"],
                "meta_point_matrix": [gffx, "meta", "-i", gff, "-s", bed, "-o", out, "--matrix", os.path.join(a.dir, "matrix.tsv")],
                "coverage_mean_depth": [gffx, "coverage", "-i", gff, "-s", bed, "-o", out, "--mean-depth"]}
        res["wall_s"] = {}
        for name, cmd in cmds.items():
            walls = []
            for _ in range(max(1, a.runs)):
                t0 = time.time()
                r = subprocess.run(cmd, capture_output=True)
                walls.append(round(time.time() - t0, 3))
                if r.returncode != 0:
                    sys.stderr.write(r.stderr.decode(errors="replace"))
                    sys.exit(r.returncode)
            res["wall_s"][name] = walls
        res["rows"], res["bed_bytes"] = a.rows, os.path.getsize(bed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
