"""Measures `gffx index` (the host path: the parent commit's code) against `gffx index --gpu` on the GENCODE-shaped synthetic GFF3
that bench.py writes (synth.write_gff3_fast around gencode_like_roots(63000, seed=42): ~3.5 M lines, ~290 MB).

Protocol.  Both paths are the same binary and write into a directory of their own; the page cache is warm
(one untimed run of each first); --repeats runs each (at least five), wall clock of the whole process, median and min .. max:
    once with GFFX_LINE_TABLE=off      the eight side-cars alone
    once with the default              with `.lsoa` / `.lall` built after them (the same host code for both paths)
After the first pair of runs the eight side-cars of the two directories are compared byte for byte.
Device stages: HIP-event times of engine.GffIndexer.stage_ms over the same text (one warm-up, then --repeats runs; median).
Roofline: the text's bytes over 8 TB/s, against the line scan plus the rows kernels (each reads the text twice: the share
is of one read).  Nothing here is a pass/fail number.  Not measured: the Rust binary (it cannot be built here), HBM counters.
Usage: python tools/index_bench.py [--genes 63000] [--repeats 5] [--dir DIR] [--out profiles/index.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gffx_amd import engine, synth  # noqa: E402

GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
HBM_BPS = 8e12
SIDE_CARS = (".fts", ".prt", ".a2f", ".atn", ".sqs", ".gof", ".rit", ".rix")


def say(out, s):
    out.append(s)
    print(s, flush=True)


def wall(gff, gpu, env, reps):
    t = []
    for i in range(reps + 1):  # the first run is the warm-up
        t0 = time.perf_counter()
        r = subprocess.run([GFFX, "index", "-i", gff] + (["--gpu"] if gpu else []), capture_output=True, env=dict(os.environ, **env))
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit("gffx index failed: " + r.stderr.decode(errors="replace")[:300])
        if i:
            t.append(dt)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.repeats, 5)
    work = a.dir or tempfile.mkdtemp(prefix="index_bench_")
    out = []
    paths = {}
    for sub in ("host", "gpu"):
        os.makedirs(os.path.join(work, sub), exist_ok=True)
        paths[sub] = os.path.join(work, sub, "g.gff")
    n_lines = synth.write_gff3_fast(paths["host"], synth.gencode_like_roots(a.genes, seed=42))
    if os.path.exists(paths["gpu"]):
        os.remove(paths["gpu"])
    os.link(paths["host"], paths["gpu"])
    size = os.path.getsize(paths["host"])
    say(out, "gffx index on one MI355X host + device: %d genes, %d lines, %.1f MB; wall clock of the process, %d runs after a warm-up, median [min .. max]" %
        (a.genes, n_lines, size / 1e6, reps))
    for label, env in (("GFFX_LINE_TABLE=off (the eight side-cars alone)", {"GFFX_LINE_TABLE": "off"}), ("default (with .lsoa / .lall)", {})):
        h = wall(paths["host"], False, env, reps)
        g = wall(paths["gpu"], True, env, reps)
        say(out, "%s:" % label)
        say(out, "  gffx index        %.3f s [%.3f .. %.3f]" % h)
        say(out, "  gffx index --gpu  %.3f s [%.3f .. %.3f]   host / device = %.2f" % (g + (h[0] / g[0],)))
        same = all(open(paths["host"] + s, "rb").read() == open(paths["gpu"] + s, "rb").read() for s in SIDE_CARS)
        say(out, "  the eight side-cars of the two runs: %s" % ("identical" if same else "DIFFERENT"))
    text = open(paths["host"], "rb").read()
    stages = {k: [] for k in ("scan", "rows", "table", "resolve", "number")}
    t_all = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        g = engine.gff_index(text)
        dt = time.perf_counter() - t0
        ms, c = g.stage_ms, g.counts
        g.close()
        if i:
            t_all.append(dt)
            for k in stages:
                stages[k].append(ms[k])
    med = {k: statistics.median(v) for k, v in stages.items()}
    say(out, "device stages (HIP events, median of %d): line scan %.2f ms, rows kernels %.2f ms, ID table %.2f ms, resolve %.2f ms, numbering + root list %.2f ms" %
        (reps, med["scan"], med["rows"], med["table"], med["resolve"], med["number"]))
    say(out, "  feed + finish through the C-ABI (text already in memory, copies included): %.3f s median" % statistics.median(t_all))
    say(out, "  counts: %s" % ", ".join("%s %d" % kv for kv in c.items()))
    floor = size / HBM_BPS * 1e3
    say(out, "roofline: one read of the text at 8 TB/s = %.3f ms; line scan + rows kernels = %.2f ms = %.2f %% of that rate" %
        (floor, med["scan"] + med["rows"], 100 * floor / (med["scan"] + med["rows"])))
    if a.out:
        open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
