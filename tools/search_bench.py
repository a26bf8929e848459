"""Measures `gffx search` on the GENCODE-shaped synthetic GFF3 that bench.py writes (synth.write_gff3_fast around
gencode_like_roots(63000, seed=42): ~3.4 M lines), indexed once with `-a gene_name` and once with `-a ID`, with lists of 1, 1 K
and 100 K exact values and of 1, 100 and 1 K regexes drawn by seed from the index's own `.atn` values.

Protocol (DESIGN.md sections 14 and 15).  Device stages are HIP-event times (engine.AttrSearch.stage_ms): one warm-up, then
--repeats timed runs; median and min .. max.  Per stage the bytes its ALGORITHM needs (not what the kernel moved), over the
median time, as a share of 8 TB/s:
    match     value bytes + 8 B per value (its offset), once per pattern group
    resolve   4 B per `.a2f` word
CLI wall clock (index built before, page cache warm, best of two) for `-e` and for the filtered output.  Host compile of a regex
list is timed on its own.  Host yardstick: step 1 of the reference on ONE core in tools/search_host_baseline.cpp (a hash set for
exact; this project's own DFA per pattern, every value against every pattern, for regex) -- a RESTATEMENT of the reference
algorithm, NOT the Rust binary, which cannot be built here.  Where the regex yardstick would run for minutes it takes the first
--baseline-values values and the time is scaled linearly to the table (marked "scaled").
Nothing here is a pass/fail number.  Not measured: the Rust binary, more than one GPU, HBM counters.
Usage: python tools/search_bench.py [--genes 63000] [--repeats 5] [--dir DIR] [--out profiles/search.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gffx_amd import engine, synth  # noqa: E402

GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
BASELINE = os.path.join(ROOT, "gffx_amd", "bin", "search_host_baseline")
HBM_BPS = 8e12
META = set("\\.+*?()|[]{}^$-")


def esc(s):
    return "".join("\\" + c if c in META else c for c in s)


def host_baseline(atn, lst, mode, limit):
    if not os.path.exists(BASELINE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "search_host_baseline"], stdout=subprocess.DEVNULL)
    cmd = ["taskset", "-c", "0", BASELINE, atn, lst, mode] + ([str(limit)] if limit else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout)


def cli_wall(gff, lst, regex, entire_group):
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        r = subprocess.run([GFFX, "search", "-i", gff, "-A", lst, "-o", os.devnull] + (["-r"] if regex else []) + (["-e"] if entire_group else []),
                           capture_output=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            return "failed: " + r.stderr.decode(errors="replace").strip()[:80]
        best = dt if best is None else min(best, dt)
    return "%.2f s" % best


def timed(a, key, fn, reps):
    fn()  # warm-up
    ms = []
    for _ in range(reps):
        a.reset()
        before = a.stage_ms()[key]
        fn()
        ms.append(a.stage_ms()[key] - before)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-values", type=int, default=100_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix="search_bench_")
    os.makedirs(work, exist_ok=True)
    out = ["gffx search on one MI355X: HIP-event ms = median of %d after a warm-up (min .. max); share = algorithmic bytes / time / 8 TB/s;" % a.repeats,
           "host yardstick = the reference's step 1 RESTATED on one core (tools/search_host_baseline.cpp), not the Rust binary; CLI = wall clock, best of two"]
    gff0 = os.path.join(work, "g.gff")
    n_lines = synth.write_gff3_fast(gff0, synth.gencode_like_roots(a.genes, seed=42))
    out.append("GFF3: %d genes, %d lines, %.0f MB" % (a.genes, n_lines, os.path.getsize(gff0) / 1e6))
    rng = np.random.Generator(np.random.PCG64(5))
    for attr in ("gene_name", "ID"):
        gff = os.path.join(work, attr + ".gff")
        if os.path.exists(gff):
            os.remove(gff)
        os.link(gff0, gff)
        t0 = time.perf_counter()
        subprocess.check_call([GFFX, "index", "-i", gff, "-a", attr])
        t_index = time.perf_counter() - t0
        values = [ln.strip() for ln in open(gff + ".atn", "rb").read().decode().split("\n")]
        values = [v for v in values if v and not v.startswith("#")]
        a2f = np.fromfile(gff + ".a2f", dtype="<u4")
        prt = np.fromfile(gff + ".prt", dtype="<u4")
        n = len(values)
        nbytes = sum(len(v.encode()) for v in values) + 8 * (n + 1)
        h = engine.AttrSearch.from_arrays(values, a2f, prt, key=attr)
        out.append("")
        out.append("index -a %s (%.1f s): %d values, %.1f MB with offsets, %d fids; value table + classes on the device %.3f ms" %
                   (attr, t_index, n, nbytes / 1e6, len(a2f), h.stage_ms()["build"]))
        for regex, sizes in ((False, (1, 1000, 100_000)), (True, (1, 100, 1000))):
            for k in sizes:
                picks = [values[i] for i in rng.integers(0, n, size=k).tolist()]
                pats = ["^" + esc(p[:-1]) + "[0-9a-z]$" for p in picks] if regex else picks
                lst = os.path.join(work, "%s_%s_%d.txt" % (attr, "re" if regex else "ex", k))
                open(lst, "w").write("".join(p + "\n" for p in pats))
                if regex:
                    t0 = time.perf_counter()
                    c = engine.compile_regex(pats)
                    t_comp = time.perf_counter() - t0
                    med, lo, hi = timed(h, "match", lambda: h.match_regex(c), a.repeats)
                    groups = len(c.groups)
                    what = "k_attr_match_dfa, %d group(s), host compile %.2f s" % (groups, t_comp)
                else:
                    med, lo, hi = timed(h, "match", lambda: h.match(pats), a.repeats)
                    groups = 1
                    what = "k_table_insert + k_attr_match_exact"
                limit = a.baseline_values if regex and k * n > 2e8 else 0
                b = host_baseline(gff + ".atn", lst, "regex" if regex else "exact", limit)
                scale = b["values"] / max(b["values_used"], 1)
                base = "host 1 core: match %.1f ms%s + build/compile %.1f ms" % (b["match_ms"] * scale, " (scaled from %d values)" % b["values_used"] if limit else "",
                                                                                   b["compile_ms"])
                out.append("  %s %6d: %s %.3f ms (%.3f .. %.3f), %.1f %% of peak | %s | CLI -e %s, filtered %s" %
                           ("regex" if regex else "exact", k, what, med, lo, hi, 100 * nbytes * groups / (med / 1e3) / HBM_BPS, base,
                            cli_wall(gff, lst, regex, True), cli_wall(gff, lst, regex, False)))
        h.reset()
        h.match([values[i] for i in rng.integers(0, n, size=1000).tolist()])
        ms = []
        for _ in range(a.repeats + 1):
            before = h.stage_ms()["resolve"]
            h.resolve()
            ms.append(h.stage_ms()["resolve"] - before)
        ms = ms[1:]
        out.append("  resolve, 1000 wanted: k_attr_resolve %.3f ms (%.3f .. %.3f), %.1f %% of peak" %
                   (statistics.median(ms), min(ms), max(ms), 100 * 4 * len(a2f) / (statistics.median(ms) / 1e3) / HBM_BPS))
        h.close()
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
