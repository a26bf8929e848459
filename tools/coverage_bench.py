"""Measures `gffx coverage` at scale: writes a seeded BED of N rows (width U[100, 10 000] over GRCh38-shaped chromosomes) and a
GENCODE-shaped GFF with its index, runs `gffx coverage -v --stats-json` on them and prints the stage timers, the union's
HIP-event kernel time and its fraction of the HBM roofline (algorithmic bytes: 12 per row in + 16 per span out) as one JSON
object.  The files are kept in --dir between runs (the name carries N and the seed), so another build of the binary can be
timed on the same input with --gffx.  --mean-depth times the run with that flag (the pileup's stage times are in `counts`),
--thresholds T1,T2,... and --bedgraph the run with those (the depth profile's stage times are in `counts` as profile_*);
`wall_runs_s` lists every run, so a median of five after a warm-up is --runs 6 without its first entry.
Usage: python tools/coverage_bench.py [--rows 20000000] [--gpus 1] [--genes 63000] [--seed 5] [--dir DIR] [--gffx PATH] [--runs 2]
                                      [--threads N] [--mean-depth] [--thresholds 1,10,30] [--bedgraph]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def write_bed(path, n, seed, names, synth):
    """N rows in pieces of 25 M (the generator's arrays stay small), appended to one file."""
    piece = 25_000_000
    with open(path, "wb") as out:
        for k, a in enumerate(range(0, n, piece)):
            regions = synth.synth_bed(min(piece, n - a), seed=seed + 1000 * k)
            tmp = path + ".part"
            synth.write_bed_fast(tmp, regions, names)
            with open(tmp, "rb") as f:
                while True:
                    buf = f.read(1 << 26)
                    if not buf:
                        break
                    out.write(buf)
            os.remove(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory for the files (default: a temporary one, removed)")
    ap.add_argument("--gffx", default=os.path.join(ROOT, "gffx_amd", "bin", "gffx"), help="the binary to time")
    ap.add_argument("--runs", type=int, default=2, help="timed runs; the last one is reported (the first warms the page cache)")
    ap.add_argument("--threads", type=int, default=0, help="-t of the command (default: the command's own)")
    ap.add_argument("--mean-depth", action="store_true", help="run with --mean-depth")
    ap.add_argument("--thresholds", default=None, help="run with --thresholds LIST")
    ap.add_argument("--bedgraph", action="store_true", help="run with --bedgraph (the file goes beside the output)")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="coverage_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import synth
    roots = synth.gencode_like_roots(a.genes, seed=a.seed)
    gff = os.path.join(a.dir, "genes_%d_%d.gff" % (a.genes, a.seed))
    if not os.path.exists(gff + ".gof"):
        synth.write_gff3_fast(gff, roots, seed=a.seed)
        subprocess.check_call([os.path.join(ROOT, "gffx_amd", "bin", "gffx"), "index", "-i", gff])
    bed = os.path.join(a.dir, "rows_%d_%d.bed" % (a.rows, a.seed))
    if not os.path.exists(bed):
        write_bed(bed, a.rows, a.seed + 1, roots["names"], synth)
    out, stats = os.path.join(a.dir, "coverage.tsv"), os.path.join(a.dir, "stats.json")
    cmd = [a.gffx, "coverage", "-v", "-i", gff, "-s", bed, "-o", out, "--stats-json", stats]
    if a.gpus != 1:
        cmd += ["--gpus", str(a.gpus)]
    if a.threads:
        cmd += ["-t", str(a.threads)]
    if a.mean_depth:
        cmd += ["--mean-depth"]
    if a.thresholds:
        cmd += ["--thresholds", a.thresholds]
    if a.bedgraph:
        cmd += ["--bedgraph", os.path.join(a.dir, "coverage.bedgraph")]
    wall, walls = 0.0, []
    for _ in range(max(1, a.runs)):
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True)
        wall = time.time() - t0
        walls.append(round(wall, 3))
        if r.returncode != 0:
            sys.stderr.write(r.stderr.decode(errors="replace"))
            sys.exit(r.returncode)
    st = json.load(open(stats))
    res = {"rows": a.rows, "gpus": a.gpus, "bed_bytes": os.path.getsize(bed), "wall_s": round(wall, 3), "wall_runs_s": walls,
           "total_ms": st["total_ms"], "stages_ms": st["stages_ms"], "counts": st.get("counts", {}),
           "output_rows": sum(1 for _ in open(out, "rb")) - 1}
    if a.bedgraph:
        res["bedgraph_bytes"] = os.path.getsize(os.path.join(a.dir, "coverage.bedgraph"))
    c = res["counts"]
    if c.get("union_kernels_ms"):
        algo = 12.0 * c["rows"] + 16.0 * c["union_spans"]
        res["union_algorithmic_bytes"] = algo
        res["union_fraction_of_hbm_roofline"] = round(algo / (c["union_kernels_ms"] * 1e-3) / HBM_BYTES_PER_S, 5)
    for name, ms in res["stages_ms"]:
        sys.stderr.write("%10.3f ms  %s\n" % (ms, name))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
