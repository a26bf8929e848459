"""Measures `gffx seq` at scale: a GENCODE-shaped GFF3 (synth.write_gff3_fast: gene, mRNA, exon and CDS lines) over chromosomes
shaped like GRCh38 divided by --genome-div, and a random genome for the same seqids in lines of 60 (synth.write_fasta_fast).

Per mode (`-T exon -j`, `-T CDS -j --translate`, `-T gene`), one warm-up run and --reps timed runs of the command with
--stats-json, the median [min .. max] of
  the kernels' HIP-event times   pack (FASTA line kernels + classify / prefix sums / copy), plan (sort, lengths, body sizes and
                                 their prefix sums), emit (k_seq_emit over all slices)
  the emit beside the roofline   its algorithmic bytes -- bases read (three per character with --translate) plus body bytes
                                 written -- over the emit time, against 8 TB/s
  the wall clock                 of the whole command
and beside them one host core: bin/seq_host_baseline (`make seq_host_baseline`: tools/seq_check.cpp --run without the
sanitizers, the same rules through device/seq_core.hpp), its FASTA parse, its records stage (grouping, gathering, complementing,
translating, wrapping: what plan + emit do) and its wall clock; its output must be the command's, byte for byte.
One JSON object on stdout.  The files are kept in --dir between runs.
Usage: python tools/seq_bench.py [--genes 63000] [--genome-div 8] [--seed 5] [--reps 5] [--dir DIR] [--skip-host]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"exon_join": (["-T", "exon", "-j"], ("exon", 1, 0)), "cds_join_translate": (["-T", "CDS", "-j", "--translate"], ("CDS", 1, 1)),
         "gene": (["-T", "gene"], ("gene", 0, 0))}
HBM_BYTES_PER_S = 8e12


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--genome-div", type=int, default=8, help="GRCh38's chromosome lengths are divided by this")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory for the files (default: a temporary one, removed)")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="seq_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import synth
    gffx = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
    chroms = [(n, max(l // a.genome_div, 1000)) for n, l in synth.GRCH38]
    roots = synth.gencode_like_roots(a.genes, seed=a.seed, chroms=chroms)
    gff = os.path.join(a.dir, "genes_%d_%d_%d.gff" % (a.genes, a.genome_div, a.seed))
    if not os.path.exists(gff + ".gof"):
        synth.write_gff3_fast(gff, roots, seed=a.seed)
        subprocess.check_call([gffx, "index", "-i", gff])
    fa = os.path.join(a.dir, "genome_%d_%d.fa" % (a.genome_div, a.seed))
    if not os.path.exists(fa):
        synth.write_fasta_fast(fa, chroms, 60, a.seed)
    res = {"genes": a.genes, "genome_bases": sum(l for _, l in chroms), "fasta_bytes": os.path.getsize(fa), "gff_bytes": os.path.getsize(gff), "reps": a.reps,
           "modes": {}}
    out, stats = os.path.join(a.dir, "out.fa"), os.path.join(a.dir, "stats.json")
    tool = os.path.join(ROOT, "gffx_amd", "bin", "seq_host_baseline")
    if not a.skip_host:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "seq_host_baseline"], stdout=subprocess.DEVNULL)
    for name, (flags, host_args) in MODES.items():
        runs = []
        for k in range(a.reps + 1):  # (the first one warms the page cache and the device up)
            t0 = time.time()
            r = subprocess.run([gffx, "seq", "-i", gff, "-f", fa, "-o", out, "--stats-json", stats] + flags, capture_output=True)
            wall = time.time() - t0
            if r.returncode != 0:
                sys.stderr.write(r.stderr.decode(errors="replace"))
                sys.exit(r.returncode)
            s = json.load(open(stats))
            flat = dict(s.get("counts", s))
            flat["wall_s"] = wall
            if k:
                runs.append(flat)
        first = runs[0]
        body = float(first["body_bytes"])
        algo = body * (4 if "--translate" in flags else 2)  # (bases read + bytes written: the newlines are ~1/61 of the body)
        emit = [x["emit_kernels_ms"] for x in runs]
        m = {"features": first["features"], "records_written": first["records_written"], "body_bytes": body, "output_bytes": os.path.getsize(out),
             "pack_ms": spread([x["line_kernels_ms"] + x["pack_kernels_ms"] for x in runs]), "plan_ms": spread([x["plan_kernels_ms"] for x in runs]),
             "emit_ms": spread(emit), "write_ms": spread([x["write_ms"] for x in runs]), "wall_s": spread([x["wall_s"] for x in runs]),
             "emit_algorithmic_bytes": algo, "emit_gb_per_s": round(algo / (statistics.median(emit) * 1e-3) / 1e9, 1),
             "emit_share_of_8_tb_per_s": round(algo / (statistics.median(emit) * 1e-3) / HBM_BYTES_PER_S, 4)}
        if not a.skip_host:
            host_out = os.path.join(a.dir, "host.fa")
            takes = []
            for _ in range(3):
                t0 = time.time()
                r = subprocess.run([tool, "--run", gff, fa, host_args[0], str(host_args[1]), str(host_args[2]), "60", host_out], capture_output=True, check=True)
                t = dict(zip(r.stderr.split()[0::2], (float(x) for x in r.stderr.split()[1::2])))
                takes.append({"fasta_ms": t[b"fasta_ms"], "records_ms": t[b"records_ms"], "total_ms": t[b"total_ms"], "wall_s": time.time() - t0})
            m["one_host_core"] = {k: spread([x[k] for x in takes]) for k in takes[0]}
            m["one_host_core"]["same_bytes"] = subprocess.run(["cmp", "-s", out, host_out]).returncode == 0
            os.remove(host_out)
        res["modes"][name] = m
        sys.stderr.write("%s: %s\n" % (name, json.dumps(m)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
