"""Measures the device BED reader against the host parsers on one synthetic BED file (synth.write_bed_fast; --rows, default
10 M) and its bgzipped twin.
  1. The three device stages (inflate, line scan, rows: the `_stage_ms` triple, HIP events) and the wall clock of feed + finish
     through engine.BedReader, per dialect, for the plain text and for the BGZF file: one warm-up read, then --repeats timed.
  2. The wall clock of the CLI, `gffx intersect -e` and `gffx depth`, with -t 16, for (a) the host parser on the plain file,
     (b) GFFX_BED_DEVICE=1 on the plain file, (c) the .bed.gz file: one warm-up run, then the median of --repeats runs; the
     outputs of the three are compared byte for byte.
No threshold: the numbers say which of (a) and (b) is faster on plain text here; (c) has no host rival.
Prints a text table and one JSON line.  Usage: python tools/bed_device_bench.py [--rows 10000000] [--repeats 5] [--dir DIR]"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


def _member(data):
    from gffx_amd import synth
    return synth.bgzf_member(data, 6)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--dir", default=None, help="scratch directory for the files (default: a temporary one, removed)")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="bed_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import synth
    t = time.perf_counter()
    roots = synth.gencode_like_roots(63000, seed=42)
    names = list(roots["names"])
    gff, bed = os.path.join(a.dir, "g.gff"), os.path.join(a.dir, "q.bed")
    synth.write_gff3_fast(gff, roots)
    subprocess.check_call([GFFX, "index", "-i", gff], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    synth.write_bed_fast(bed, synth.synth_bed(a.rows, seed=43, roots=roots), names)
    text = open(bed, "rb").read()
    ctx = mp.get_context("fork")  # before anything opens the GPU in this process
    with ctx.Pool(a.procs) as pool:
        gz = b"".join(pool.map(_member, [text[i:i + synth.BGZF_BLOCK] for i in range(0, len(text), synth.BGZF_BLOCK)], chunksize=64))
    gz += synth.BGZF_EOF
    open(bed + ".gz", "wb").write(gz)
    res = {"rows": a.rows, "repeats": a.repeats, "threads": a.threads, "text_bytes": len(text), "bgzf_bytes": len(gz),
           "write_s": round(time.perf_counter() - t, 1)}

    from gffx_amd import engine
    if engine.device_count() < 1:
        raise SystemExit("bed_device_bench needs an MI355X: no HIP device visible (nothing is measured on the CPU)")
    engine.warmup(0)
    kept = {}
    for dialect, dname in ((engine.BED_INTERSECT, "intersect"), (engine.BED_DEPTH, "depth")):
        for form, data in (("plain", text), ("bgzf", gz)):
            stages, walls = [], []
            for rep in range(a.repeats + 1):  # the first read is the warm-up
                t = time.perf_counter()
                r = engine.BedReader(names, dialect, 0, bgzf=form == "bgzf")
                r.feed(data)
                r.finish()
                wall = (time.perf_counter() - t) * 1e3
                ms, c = r.stage_ms(), r.counts()
                if rep == 0:
                    kept[(dname, form)] = r.rows()
                r.close()
                if rep:
                    stages.append(ms)
                    walls.append(wall)
            out = {k + "_ms": spread([s[k] for s in stages]) for k in ("inflate", "lines", "rows")}
            out["wall_ms"] = spread(walls)
            out["kept"] = c["kept"]
            out["text_GBps_line_scan"] = round(len(text) / statistics.median([s["lines"] for s in stages]) / 1e6, 2)
            out["text_GBps_rows"] = round(len(text) / statistics.median([s["rows"] for s in stages]) / 1e6, 2)
            res["device %s %s" % (dname, form)] = out
        res["rows_equal_" + dname] = bool(np.array_equal(kept[(dname, "plain")], kept[(dname, "bgzf")]))
    del kept

    env0 = {k: v for k, v in os.environ.items() if k not in ("GFFX_BED_DEVICE", "GFFX_BED_CHUNK_BYTES")}
    routes = (("a host parser, plain", bed, {}), ("b GFFX_BED_DEVICE=1, plain", bed, {"GFFX_BED_DEVICE": "1"}), ("c .bed.gz", bed + ".gz", {}))
    for cmd, flags in (("intersect", ["-e", "-b"]), ("depth", ["-s"])):
        outs = []
        for label, path, knob in routes:
            out = os.path.join(a.dir, "out_%s_%s" % (cmd, label[0]))
            walls = []
            for rep in range(a.repeats + 1):
                t = time.perf_counter()
                subprocess.check_call([GFFX, cmd, "-i", gff, "-t", str(a.threads), "-o", out] + flags + [path], env=dict(env0, **knob),
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                if rep:
                    walls.append((time.perf_counter() - t) * 1e3)
            res["cli %s, %s" % (cmd, label)] = {"wall_ms": spread(walls)}
            outs.append(open(out, "rb").read())
        res["cli %s outputs equal" % cmd] = bool(outs[0] == outs[1] == outs[2] and len(outs[0]) > 0)

    print("BED on the device, %d rows: text %.1f MB, bgzipped %.1f MB; %d timed runs after one warm-up (median [min .. max], ms)"
          % (a.rows, len(text) / 1e6, len(gz) / 1e6, a.repeats))
    for k, o in res.items():
        if isinstance(o, dict):
            print("%-38s %s" % (k, "  ".join("%s %.3f [%.3f .. %.3f]" % (n, v["median"], v["min"], v["max"]) for n, v in o.items() if isinstance(v, dict))))
            rest = "  ".join("%s %s" % (n, v) for n, v in o.items() if not isinstance(v, dict))
            if rest:
                print("%-38s %s" % ("", rest))
        elif k.startswith(("rows_equal", "cli ")):
            print("%s: %s" % (k, o))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
