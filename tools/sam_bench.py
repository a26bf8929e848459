"""Measures the SAM source path against the BAM path on the same records: one synthetic coordinate-sorted file of 150-base
reads with realistic CIGARs (mostly 150M; insertions, deletions, soft clips, a spliced read now and then), written three ways --
BAM, BGZF-compressed SAM and plain SAM -- and read through engine.BamReader / engine.SamReader.  Per format: one warm-up read,
then --repeats timed reads; median and min..max of the device stages (the `_stage_ms` triples, HIP events) and of the wall
clock of feed + finish, rows per second, and GB/s of SAM text through the line scan and the rows pass.  The yardstick is the
BAM path's framing + rows on the same records, not a fixed number.  The row arrays of the three formats are compared too.
Prints a text table and one JSON line.  Usage: python tools/sam_bench.py [--reads 1000000] [--repeats 5] [--procs 16] [--dir DIR]"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CIGARS = [([(0, 150)], 0.80), ([(0, 100), (1, 1), (0, 49)], 0.05), ([(0, 60), (2, 2), (0, 90)], 0.05), ([(4, 20), (0, 130)], 0.05),
          ([(0, 75), (3, 1000), (0, 75)], 0.03), ([(0, 148), (4, 2)], 0.02)]
FLAGS = [0, 16, 99, 147, 4]
FLAG_P = [0.4, 0.4, 0.09, 0.09, 0.02]


def _member(data):
    from gffx_amd import synth
    return synth.bgzf_member(data, 1)


def make_records(n, names, lengths, seed):
    """(SAM lines, BAM records) of the same n reads, sorted by (reference, position)."""
    from gffx_amd import synth
    rng = np.random.default_rng(seed)
    per = np.diff(np.linspace(0, n, len(names) + 1).astype(np.int64))
    which = rng.choice(len(CIGARS), n, p=[p for _, p in CIGARS])
    flags = rng.choice(FLAGS, n, p=FLAG_P)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, 150))]
    quals = rng.integers(33 + 20, 33 + 41, (n, 150), dtype=np.uint8)
    packed = rng.choice(np.array([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88], np.uint8), (n, 75))
    cig_txt = [synth.sam_cigar(c) for c, _ in CIGARS]
    cig_bin = [b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in c) for c, _ in CIGARS]
    lines, recs, i = [], [], 0
    for t, k in enumerate(per):
        pos = np.sort(rng.integers(0, max(1, lengths[t] - 2000), k))
        rname = names[t].encode()
        for p in pos.tolist():
            w, flag = int(which[i]), int(flags[i])
            name = b"read.%014d" % i
            lines.append(b"%s\t%d\t%s\t%d\t60\t%s\t=\t%d\t300\t%s\t%s\tNM:i:1\n" % (name, flag, rname, p + 1, cig_txt[w], p + 151, bases[i].tobytes(),
                                                                                   quals[i].tobytes()))
            body = (struct.pack("<iiBBHHHiiii", t, p, len(name) + 1, 60, 4680, len(CIGARS[w][0]), flag, 150, t, p + 150, 300) + name + b"\x00" +
                    cig_bin[w] + packed[i].tobytes() + (quals[i] - 33).tobytes() + b"NMC\x01")
            recs.append(struct.pack("<i", len(body)) + body)
            i += 1
    return lines, recs


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--dir", default=None, help="scratch directory for the files (default: a temporary one, removed)")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="sam_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import synth
    refs = list(synth.GRCH38)[:24]
    names, lengths = [n for n, _ in refs], [ln for _, ln in refs]
    t = time.perf_counter()
    lines, recs = make_records(a.reads, names, lengths, seed=1)
    sam_header, bam_header = synth.sam_header(refs), synth.bam_header(refs)
    ctx = mp.get_context("fork")  # before anything opens the GPU in this process
    with ctx.Pool(a.procs) as pool:
        files = {"plain SAM": sam_header + b"".join(lines)}
        for name, header, items in (("BGZF SAM", sam_header, lines), ("BAM", bam_header, recs)):
            blocks = synth.bgzf_blocks(header, items, "aligned")
            files[name] = b"".join(pool.map(_member, blocks, chunksize=64)) + synth.BGZF_EOF
    text_bytes = len(files["plain SAM"])
    res = {"reads": a.reads, "repeats": a.repeats, "sam_text_bytes": text_bytes, "bam_record_bytes": sum(len(r) for r in recs),
           "file_bytes": {k: len(v) for k, v in files.items()}, "write_s": round(time.perf_counter() - t, 1)}
    del lines, recs

    from gffx_amd import engine
    if engine.device_count() < 1:
        raise SystemExit("sam_bench needs an MI355X: no HIP device visible (nothing is measured on the CPU)")
    engine.warmup(0)
    ref_seq = list(range(len(names)))

    def reader(fmt):
        if fmt == "BAM":
            return engine.BamReader(ref_seq, len(bam_header), 0)
        return engine.SamReader(names, ref_seq, len(sam_header), 0, bgzf=fmt == "BGZF SAM")

    rows = {}
    for fmt in ("BAM", "BGZF SAM", "plain SAM"):
        data = files[fmt]
        stages, walls = [], []
        for rep in range(a.repeats + 1):  # the first read is the warm-up
            t = time.perf_counter()
            r = reader(fmt)
            r.feed(data)
            r.finish()
            wall = (time.perf_counter() - t) * 1e3
            ms, c = r.stage_ms(), r.counts()
            if rep == 0:
                rows[fmt] = r.rows()
            r.close()
            if rep:
                stages.append(ms)
                walls.append(wall)
        keys = list(stages[0])
        out = {k + "_ms": spread([s[k] for s in stages]) for k in keys}
        out["wall_ms"] = spread(walls)
        out["kept"] = c["kept"]
        second, third = keys[1], keys[2]  # BAM: frame, rows; SAM: lines, rows
        after_inflate = [s[second] + s[third] for s in stages]
        out["after_inflate_ms"] = spread(after_inflate)
        out["rows_per_s_after_inflate"] = round(a.reads / statistics.median(after_inflate) * 1e3)
        if fmt != "BAM":
            out["text_GBps_line_scan"] = round(text_bytes / statistics.median([s["lines"] for s in stages]) / 1e6, 2)
            out["text_GBps_rows"] = round(text_bytes / statistics.median([s["rows"] for s in stages]) / 1e6, 2)
        res[fmt] = out
    res["rows_equal"] = bool(np.array_equal(rows["BAM"], rows["BGZF SAM"]) and np.array_equal(rows["BAM"], rows["plain SAM"]))
    print("SAM source path, %d reads of 150 bases, %d timed reads per format after one warm-up (median [min .. max], ms)" % (a.reads, a.repeats))
    print("SAM text %.1f MB, BAM records %.1f MB; files: %s" % (text_bytes / 1e6, res["bam_record_bytes"] / 1e6,
                                                               ", ".join("%s %.1f MB" % (k, v / 1e6) for k, v in res["file_bytes"].items())))
    for fmt in ("BAM", "BGZF SAM", "plain SAM"):
        o = res[fmt]
        print("%-10s %s" % (fmt, "  ".join("%s %.3f [%.3f .. %.3f]" % (k, v["median"], v["min"], v["max"]) for k, v in o.items() if isinstance(v, dict))))
        print("%-10s %s" % ("", "  ".join("%s %s" % (k, v) for k, v in o.items() if not isinstance(v, dict))))
    print("rows of the three formats equal: %s" % res["rows_equal"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
