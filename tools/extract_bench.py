"""Measures `gffx extract` on the GENCODE-shaped synthetic GFF3 that bench.py writes (synth.write_gff3_fast around
gencode_like_roots(63000, seed=42): ~3.4 M lines), with ID lists of 1 K, 100 K and 1 M names drawn by seed from the file's IDs.

Protocol.  Device stages are HIP-event times (engine.FeatureIds.stage_ms): one warm-up, then --repeats timed runs; median and
min .. max.  Per stage the bytes its ALGORITHM needs (not what the kernel moved), over the median time, as a share of 8 TB/s:
    table build   name bytes + 12 B per entry (one 8-byte slot word + one 4-byte value)
    resolve       query bytes + 8 B per name (fid + root out)
    line filter   chunk bytes + 9 B per line (line offset in + one keep byte out), summed over the chunks of <= 64 MiB
CLI wall clock (index built before, page cache warm, best of two) for `-e` and for the per-feature mode.  Host yardstick: the
same steps on ONE core in tools/extract_host_baseline.cpp (std::unordered_map build and lookup, array chase, memchr / memmem
filter) -- a restatement of the reference algorithm, NOT the Rust binary, which cannot be built here.
Nothing here is a pass/fail number.  Prints a text table (kept as profiles/extract.txt) and one JSON line.
Usage: python tools/extract_bench.py [--genes 63000] [--repeats 5] [--sizes 1000 100000 1000000] [--dir DIR]"""
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
CHUNK = 64 << 20


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_BPS * 100, 3) if ms > 0 else None


def host_baseline(gff, lst):
    exe = os.path.join(ROOT, "gffx_amd", "bin", "extract_host_baseline")
    src = os.path.join(ROOT, "tools", "extract_host_baseline.cpp")
    if not os.path.exists(exe) or os.path.getmtime(src) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])
    return json.loads(subprocess.run(["taskset", "-c", "0", exe, gff, lst], check=True, capture_output=True, text=True).stdout)


def hit_chunks(data, gof, roots):
    """the lines of the hit blocks as the CLI's text pass cuts them: (text, line_off, line_root) per chunk of <= 64 MiB"""
    rec = np.frombuffer(gof, dtype=np.dtype([("fid", "<u4"), ("seq", "<u4"), ("s", "<u8"), ("e", "<u8")]))
    block = {int(r["fid"]): (int(r["s"]), int(r["e"])) for r in rec}
    ranges = sorted((block[r][0], min(block[r][1], len(data)), r) for r in roots.tolist() if r in block)
    buf = np.frombuffer(data, np.uint8)
    texts, lens, lroots = [], [], []
    for s, e, r in ranges:
        if s >= e:
            continue
        nl = np.flatnonzero(buf[s:e] == 10) + 1
        ends = nl if len(nl) and nl[-1] == e - s else np.append(nl, e - s)
        texts.append(data[s:e])
        lens.append(np.diff(np.concatenate([[0], ends])))
        lroots.append(np.full(len(ends), r, np.uint32))
    if not texts:
        return []
    lens, lroots, text = np.concatenate(lens), np.concatenate(lroots), b"".join(texts)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    chunks, i = [], 0
    while i < len(lens):
        j = int(np.searchsorted(off, off[i] + CHUNK, side="right")) - 1
        j = max(j, i + 1)
        chunks.append((text[int(off[i]):int(off[j])], (off[i:j + 1] - off[i]).astype(np.uint64), lroots[i:j]))
        i = j
    return chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 100_000, 1_000_000])
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one, removed)")
    a = ap.parse_args()
    assert a.repeats >= 5, "the protocol asks for at least 5 timed runs"
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="extract_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import engine, synth
    if engine.device_count() < 1:
        raise SystemExit("extract_bench needs an MI355X: no HIP device visible (nothing is measured on the CPU)")
    synth.build_synth_text()
    gff = os.path.join(a.dir, "anno.gff")
    n_lines = synth.write_gff3_fast(gff, synth.gencode_like_roots(a.genes, seed=42))
    t = time.perf_counter()
    subprocess.run([GFFX, "index", "-i", gff], check=True, capture_output=True)
    res = {"gff_lines": n_lines, "gff_MB": round(os.path.getsize(gff) / 1e6, 1), "index_s": round(time.perf_counter() - t, 2), "repeats": a.repeats}
    data = open(gff, "rb").read()
    gof = open(gff + ".gof", "rb").read()
    names = [ln for ln in open(gff + ".fts", "rb").read().split(b"\n") if ln]
    prt = np.frombuffer(open(gff + ".prt", "rb").read(), "<u4")
    uniq = list(dict.fromkeys(names))
    name_bytes = sum(len(n) for n in names)
    res["table_names"], res["name_bytes"] = len(names), name_bytes
    engine.warmup(0)

    builds = []
    for rep in range(a.repeats + 1):
        ids = engine.FeatureIds.from_arrays(names, prt)
        if rep:
            builds.append(ids.stage_ms()["build"])
        if rep < a.repeats:
            ids.close()
    res["build_ms"] = spread(builds)
    res["build_algorithm_bytes"] = name_bytes + 12 * len(names)
    res["build_share_of_8TBps_pct"] = share(res["build_algorithm_bytes"], res["build_ms"]["median"])

    rng = np.random.Generator(np.random.PCG64(17))
    res["lists"] = {}
    for size in a.sizes:
        k = min(size, len(uniq))
        picked = [uniq[i] for i in rng.choice(len(uniq), size=k, replace=False).tolist()]
        lst = os.path.join(a.dir, "names_%d.txt" % size)
        open(lst, "wb").write(b"".join(p + b"\n" for p in picked))
        q_bytes = sum(len(p) for p in picked)
        out = {"names": k, "query_bytes": q_bytes}
        times = []
        for rep in range(a.repeats + 1):
            ids.reset()
            before = ids.stage_ms()["resolve"]
            ids.resolve(picked)
            if rep:
                times.append(ids.stage_ms()["resolve"] - before)
        out["resolve_ms"] = spread(times)
        out["resolve_algorithm_bytes"] = q_bytes + 8 * k
        out["resolve_share_of_8TBps_pct"] = share(out["resolve_algorithm_bytes"], out["resolve_ms"]["median"])
        chunks = hit_chunks(data, gof, ids.unique_roots())
        n_l, n_b = sum(len(c[2]) for c in chunks), sum(len(c[0]) for c in chunks)
        times, kept = [], 0
        for rep in range(a.repeats + 1):
            before = ids.stage_ms()["filter"]
            kept = sum(int(ids.filter_lines(*c).sum()) for c in chunks)
            if rep:
                times.append(ids.stage_ms()["filter"] - before)
        out.update(filter_lines=n_l, filter_bytes=n_b, filter_chunks=len(chunks), kept_lines=kept, filter_ms=spread(times))
        out["filter_algorithm_bytes"] = n_b + 9 * n_l
        out["filter_share_of_8TBps_pct"] = share(out["filter_algorithm_bytes"], out["filter_ms"]["median"])
        for label, extra in (("cli_entire_group_s", ["-e"]), ("cli_per_feature_s", [])):
            best = None
            for _ in range(2):
                t = time.perf_counter()
                subprocess.run([GFFX, "extract", "-i", gff, "-F", lst, "-o", os.path.join(a.dir, "out.gff")] + extra, check=True, capture_output=True)
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
            out[label] = round(best, 3)
        out["host_one_core"] = host_baseline(gff, lst)
        assert out["host_one_core"]["kept_lines"] == kept, "the host restatement and the device keep different lines"
        res["lists"][str(size)] = out
    ids.close()

    print("gffx extract on %d GFF lines (%.1f MB), %d table names; %d timed runs after one warm-up, median [min .. max]"
          % (n_lines, res["gff_MB"], len(names), a.repeats))
    b = res["build_ms"]
    print("table build (k_table_fill + k_table_insert)  %.3f ms [%.3f .. %.3f]   algorithm bytes %.1f MB = %s %% of 8 TB/s"
          % (b["median"], b["min"], b["max"], res["build_algorithm_bytes"] / 1e6, res["build_share_of_8TBps_pct"]))
    for size, o in res["lists"].items():
        r, f, h = o["resolve_ms"], o["filter_ms"], o["host_one_core"]
        print("list of %s names:" % size)
        print("  resolve (k_ids_resolve)       %.3f ms [%.3f .. %.3f]   algorithm bytes %.2f MB = %s %% of 8 TB/s"
              % (r["median"], r["min"], r["max"], o["resolve_algorithm_bytes"] / 1e6, o["resolve_share_of_8TBps_pct"]))
        print("  line filter (k_ids_filter)    %.3f ms [%.3f .. %.3f]   %d lines, %.1f MB in %d chunks, %d kept; algorithm bytes = %s %% of 8 TB/s"
              % (f["median"], f["min"], f["max"], o["filter_lines"], o["filter_bytes"] / 1e6, o["filter_chunks"], o["kept_lines"],
                 o["filter_share_of_8TBps_pct"]))
        print("  CLI wall clock                -e %.3f s   per-feature %.3f s" % (o["cli_entire_group_s"], o["cli_per_feature_s"]))
        print("  one host core (restatement of the reference algorithm, not the Rust binary): map build %.1f ms, lookup %.1f ms, "
              "chase %.1f ms, memmem filter %.1f ms" % (h["map_build_ms"], h["map_lookup_ms"], h["chase_ms"], h["filter_ms"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
