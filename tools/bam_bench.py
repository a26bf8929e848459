"""Measures the BAM source path: a synthetic coordinate-sorted BAM of 150-bp reads written with Python's zlib in two block
layouts -- aligned (samtools / htslib: a block is flushed before a record that would not fit) and spanning (htsjdk: records
cross block boundaries, so framing takes the serial fix-up) -- then
  * device inflate GB/s (decompressed bytes / k_bgzf_inflate time, HIP events), framing and rows M records/s per layout;
  * a CPU baseline: the same members inflated by zlib in N worker processes (no torch, no GPU in the workers);
  * `gffx depth -s x.bam` wall time against `-s x.bed` holding the same rows.
Prints one JSON object.  Usage: python tools/bam_bench.py [--reads 20000000] [--procs 16] [--dir DIR]"""
import argparse
import json
import mmap
import multiprocessing as mp
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK = 0xFF00
REC = 4 + 32 + 20 + 4 + 75 + 150  # block_size, fixed fields, read name (19 + NUL), 150M, 75 B of packed bases, 150 qualities


def _records(first, n, tid, pos, rng):
    """n fixed-size records of reads first .. first + n - 1 (150M) as one uint8 array."""
    r = np.zeros((n, REC), np.uint8)
    head = np.zeros(n, dtype=[("bs", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                              ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"), ("ntid", "<i4"), ("npos", "<i4"), ("tlen", "<i4")])
    head["bs"], head["tid"], head["pos"], head["lrn"], head["mapq"] = REC - 4, tid, pos, 20, 60
    head["ncig"], head["lseq"], head["ntid"], head["npos"] = 1, 150, -1, -1
    r[:, :36] = head.view(np.uint8).reshape(n, 36)
    names = np.char.encode(np.char.add("read.", np.char.zfill((np.arange(first, first + n)).astype(str), 14)), "ascii")
    r[:, 36:55] = np.frombuffer(names.tobytes(), np.uint8).reshape(n, 19)
    r[:, 56:60] = np.frombuffer(np.uint32(150 << 4).tobytes(), np.uint8)
    r[:, 60:135] = rng.choice(np.array([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88],
                                       np.uint8), size=(n, 75))
    r[:, 135:] = rng.integers(25, 41, size=(n, 150), dtype=np.uint8)
    return r


def _member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, 0)
    body = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (18 + len(body) + 8 - 1).to_bytes(2, "little") + body +
            (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + len(data).to_bytes(4, "little"))


def _compress(blocks):
    return b"".join(_member(b) for b in blocks)


def _inflate_ranges(args):
    path, ranges = args
    with open(path, "rb") as f:
        m = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        n = 0
        for a, z in ranges:
            n += len(zlib.decompressobj(-15).decompress(m[a + 18:z - 8]))
        m.close()
    return n


def write_bam(path, header, n_reads, layout, pool, names, lengths, seed=1):
    rng = np.random.default_rng(seed)
    per_chr = np.diff(np.linspace(0, n_reads, len(names) + 1).astype(np.int64))
    with open(path, "wb") as f:
        f.write(_member(header))
        done, carry = 0, b""
        batch = 200_000
        for c, k in enumerate(per_chr):
            pos_all = np.sort(rng.integers(0, max(1, lengths[c] - 200), k)).astype(np.int32)
            for a in range(0, k, batch):
                n = min(batch, k - a)
                rec = _records(done, n, c, pos_all[a:a + n], rng)
                done += n
                if layout == "aligned":
                    per = BLOCK // REC
                    blocks = [rec[i:i + per].tobytes() for i in range(0, n, per)]
                else:
                    s = carry + rec.tobytes()
                    cut = len(s) - len(s) % BLOCK
                    blocks, carry = [s[i:i + BLOCK] for i in range(0, cut, BLOCK)], s[cut:]
                step = max(1, len(blocks) // 64)
                for out in pool.map(_compress, [blocks[i:i + step] for i in range(0, len(blocks), step)]):
                    f.write(out)
        if carry:
            f.write(_member(carry))
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def members(data):
    off, at = [], 0
    while at < len(data):
        off.append(at)
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
    off.append(len(data))
    return off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--dir", default=None, help="scratch directory for the files (default: a temporary one, removed)")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="bam_bench_")
        atexit.register(shutil.rmtree, a.dir, True)
    os.makedirs(a.dir, exist_ok=True)
    from gffx_amd import synth
    roots = synth.gencode_like_roots(20000, seed=3)
    names = list(roots["names"])
    lengths = [n for _, n in synth.GRCH38][:len(names)]
    header = synth.bam_header(list(zip(names, lengths)))
    res = {"reads": a.reads, "record_bytes": REC, "procs": a.procs}
    ctx = mp.get_context("fork")  # before anything opens the GPU in this process
    paths = {}
    with ctx.Pool(a.procs) as pool:
        for layout in ("aligned", "spanning"):
            p = os.path.join(a.dir, "x_%s.bam" % layout)
            t = time.perf_counter()
            write_bam(p, header, a.reads, layout, pool, names, lengths)
            res["write_s_" + layout] = round(time.perf_counter() - t, 2)
            paths[layout] = p
            data = open(p, "rb").read()
            off = members(data)
            ranges = list(zip(off[:-1], off[1:]))
            step = (len(ranges) + a.procs * 4 - 1) // (a.procs * 4)
            t = time.perf_counter()
            n = sum(pool.map(_inflate_ranges, [(p, ranges[i:i + step]) for i in range(0, len(ranges), step)]))
            dt = time.perf_counter() - t
            res["zlib_%dproc_GBps_%s" % (a.procs, layout)] = round(n / dt / 1e9, 3)
            res["bytes_" + layout] = {"compressed": len(data), "decompressed": n, "members": len(ranges)}
    from gffx_amd import engine
    engine.warmup(0)
    ref_seq = list(range(len(names)))
    for layout, p in paths.items():
        data = open(p, "rb").read()
        dec = res["bytes_" + layout]["decompressed"]
        best = None
        for _ in range(2):
            t = time.perf_counter()
            r = engine.BamReader(ref_seq, len(header), 0)
            r.feed(data)
            r.finish()
            wall = time.perf_counter() - t
            ms, c = r.stage_ms(), r.counts()
            r.close()
            if best is None or wall < best[0]:
                best = (wall, ms, c)
        wall, ms, c = best
        res["device_" + layout] = {"wall_s": round(wall, 3), "inflate_ms": round(ms["inflate"], 2), "frame_ms": round(ms["frame"], 2),
                                   "rows_ms": round(ms["rows"], 2), "inflate_GBps": round(dec / ms["inflate"] / 1e6, 3),
                                   "frame_Mrec_s": round(c["records"] / ms["frame"] / 1e3, 1),
                                   "rows_Mrec_s": round(c["records"] / ms["rows"] / 1e3, 1), "records": c["records"], "kept": c["kept"]}
    # the CLI on the BAM against a BED of the same rows
    gff = os.path.join(a.dir, "g.gff")
    synth.write_gff3_fast(gff, roots)
    gffx = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
    subprocess.check_call([gffx, "index", "-i", gff], stdout=subprocess.DEVNULL)
    rows = engine.bam_rows(open(paths["aligned"], "rb").read(), ref_seq, len(header))
    bed = os.path.join(a.dir, "x.bed")
    synth.write_bed_fast(bed, rows, names)
    for src in (paths["aligned"], paths["spanning"], bed):
        t = time.perf_counter()
        subprocess.check_call([gffx, "depth", "-i", gff, "-s", src, "-o", os.path.join(a.dir, "out.tsv")])
        res["cli_depth_s_" + os.path.basename(src)] = round(time.perf_counter() - t, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
