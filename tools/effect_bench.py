"""Measures `gffx effect` at scale, on the files of tools/seq_bench.py: a GENCODE-shaped GFF3 (synth.write_gff3_fast: gene, mRNA,
exon and CDS lines) over chromosomes shaped like GRCh38 divided by --genome-div and a random genome for the same seqids, with a
synthetic variants file of --snvs single-base substitutions in two modes: `uniform` positions over the genome, and `cds`
positions drawn from the bases of the CDS lines, so that rule 1 (the codon) dominates.

Per mode, one warm-up run and --reps timed runs of the command with --stats-json and --summary, the median [min .. max] of
  the kernels' HIP-event times   build (sort, rows, prefix sums, transcripts), pairs (the engine's direct count and emit passes
                                 over the private span index), classify (k_effect_pairs over all chunks)
  pairs per second               of the classify kernel
  classify beside the roofline   its algorithmic bytes -- per pair the transcript number (4), the transcript (48) and the record
                                 (32), per allele its row, offset and ref_match (21), per pair of rule 1 three prefix sums and
                                 three bases (27); the searches' loads are NOT counted -- over the classify time, against 8 TB/s
  the wall clock                 of the whole command
and beside them one host core: bin/effect_host_baseline (`make effect_host_baseline`: tools/effect_check.cpp --run without the
sanitizers, the same rules through device/effect_core.hpp), likewise one warm-up run and --reps timed ones: its pairs stage (span
lookup + rules: what the pair passes and k_effect_pairs do), its formatting and its wall clock; its output must be the command's,
byte for byte.
--indels (profiles/effect_indels.txt) measures `gffx effect --indels` instead: the `uniform` file with every tenth
allele turned into an indel (`mixed`: a deletion of the genome's own bases or an insertion, by turns, of 1 to 30 bases drawn from
the fixed seed), and the SNV-only `uniform` file run with and without the flag, so that k_effect_pairs_any stands beside
k_effect_pairs on the same pairs; the one-core baseline runs `--run --indels` on the mixed file.
One JSON object on stdout; --profile FILE writes the lines of profiles/effect.txt (the text, then the JSON).  The files are kept
in --dir between runs.
Usage: python tools/effect_bench.py [--genes 63000] [--genome-div 8] [--snvs 5000000] [--seed 5] [--reps 5] [--dir DIR] [--skip-host]
                                    [--profile FILE]"""
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

HBM_BYTES_PER_S = 8e12
CLASSES_RULE_1 = 8  # the first eight classes of the summary read the prefix sums; all but partial_codon the three bases too


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def write_vcf(path, chrom_names, chrom_idx, pos, seed):
    """CHROM POS . REF ALT lines, REF and ALT two different bases (REF is not read from the genome: ref_match is mostly 0)."""
    rng = np.random.RandomState(seed)
    ref = rng.randint(0, 4, len(pos))
    alt = (ref + rng.randint(1, 4, len(pos))) % 4
    bases = "ACGT"
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        step = 1 << 18
        for at in range(0, len(pos), step):
            f.write("".join("%s\t%d\t.\t%s\t%s\n" % (chrom_names[c], p, bases[r], bases[a]) for c, p, r, a in
                            zip(chrom_idx[at:at + step].tolist(), pos[at:at + step].tolist(), ref[at:at + step].tolist(), alt[at:at + step].tolist())))


def write_mixed_vcf(path, snv_vcf, fa, seed):
    """The lines of snv_vcf, every tenth one an indel of 1 to 30 bases at the same POS: by turns a deletion of the genome's own
    bases behind POS (REF = the anchor and the bases, ALT = the anchor) and an insertion of random bases behind the anchor."""
    seqs, name = {}, None
    with open(fa, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                name = line[1:].split()[0].decode()
                seqs[name] = []
            else:
                seqs[name].append(line.rstrip(b"\r\n"))
    seqs = {k: b"".join(v) for k, v in seqs.items()}
    rng = np.random.RandomState(seed)
    n = 0
    with open(snv_vcf) as src, open(path, "w") as out:
        for line in src:
            if line.startswith("#"):
                out.write(line)
                continue
            n += 1
            if n % 10:
                out.write(line)
                continue
            chrom, pos = line.split("\t", 2)[:2]
            pos, ln, seq = int(pos), int(rng.randint(1, 31)), seqs[chrom]
            anchor = seq[pos - 1:pos].decode().upper()
            if (n // 10) % 2 and pos + ln <= len(seq):
                out.write("%s\t%d\t.\t%s\t%s\n" % (chrom, pos, anchor + seq[pos:pos + ln].decode().upper(), anchor))
            else:
                out.write("%s\t%d\t.\t%s\t%s\n" % (chrom, pos, anchor, anchor + "".join("ACGT"[b] for b in rng.randint(0, 4, ln))))


def indel_runs(a, gffx, tool, gff, fa, vcfs):
    """The --indels measurements: {name: {wall_s, build_ms, pairs_ms, classify_ms, alleles, pairs}} for the mixed file with the
    flag, the SNV-only file with it and without it, and the one-core baseline on the mixed file."""
    out, stats = os.path.join(a.dir, "out.tsv"), os.path.join(a.dir, "stats.json")
    mixed = os.path.join(a.dir, "mixed_%d_%d_%d_%d.vcf" % (a.snvs, a.genes, a.genome_div, a.seed))
    if not os.path.exists(mixed):
        write_mixed_vcf(mixed, vcfs["uniform"], fa, a.seed + 4)
    res = {}
    configs = [("mixed --indels", gffx, mixed, ["--indels"]), ("snvs --indels", gffx, vcfs["uniform"], ["--indels"]), ("snvs", gffx, vcfs["uniform"], [])]
    if a.other_gffx:  # (the flagless command of another build, such as the commit before --indels, on the same file)
        configs.append(("snvs, other build", a.other_gffx, vcfs["uniform"], []))
    for name, binary, vcf, flag in configs:
        runs = []
        for k in range(a.reps + 1):
            t0 = time.time()
            r = subprocess.run([binary, "effect", "-i", gff, "-f", fa, "-V", vcf, "-o", out, "--stats-json", stats] + flag, capture_output=True)
            wall = time.time() - t0
            if r.returncode != 0:
                sys.stderr.write(r.stderr.decode(errors="replace"))
                sys.exit(r.returncode)
            flat = json.load(open(stats))
            flat = dict(flat.get("counts", flat), wall_s=wall)
            if k:
                runs.append(flat)
        res[name] = {"alleles": runs[0]["alleles"], "pairs": runs[0]["pairs"], "output_bytes": os.path.getsize(out), "wall_s": spread([x["wall_s"] for x in runs]),
                     "build_ms": spread([x["build_kernels_ms"] for x in runs]), "pairs_ms": spread([x["pair_kernels_ms"] for x in runs]),
                     "classify_ms": spread([x["classify_kernels_ms"] for x in runs])}
        sys.stderr.write("%s: %s\n" % (name, json.dumps(res[name])))
    if a.other_gffx:
        res["flagless_wall_over_other_build"] = round(res["snvs"]["wall_s"]["median"] / res["snvs, other build"]["wall_s"]["median"], 3)
    res["classify_any_over_classify"] = round(res["snvs --indels"]["classify_ms"]["median"] / res["snvs"]["classify_ms"]["median"], 3)
    if not a.skip_host:
        host_out, takes = os.path.join(a.dir, "host.tsv"), []
        for k in range(a.reps + 1):
            t0 = time.time()
            r = subprocess.run([tool, "--run", "--indels", gff, fa, mixed, "CDS", "exon", host_out, "-"], capture_output=True, check=True)
            words = r.stderr.split(b"\n")[-2].split()
            t = dict(zip(words[0::2], (float(x) for x in words[1::2])))
            if k:
                takes.append({"pairs_ms": t[b"pairs_ms"], "format_ms": t[b"format_ms"], "wall_s": time.time() - t0})
        subprocess.check_call([gffx, "effect", "--indels", "-i", gff, "-f", fa, "-V", mixed, "-o", out])
        res["one_host_core mixed --indels"] = dict({k: spread([x[k] for x in takes]) for k in takes[0]}, same_bytes=subprocess.run(["cmp", "-s", out, host_out]).returncode == 0)
        os.remove(host_out)
    return res


def cds_lines(gff):
    """(seqid, start, end) of every CDS line."""
    out = []
    with open(gff, "rb") as f:
        for line in f:
            if line.startswith(b"#"):
                continue
            c = line.split(b"\t", 5)
            if len(c) > 4 and c[2] == b"CDS":
                out.append((c[0].decode(), int(c[3]), int(c[4])))
    return out


def profile_text(r, genome_div):
    """The measurements as profiles/effect.txt lists them, the JSON on the last line."""
    def s(d, unit="ms", fmt="%.3f"):
        return (fmt + " %s [" + fmt + " .. " + fmt + "]") % (d["median"], unit, d["min"], d["max"])

    out = ["gffx effect: GENCODE-shaped synthetic GFF3 (%d genes, %d bytes; gene, mRNA, exon and CDS lines) over chromosomes shaped like GRCh38 / %d (%d bases) and a "
           "random genome for them in lines of 60 (%d bytes of FASTA), with a synthetic variants file of %d single-base substitutions (REF and ALT two random different "
           "bases, REF not read from the genome); one MI355X; per mode one warm-up run, then %d timed runs, of the command and of the one-core baseline alike, median "
           "[min .. max]; kernel times are HIP events summed over the run (--stats-json) (tools/effect_bench.py --profile)"
           % (r["genes"], r["gff_bytes"], genome_div, r["genome_bases"], r["fasta_bytes"], r["snvs"], r["reps"])]
    names = {"uniform": "uniform positions over the genome", "cds": "positions drawn from the bases of the CDS lines (rule 1 dominates)"}
    for mode, m in r["modes"].items():
        out.append("%s (%d alleles, %d pairs = %.1f per allele, %d of them of rule 1; %d of %d transcripts kept; %d chunks; %d bytes of output)"
                   % (names[mode], m["alleles"], m["pairs"], m["pairs"] / max(m["alleles"], 1), m["pairs_rule_1"], m["transcripts_kept"], m["transcripts"], m["chunks"], m["output_bytes"]))
        out.append("  build: keys, radix sort, rows, prefix sum, transcripts (once)                                  " + s(m["build_ms"]))
        out.append("  pairs: the engine's direct count + emit passes over the private span index, all chunks         " + s(m["pairs_ms"]))
        out.append("  classify: k_effect_pairs over all chunks                                                      " + s(m["classify_ms"])
                   + "   %.2f G pairs/s; %.1f GB/s on %d algorithmic bytes (%.1f per pair: per pair 4 + 48 + 32, per allele 21, per pair of rule 1 27; the searches' loads not "
                   "counted) = %.1f %% of 8 TB/s" % (m["classify_pairs_per_s"] / 1e9, m["classify_gb_per_s"], m["classify_algorithmic_bytes"],
                                                      m["classify_algorithmic_bytes_per_pair"], 100 * m["classify_share_of_8_tb_per_s"]))
        out.append("  the host formatting the chunks' lines on its threads and writing them (overlaps the next chunk) " + s(m["format_ms"]))
        out.append("  gffx effect, wall clock                                                                       " + s(m["wall_s"], "s"))
        h = m.get("one_host_core")
        if h:
            out.append("  one host core (bin/effect_host_baseline: effect_core.hpp -O2, a sorted span list with a running maximum for the lookup, the same bytes: %s): variants "
                       "file %s; build %s; pairs (span lookup + rules: what the pair passes and k_effect_pairs do) %s; formatting %s; wall clock %s"
                       % ("yes" if h["same_bytes"] else "NO", s(h["vcf_ms"], fmt="%.1f"), s(h["build_ms"], fmt="%.1f"), s(h["pairs_ms"], fmt="%.1f"), s(h["format_ms"], fmt="%.1f"),
                          s(h["wall_s"], "s")))
        else:
            out.append("  one host core: not measured (--skip-host)")
    out.append("not run: a real human genome, annotation and call set (GRCh38 is %d times this genome, so a real call set meets fewer of these transcripts per "
               "allele); any GFFX_EFFECT_CHUNK_ROWS but the default at scale (the tests run chunks of 1, 3 and 7 alleles on small inputs); a rocprofv3 counter run of "
               "k_effect_pairs (what bounds it is argued from the rates above, not measured by counters); more than one device; bgzipped input (out of scope)" % genome_div)
    out.append(json.dumps(r))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=63000)
    ap.add_argument("--genome-div", type=int, default=8, help="GRCh38's chromosome lengths are divided by this")
    ap.add_argument("--snvs", type=int, default=5000000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory for the files (default: a temporary one, removed)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--other-gffx", default=None, help="with --indels: another build's gffx binary, run without the flag on the SNV-only file beside this one's")
    ap.add_argument("--indels", action="store_true", help="measure --indels on the mixed file and beside the flagless command (profiles/effect_indels.txt)")
    ap.add_argument("--profile", default=None, help="write the measurements as text, then the JSON, to this file")
    a = ap.parse_args()
    if a.dir is None:
        import atexit
        import shutil
        import tempfile
        a.dir = tempfile.mkdtemp(prefix="effect_bench_")
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
    names = [n for n, _ in chroms]
    rng = np.random.RandomState(a.seed + 1)
    vcfs = {}
    for mode in ("uniform", "cds"):
        vcfs[mode] = os.path.join(a.dir, "%s_%d_%d_%d_%d.vcf" % (mode, a.snvs, a.genes, a.genome_div, a.seed))
        if os.path.exists(vcfs[mode]):
            continue
        if mode == "uniform":
            lens = np.array([l for _, l in chroms], dtype=np.int64)
            edges = np.concatenate(([0], np.cumsum(lens)))
            g = rng.randint(0, int(edges[-1]), a.snvs).astype(np.int64)
            ci = np.searchsorted(edges, g, side="right") - 1
            write_vcf(vcfs[mode], names, ci, g - edges[ci] + 1, a.seed + 2)
        else:
            cds = cds_lines(gff)
            number = {n: i for i, n in enumerate(names)}
            c = np.array([number[s] for s, _, _ in cds], dtype=np.int64)
            lo = np.array([s for _, s, _ in cds], dtype=np.int64)
            ln = np.array([e - s + 1 for _, s, e in cds], dtype=np.int64)
            edges = np.concatenate(([0], np.cumsum(ln)))
            g = rng.randint(0, int(edges[-1]), a.snvs).astype(np.int64)
            k = np.searchsorted(edges, g, side="right") - 1
            write_vcf(vcfs[mode], names, c[k], lo[k] + (g - edges[k]), a.seed + 3)
    if a.indels:
        tool = os.path.join(ROOT, "gffx_amd", "bin", "effect_host_baseline")
        if not a.skip_host:
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "effect_host_baseline"], stdout=subprocess.DEVNULL)
        res = {"genes": a.genes, "genome_bases": sum(l for _, l in chroms), "snvs": a.snvs, "reps": a.reps, "runs": indel_runs(a, gffx, tool, gff, fa, vcfs)}
        print(json.dumps(res))
        if a.profile:
            with open(a.profile, "w") as f:
                f.write("gffx effect --indels: tools/effect_bench.py --indels --genes %d --genome-div %d --snvs %d --reps %d; one MI355X; one warm-up run, then the timed "
                        "runs, median [min .. max]; kernel times are HIP events summed over the run\n" % (a.genes, a.genome_div, a.snvs, a.reps))
                f.write("mixed: the uniform SNV file with every tenth allele a deletion or an insertion of 1 to 30 bases; snvs: that file as it is, with the flag (k_effect_pairs_any) and without it (k_effect_pairs); other build: the flagless command of the build given with --other-gffx (the commit before --indels) on the same file; classify_ms is the classify kernel, pairs_ms the engine's pair passes\n")
                for name, m in res["runs"].items():
                    f.write("%s: %s\n" % (name, json.dumps(m)))
                f.write(json.dumps(res) + "\n")
        return
    res = {"genes": a.genes, "genome_bases": sum(l for _, l in chroms), "fasta_bytes": os.path.getsize(fa), "gff_bytes": os.path.getsize(gff), "snvs": a.snvs,
           "reps": a.reps, "modes": {}}
    out, stats, summary = os.path.join(a.dir, "out.tsv"), os.path.join(a.dir, "stats.json"), os.path.join(a.dir, "summary.tsv")
    tool = os.path.join(ROOT, "gffx_amd", "bin", "effect_host_baseline")
    if not a.skip_host:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "effect_host_baseline"], stdout=subprocess.DEVNULL)
    for mode, vcf in vcfs.items():
        runs = []
        for k in range(a.reps + 1):  # (the first one warms the page cache and the device up)
            t0 = time.time()
            r = subprocess.run([gffx, "effect", "-i", gff, "-f", fa, "-V", vcf, "-o", out, "--summary", summary, "--stats-json", stats], capture_output=True)
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
        per_class = [line.split("\t") for line in open(summary).read().split("\n")[:-1]]
        pairs, alleles = float(first["pairs"]), float(first["alleles"])
        rule_1 = sum(int(p) for _, _, p in per_class[:CLASSES_RULE_1])
        algo = 84.0 * pairs + 21.0 * alleles + 27.0 * rule_1
        classify = [x["classify_kernels_ms"] for x in runs]
        med = statistics.median(classify) * 1e-3
        m = {"alleles": alleles, "pairs": pairs, "pairs_rule_1": rule_1, "transcripts": first["transcripts"], "transcripts_kept": first["transcripts_kept"],
             "chunks": first["chunks"], "output_bytes": os.path.getsize(out), "classes": {c: [int(x), int(p)] for c, x, p in per_class},
             "build_ms": spread([x["build_kernels_ms"] for x in runs]), "pairs_ms": spread([x["pair_kernels_ms"] for x in runs]), "classify_ms": spread(classify),
             "format_ms": spread([x["format_ms"] for x in runs]), "wall_s": spread([x["wall_s"] for x in runs]),
             "classify_pairs_per_s": round(pairs / med, 0) if med else None, "classify_algorithmic_bytes": algo,
             "classify_algorithmic_bytes_per_pair": round(algo / pairs, 1) if pairs else None,
             "classify_gb_per_s": round(algo / med / 1e9, 1) if med else None, "classify_share_of_8_tb_per_s": round(algo / med / HBM_BYTES_PER_S, 4) if med else None}
        if not a.skip_host:
            host_out = os.path.join(a.dir, "host.tsv")
            takes = []
            for k in range(a.reps + 1):  # (the first one warms the page cache up)
                t0 = time.time()
                r = subprocess.run([tool, "--run", gff, fa, vcf, "CDS", "exon", host_out, "-"], capture_output=True, check=True)
                words = r.stderr.split(b"\n")[-2].split()
                t = dict(zip(words[0::2], (float(x) for x in words[1::2])))
                if k:
                    takes.append({"vcf_ms": t[b"vcf_ms"], "build_ms": t[b"build_ms"], "pairs_ms": t[b"pairs_ms"], "format_ms": t[b"format_ms"],
                                  "total_ms": t[b"total_ms"], "wall_s": time.time() - t0})
            m["one_host_core"] = {k: spread([x[k] for x in takes]) for k in takes[0]}
            m["one_host_core"]["same_bytes"] = subprocess.run(["cmp", "-s", out, host_out]).returncode == 0
            os.remove(host_out)
        res["modes"][mode] = m
        sys.stderr.write("%s: %s\n" % (mode, json.dumps(m)))
    print(json.dumps(res))
    if a.profile:
        with open(a.profile, "w") as f:
            f.write(profile_text(res, a.genome_div))


if __name__ == "__main__":
    main()
