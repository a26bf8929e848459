"""Seeded synthetic inputs for the `gffx intersect` path.

Nothing real (GENCODE GFF3, BED) is available offline, so every workload is generated:

* ``gencode_like_roots``  -- the root-feature intervals of a GENCODE/GRCh38-shaped annotation
  as arrays (what the reference keeps in its per-seqid interval trees,
  index_builder/core.rs:170-180), without materialising the GFF text;
* ``write_gff3``          -- a GFF3 text with gene -> mRNA -> exon/CDS models whose roots are
  exactly those intervals (plus optional quirks the reference's builder has to survive);
* ``synth_bed`` / ``write_bed`` -- BED query regions: chromosome drawn proportionally to its
  length, start uniform, width uniform in [100, 10000], rows in random order.

All randomness is numpy PCG64 with the seed given by the caller.
"""
from __future__ import annotations

import os
import subprocess
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

GRCH38: List[Tuple[str, int]] = [
    ("chr1", 248956422), ("chr2", 242193529), ("chr3", 198295559), ("chr4", 190214555),
    ("chr5", 181538259), ("chr6", 170805979), ("chr7", 159345973), ("chr8", 145138636),
    ("chr9", 138394717), ("chr10", 133797422), ("chr11", 135086622), ("chr12", 133275309),
    ("chr13", 114364328), ("chr14", 107043718), ("chr15", 101991189), ("chr16", 90338345),
    ("chr17", 83257441), ("chr18", 80373285), ("chr19", 58617616), ("chr20", 64444167),
    ("chr21", 46709983), ("chr22", 50818468), ("chrX", 156040895), ("chrY", 57227415),
    ("chrM", 16569),
]

SMALL2: List[Tuple[str, int]] = [("chr1", 3_000_000), ("chr2", 2_000_000)]


def gencode_like_roots(n_genes: int = 63000, seed: int = 42,
                       chroms: Sequence[Tuple[str, int]] = GRCH38,
                       fid_stride: int = 54) -> Dict[str, np.ndarray]:
    """Root intervals, per chromosome in file order (sorted by 1-based gene start).

    Returns dict with ``chr_offsets`` (n_chr+1), ``start`` (0-based), ``end`` (exclusive),
    ``fid`` (root feature ids, increasing in file order, ~fid_stride apart like a gene with
    ~53 child lines) -- the tree inputs of index_builder/core.rs:177-180.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.array([l for _, l in chroms], dtype=np.float64)
    per = np.maximum(1, np.round(n_genes * lens / lens.sum()).astype(np.int64))
    starts, ends, offs = [], [], [0]
    for (name, clen), k in zip(chroms, per):
        glen = np.exp(rng.normal(np.log(4000.0), 2.007, size=k))
        glen = np.clip(glen, 50, min(2_400_000, max(50, clen - 2))).astype(np.int64)
        s1 = 1 + (rng.random(k) * np.maximum(1, clen - glen)).astype(np.int64)  # 1-based start
        order = np.argsort(s1, kind="stable")
        s1, glen = s1[order], glen[order]
        starts.append(s1 - 1)
        ends.append(np.minimum(s1 + glen - 1, clen))
        offs.append(offs[-1] + k)
    start = np.concatenate(starts).astype(np.uint32)
    end = np.concatenate(ends).astype(np.uint32)
    fid = (np.arange(len(start), dtype=np.uint64) * fid_stride).astype(np.uint32)
    return {"chr_offsets": np.array(offs, dtype=np.uint32), "start": start, "end": end, "fid": fid,
            "names": [n for n, _ in chroms]}


def synth_bed(n: int, seed: int, chroms: Sequence[Tuple[str, int]] = GRCH38,
              width: Tuple[int, int] = (100, 10000), edge_frac: float = 0.0,
              roots: Optional[Dict[str, np.ndarray]] = None) -> np.ndarray:
    """(n,3) uint32 AoS rows (chr index, start, end), unsorted.

    ``edge_frac`` of the rows are replaced by edge cases the reference keeps and queries as-is
    (commands/intersect.rs:223-225): s==e, s>e, s=0, and -- when ``roots`` is given -- regions
    touching a root's boundary exactly.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.array([l for _, l in chroms], dtype=np.float64)
    chr_idx = rng.choice(len(chroms), size=n, p=lens / lens.sum()).astype(np.int64)
    clen = np.array([l for _, l in chroms], dtype=np.int64)[chr_idx]
    w = rng.integers(width[0], width[1] + 1, size=n)
    w = np.minimum(w, np.maximum(1, clen - 1))
    s = (rng.random(n) * np.maximum(1, clen - w)).astype(np.int64)
    e = s + w
    if edge_frac > 0 and n > 0:
        k = max(1, int(n * edge_frac))
        pick = rng.choice(n, size=k, replace=False)
        kind = rng.integers(0, 5 if roots is not None else 3, size=k)
        for i, kd in zip(pick, kind):
            if kd == 0:
                e[i] = s[i]
            elif kd == 1:
                s[i], e[i] = e[i], s[i]
            elif kd == 2:
                e[i] = e[i] - s[i]
                s[i] = 0
            else:
                c = chr_idx[i]
                lo, hi = int(roots["chr_offsets"][c]), int(roots["chr_offsets"][c + 1])
                if hi > lo:
                    j = int(rng.integers(lo, hi))
                    if kd == 3:  # region ends exactly where the root starts / starts where it ends
                        if rng.random() < 0.5 and roots["start"][j] > 0:
                            e[i] = int(roots["start"][j])
                            s[i] = max(0, int(e[i]) - int(w[i]))
                        else:
                            s[i] = int(roots["end"][j])
                            e[i] = int(s[i]) + int(w[i])
                    else:  # region == root interval (both containment predicates fire)
                        s[i], e[i] = int(roots["start"][j]), int(roots["end"][j])
    out = np.empty((n, 3), dtype=np.uint32)
    out[:, 0] = chr_idx
    out[:, 1] = s
    out[:, 2] = e
    return out


def gencode_like_block_table(roots: Dict[str, np.ndarray], seed: int = 7, lines_per_gene: float = 53.0):
    """The feature-line table of `gffx depth` (include/gffx_hip.h) for ``roots`` without materialising GFF
    text: per root one block holding the gene line plus ~``lines_per_gene`` child lines (transcripts,
    exons, CDS) with 0-based half-open coordinates inside the gene; 30 % of the lines share their ID with
    the previous one (multi-line CDS), so groups are ~0.7 per line.  Returns a dict with ``block_line_off``
    (u64), ``line_start/line_end/line_group`` (u32), ``block_of_fid`` (u32, indexed by root fid) and
    ``n_groups``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(roots["fid"])
    per = 1 + rng.poisson(lines_per_gene, size=n).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    total = int(off[-1])
    blk = np.repeat(np.arange(n), per)
    gs = roots["start"].astype(np.int64)[blk]
    ge = roots["end"].astype(np.int64)[blk]
    span = np.maximum(ge - gs, 1)
    a = gs + (rng.random(total) * span).astype(np.int64)
    w = 1 + (rng.random(total) * np.minimum(span, 2000)).astype(np.int64)
    first = np.zeros(total, bool)
    first[off[:-1].astype(np.int64)] = True
    a[first], w[first] = gs[first], span[first]  # the gene line itself
    b = np.minimum(a + w, ge)
    b = np.maximum(b, a + 1)
    new_group = first | (rng.random(total) > 0.3)
    group = np.cumsum(new_group) - 1
    block_of_fid = np.full(int(roots["fid"].max()) + 1, 0xFFFFFFFF, np.uint32)
    block_of_fid[roots["fid"]] = np.arange(n, dtype=np.uint32)
    return {"block_line_off": off, "line_start": a.astype(np.uint32), "line_end": b.astype(np.uint32),
            "line_group": group.astype(np.uint32), "block_of_fid": block_of_fid, "n_groups": int(group[-1]) + 1}


def write_bed(path: str, regions: np.ndarray, names: Sequence[str], extra_lines: Sequence[str] = ()) -> None:
    with open(path, "w") as f:
        for ln in extra_lines:
            f.write(ln)
        for c, s, e in regions.tolist():
            f.write("%s\t%d\t%d\n" % (names[c], s, e))


def write_gff3(path: str, roots: Dict[str, np.ndarray], seed: int = 7, tx_per_gene: float = 2.0,
               exons_per_tx: float = 4.0, quirks: bool = False, crlf: bool = False) -> int:
    """Write a GFF3 whose root features are ``roots`` (1-based closed coordinates in the text).

    With ``quirks`` the file also carries what the reference's builder and writers have to cope
    with: `##sequence-region` directives and `region`-typed lines (a skipped
    type, index_builder/core.rs:95-100) in front of each chromosome -- i.e. physically inside the
    previous gene's block --, comment lines inside blocks, a blank line, a feature whose Parent
    is a comma list (becomes its own root), an orphan whose Parent never appears, and a reversed
    start/end pair.  Returns the number of lines written.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    names = roots["names"]
    eol = "\r\n" if crlf else "\n"
    n_lines = 0
    with open(path, "w", newline="") as f:
        def w(s: str) -> None:
            nonlocal n_lines
            f.write(s + eol)
            n_lines += 1

        w("##gff-version 3")
        gi = 0
        for c, name in enumerate(names):
            lo, hi = int(roots["chr_offsets"][c]), int(roots["chr_offsets"][c + 1])
            if quirks:
                w("##sequence-region %s 1 %d" % (name, 300_000_000))
                w("%s\tsynth\tregion\t1\t%d\t.\t+\t.\tID=%s;Name=%s" % (name, 300_000_000, name, name))
            for j in range(lo, hi):
                gs, ge = int(roots["start"][j]) + 1, int(roots["end"][j])
                strand = "+" if rng.random() < 0.5 else "-"
                gid = "gene%06d" % gi
                w("%s\tsynth\tgene\t%d\t%d\t.\t%s\t.\tID=%s;gene_name=G%d;gene_type=protein_coding"
                  % (name, gs, ge, strand, gid, gi))
                ntx = max(1, int(rng.poisson(tx_per_gene)))
                for t in range(ntx):
                    tid = "%s.t%d" % (gid, t)
                    ts = gs + int(rng.integers(0, max(1, (ge - gs) // 4 + 1)))
                    te = max(ts, ge - int(rng.integers(0, max(1, (ge - gs) // 4 + 1))))
                    w("%s\tsynth\tmRNA\t%d\t%d\t.\t%s\t.\tID=%s;Parent=%s;gene_name=G%d"
                      % (name, ts, te, strand, tid, gid, gi))
                    nex = max(1, int(rng.poisson(exons_per_tx)))
                    cuts = np.sort(rng.integers(ts, te + 1, size=2 * nex))
                    for x in range(nex):
                        xs, xe = int(cuts[2 * x]), int(cuts[2 * x + 1])
                        w("%s\tsynth\texon\t%d\t%d\t.\t%s\t.\tID=%s.e%d;Parent=%s"
                          % (name, xs, xe, strand, tid, x, tid))
                        if rng.random() < 0.6:
                            w("%s\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tID=%s.c%d;Parent=%s"
                              % (name, xs, xe, strand, tid, x, tid))
                    if quirks and rng.random() < 0.05:
                        w("# a comment inside a gene model")
                if quirks and rng.random() < 0.03:
                    w("")
                if quirks and rng.random() < 0.04:
                    # Parent is a comma list -> unresolvable -> the feature is its own root
                    # (index_builder/core.rs:117,163-167) and opens a new block
                    w("%s\tsynth\tmRNA\t%d\t%d\t.\t%s\t.\tID=multi%d;Parent=%s,gene%06d"
                      % (name, gs, ge, strand, gi, gid, max(0, gi - 1)))
                if quirks and rng.random() < 0.04:
                    # Parent never appears anywhere -> own root as well
                    w("%s\tsynth\texon\t%d\t%d\t.\t%s\t.\tID=orphan%d;Parent=nowhere%d"
                      % (name, gs, min(ge, gs + 99), strand, gi, gi))
                if quirks and rng.random() < 0.03:
                    # a second root line re-using the gene's ID: both lines alias to the LAST
                    # line's index (core.rs:141-144,160); the .gof lookup keeps the last record
                    w("%s\tsynth\tgene\t%d\t%d\t.\t%s\t.\tID=%s;gene_name=G%ddup"
                      % (name, gs + 10, ge + 10, strand, gid, gi))
                gi += 1
        if quirks:
            last = names[-1]
            # reversed coordinates on a child (core.rs:107 swaps them for the index only)
            w("%s\tsynth\texon\t900\t850\t.\t+\t.\tID=rev.e0;Parent=gene%06d" % (last, gi - 1))
    return n_lines


# ---- fast text writers (tools/synth_text.c, built by __graft_entry__.build()): 3.4 M GFF lines / 100 M BED rows in seconds
_SYNTH_TEXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin", "synth_text")


def build_synth_text() -> str:
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "synth_text.c")
    if not os.path.exists(_SYNTH_TEXT) or (os.path.exists(src) and os.path.getmtime(src) > os.path.getmtime(_SYNTH_TEXT)):
        os.makedirs(os.path.dirname(_SYNTH_TEXT), exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-o", _SYNTH_TEXT, src, "-lm"])
    return _SYNTH_TEXT


def _write_names(path: str, names: Sequence[str]) -> None:
    with open(path, "w") as f:
        f.write("".join(n + "\n" for n in names))


def write_gff3_fast(path: str, roots: Dict[str, np.ndarray], tx_per_gene: float = 4.0, exons_per_tx: float = 8.0,
                    seed: int = 7) -> int:
    """GENCODE-shaped GFF3 around ``roots`` (gene + mRNA + exon/CDS lines; ~54 lines per gene at the defaults, i.e.
    ~3.4 M lines for 63 k genes).  Returns the number of lines."""
    tool = build_synth_text()
    tmp = path + ".roots.bin"
    with open(tmp, "wb") as f:
        co = np.ascontiguousarray(roots["chr_offsets"], dtype=np.uint32)
        np.array([len(co) - 1, len(roots["start"])], dtype=np.uint32).tofile(f)
        co.tofile(f)
        np.ascontiguousarray(roots["start"], dtype=np.uint32).tofile(f)
        np.ascontiguousarray(roots["end"], dtype=np.uint32).tofile(f)
    _write_names(path + ".names", roots["names"])
    out = subprocess.check_output([tool, "gff", tmp, path + ".names", path, str(tx_per_gene), str(exons_per_tx), str(seed)])
    os.remove(tmp)
    os.remove(path + ".names")
    return int(out.strip())


def write_fasta_fast(path: str, chroms: Sequence[Tuple[str, int]], width: int = 60, seed: int = 7) -> int:
    """A random genome (ACGT, a few N) for ``chroms`` = (name, length) pairs in lines of ``width``.  Returns the bases written."""
    tool = build_synth_text()
    tmp = path + ".lengths"
    with open(tmp, "w") as f:
        f.write("".join("%s\t%d\n" % (n, l) for n, l in chroms))
    out = subprocess.check_output([tool, "fasta", tmp, path, str(width), str(seed)])
    os.remove(tmp)
    return int(out.strip())


def write_bed_fast(path: str, regions: np.ndarray, names: Sequence[str]) -> None:
    tool = build_synth_text()
    tmp = path + ".regions.bin"
    with open(tmp, "wb") as f:
        np.array([len(regions)], dtype=np.uint64).tofile(f)
        np.ascontiguousarray(regions, dtype=np.uint32).tofile(f)
    _write_names(path + ".names", names)
    subprocess.check_call([tool, "bed", tmp, path + ".names", path])
    os.remove(tmp)
    os.remove(path + ".names")


# ---- BAM (SAM spec §4.2) in BGZF (§4.1), written with Python's zlib: test and benchmark inputs of the BAM source path ----
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_BLOCK = 0xFF00  # htslib's uncompressed block size


def bgzf_member(data: bytes, level: int = 6, strategy: int = 0) -> bytes:
    """One BGZF member: a gzip member with the BC subfield (BSIZE), raw DEFLATE, CRC32, ISIZE."""
    import struct
    import zlib
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body = c.compress(data) + c.flush()
    total = 18 + len(body) + 8
    if total > 65536 or len(data) > 65536:
        raise ValueError("BGZF member too large (%d bytes in, %d out)" % (len(data), total))
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + body +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bam_header(refs: Sequence[Tuple[str, int]], text: bytes = b"") -> bytes:
    import struct
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        nb = name.encode() + b"\x00"
        out += [struct.pack("<i", len(nb)), nb, struct.pack("<i", length)]
    return b"".join(out)


CIGAR_OPS = "MIDNSHP=X"


def bam_record(tid: int, pos: int, flag: int = 0, cigar: Sequence[Tuple[int, int]] = ((0, 150),), name: bytes = b"r",
               l_seq: int = 0, tags: bytes = b"", mapq: int = 60) -> bytes:
    """One record; cigar = (op, length) pairs, op 0..8 = MIDNSHP=X."""
    import struct
    rn = name + b"\x00"
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    body = (struct.pack("<iiBBHHHiiii", tid, pos, len(rn), mapq, 4680, len(cigar), flag, l_seq, -1, -1, 0) + rn + cig +
            bytes((l_seq + 1) // 2) + b"\xff" * l_seq + tags)
    return struct.pack("<i", len(body)) + body


def bam_end(pos: int, cigar: Sequence[Tuple[int, int]]) -> int:
    """htslib's bam_endpos as restated in device/bgzf_core.hpp: pos + the M/D/N/=/X lengths, a sum of 0 counting as 1."""
    rlen = sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
    return pos + (rlen if rlen else 1)


def bgzf_blocks(header: bytes, records: Sequence[bytes], layout: str = "aligned", flush_header: bool = True,
                block: int = BGZF_BLOCK) -> List[bytes]:
    """The uncompressed payloads of the members.  aligned: htslib's writer (a block is flushed before a record that would
    not fit; a record larger than a block is cut into full blocks); spanning: one stream cut every `block` bytes (htsjdk)."""
    if layout == "spanning":
        s = header + b"".join(records)
        return [s[i:i + block] for i in range(0, len(s), block)]
    out, cur = [], bytearray()
    pending = [(header, flush_header)] + [(r, False) for r in records]
    for data, flush_after in pending:
        if cur and len(cur) + len(data) > block:
            out.append(bytes(cur))
            cur = bytearray()
        cur += data
        while len(cur) > block:
            out.append(bytes(cur[:block]))
            del cur[:block]
        if flush_after and cur:
            out.append(bytes(cur))
            cur = bytearray()
    if cur:
        out.append(bytes(cur))
    return out


def write_bam(path: str, header: bytes, records: Sequence[bytes], layout: str = "aligned", level: int = 6, strategy: int = 0,
              eof: bool = True, flush_header: bool = True, block: int = BGZF_BLOCK) -> int:
    """Writes a BAM file; returns the header's size in the decompressed stream."""
    with open(path, "wb") as f:
        for b in bgzf_blocks(header, records, layout, flush_header, block):
            f.write(bgzf_member(b, level, strategy))
        if eof:
            f.write(BGZF_EOF)
    return len(header)


def bam_test_records(n: int, seed: int, refs: Sequence[Tuple[str, int]], big: bool = True) -> List[tuple]:
    """Coordinate-sorted records with every quirk the BAM path has a rule for: (record bytes, tid, pos, flag, cigar).
    Unmapped reads, refID -1, pos -1, every CIGAR op, all-clip and empty CIGARs, an end past 2^32, a kSmN record with
    its CIGAR in a CG tag, and (big) one record larger than a BGZF block."""
    import struct
    rng = np.random.default_rng(seed)
    out = []
    n_ref = len(refs)
    pos = np.sort(rng.integers(0, 2_000_000, n))
    tids = np.sort(rng.integers(0, n_ref, n))
    for i in range(n):
        tid, p, flag = int(tids[i]), int(pos[i]), int(rng.choice([0, 16, 0x100, 0x400, 0x4, 0x4 | 0x10], p=[.5, .2, .1, .1, .07, .03]))
        k = int(rng.integers(0, 20))
        if k == 0:
            cigar = []
        elif k == 1:
            cigar = [(4, 50), (1, 3), (5, 9), (6, 2)]  # S I H P only: reference length 0 -> 1
        else:
            cigar = [(int(rng.integers(0, 9)), int(rng.integers(1, 300))) for _ in range(int(rng.integers(1, 7)))]
        l_seq = int(rng.integers(0, 160))
        tags = b"NMC\x02" if rng.random() < 0.3 else b""
        if rng.random() < 0.01:
            tid = -1
        if rng.random() < 0.01:
            p = -1
        out.append((bam_record(tid, p, flag, cigar, b"q%d" % i, l_seq, tags), tid, p, flag, cigar))
    # an end clamped at 2^32 - 1, a kSmN placeholder, a record larger than a BGZF block
    cig = [(3, (1 << 28) - 1)] * 10
    out.append((bam_record(n_ref - 1, 2_000_000_000, 0, cig, b"far"), n_ref - 1, 2_000_000_000, 0, cig))
    real = [(0, 100), (3, 5000), (0, 50)]
    cg = b"CGBI" + struct.pack("<i", len(real)) + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in real)
    ksmn = [(4, 150), (3, 5150)]
    out.append((bam_record(0, 1234, 0, ksmn, b"long", 150, cg), 0, 1234, 0, ksmn))
    if big:
        tag = b"XXZ" + b"A" * 150000 + b"\x00"
        out.append((bam_record(0, 777, 0, [(0, 80)], b"huge", 80, tag), 0, 777, 0, [(0, 80)]))
    return out


def bam_rows_definition(recs: Sequence[tuple], ref_seq: Sequence[int]) -> np.ndarray:
    """depth.rs:335-364 restated: the (seqid, start, end) rows a list of bam_test_records keeps, in file order."""
    rows = []
    for _, tid, pos, flag, cigar in recs:
        if flag & 0x4 or tid < 0 or ref_seq[tid] == 0xFFFFFFFF or pos < 0:
            continue
        end = bam_end(pos, cigar)
        if end <= pos:
            continue
        rows.append((ref_seq[tid], min(pos, 0xFFFFFFFF), min(end, 0xFFFFFFFF)))
    return np.array(rows, dtype=np.uint32).reshape(-1, 3)


def bam_sized_record(size: int, tid: int, pos: int, name: bytes, seed: int = 0) -> tuple:
    """A record of exactly `size` bytes, the block_size field included: a long read whose bulk is one Z tag of random bases."""
    cigar = [(0, 5000), (2, 7), (0, 300)]
    fixed = len(bam_record(tid, pos, 0, cigar, name, 0, b"XXZ\x00"))
    assert size >= fixed
    bases = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, size - fixed)].tobytes()
    rec = bam_record(tid, pos, 0, cigar, name, 0, b"XXZ" + bases + b"\x00")
    assert len(rec) == size
    return (rec, tid, pos, 0, cigar)


LONG_READ_GROUPS = ((BGZF_BLOCK, 1), (BGZF_BLOCK + 1, 2), (2 * BGZF_BLOCK, 3), (300_000, 2), (1_000_000, 1), (BGZF_BLOCK, 3),
                    (1_000_000, 2), (BGZF_BLOCK + 1, 1), (300_000, 3))


def bam_long_read_records(n: int, seed: int, refs: Sequence[Tuple[str, int]], groups=LONG_READ_GROUPS) -> List[tuple]:
    """A long-read file's records: the n + 2 ordinary records of bam_test_records(big=False) and, spread evenly between them,
    groups of back-to-back records of exactly the given sizes (size in bytes with the block_size field, records in the group):
    one block, one block + 1, two blocks, 0.3 MB and 1 MB."""
    base = bam_test_records(n, seed, refs, big=False)
    out, step = [], len(base) // (len(groups) + 1)
    for g, (size, count) in enumerate(groups):
        out += base[g * step:(g + 1) * step]
        _, tid, pos, _, _ = out[-1]
        tid, pos = max(tid, 0), max(pos, 0)
        out += [bam_sized_record(size, tid, pos + k, b"long%d.%d" % (g, k), seed * 1000 + g * 10 + k) for k in range(count)]
    return out + base[len(groups) * step:]


# ---- SAM text (SAM spec §1.3, §1.4): test and benchmark inputs of the SAM source path -----------------------------------
def sam_header(refs: Sequence[Tuple[str, int]], text: bytes = b"") -> bytes:
    """@HD, one @SQ line per reference in order, then `text` (further complete header lines, e.g. @CO)."""
    return b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), ln) for n, ln in refs) + text


def sam_cigar(cigar) -> bytes:
    """(op, length) pairs as text; no pairs: `*`.  bytes pass through (a test's malformed CIGAR)."""
    if isinstance(cigar, bytes):
        return cigar
    return b"".join(b"%d%s" % (ln, CIGAR_OPS[op].encode()) for op, ln in cigar) or b"*"


def sam_line(rname, pos: int, flag: int = 0, cigar=((0, 150),), name: bytes = b"r", l_seq: int = 0, tags: bytes = b"",
             mapq: int = 60) -> bytes:
    """One alignment line without its newline.  rname: a name or None (`*`); pos: 0-based as in BAM (POS = pos + 1, so -1 gives
    POS 0); tags: text, TAB-separated."""
    rn = b"*" if rname is None else (rname if isinstance(rname, bytes) else rname.encode())
    seq = b"A" * l_seq if l_seq else b"*"
    fields = [name, b"%d" % flag, rn, b"%d" % (pos + 1), b"%d" % mapq, sam_cigar(cigar), b"*", b"0", b"0", seq, b"*"]
    if tags:
        fields.append(tags)
    return b"\t".join(fields)


def sam_records_from(recs: Sequence[tuple], refs: Sequence[Tuple[str, int]]) -> List[bytes]:
    """The records of bam_test_records / bam_long_read_records as SAM lines: tid -1 becomes `*`, pos -1 POS 0, an empty CIGAR
    `*`; the binary tags become one Z tag of their size, so a record of 1 MB is a line of about 1 MB."""
    import struct
    out = []
    for rec, tid, pos, flag, cigar in recs:
        l_name, n_cig = rec[12], struct.unpack_from("<H", rec, 16)[0]
        l_seq = struct.unpack_from("<i", rec, 20)[0]
        name = rec[36:36 + l_name - 1]
        n_tags = len(rec) - (36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq)
        tags = b"XX:Z:" + b"A" * (n_tags - 5) if n_tags > 5 else (b"NM:i:2" if n_tags else b"")
        out.append(sam_line(None if tid < 0 else refs[tid][0], pos, flag, cigar, name, l_seq, tags))
    return out


def write_sam(path: str, header: bytes, lines: Sequence[bytes], bgzf: bool = False, layout: str = "aligned", newline: bytes = b"\n",
              final_newline: bool = True, flush_header: bool = True, block: int = BGZF_BLOCK, eof: bool = True) -> int:
    """Writes a SAM file, plain or BGZF-compressed (the text cut into members by bgzf_blocks: aligned = a member ends before
    a line that would not fit, spanning = cut every `block` bytes); returns the header's size in the text."""
    if newline != b"\n":
        header = header.replace(b"\n", newline)
    recs = [ln + newline for ln in lines]
    if recs and not final_newline:
        recs[-1] = recs[-1][:-len(newline)]
    with open(path, "wb") as f:
        if not bgzf:
            f.write(header + b"".join(recs))
        else:
            for b in bgzf_blocks(header, recs, layout, flush_header, block):
                f.write(bgzf_member(b))
            if eof:
                f.write(BGZF_EOF)
    return len(header)


def sam_counts_definition(recs: Sequence[tuple], ref_seq: Sequence[int]) -> Dict[str, int]:
    """The tallies of the SAM reader on the lines of sam_records_from(recs): unmapped = flag 0x4 or, ASSUMED htslib behaviour,
    a `*` CIGAR; no_seq = mapped, RNAME `*` or not in the index."""
    c = {"lines": len(recs), "unmapped": 0, "no_seq": 0, "kept": 0}
    for _, tid, pos, flag, cigar in recs:
        if flag & 0x4 or not cigar:
            c["unmapped"] += 1
        elif tid < 0 or ref_seq[tid] == 0xFFFFFFFF:
            c["no_seq"] += 1
        elif pos >= 0 and bam_end(pos, cigar) > pos:
            c["kept"] += 1
    return c


def sam_rows_definition(recs: Sequence[tuple], ref_seq: Sequence[int]) -> np.ndarray:
    """bam_rows_definition plus the rule of the SAM parser: a record whose CIGAR is `*` (no operations) is dropped -- ASSUMED
    htslib behaviour ("mapped query must have a CIGAR; treated as unmapped"), see device/sam_core.hpp."""
    return bam_rows_definition([r for r in recs if r[4]], ref_seq)
