"""The shared BGZF / DEFLATE decoder (device/bgzf_core.hpp, host build under ASan + UBSan: tools/bgzf_check.cpp) on streams
that zlib's encoder does not write, made by the tests' own DEFLATE writer (tests/_deflate_writer.py): 15-bit codes, distance
symbols 28 / 29, both spellings of length 258, code-length repeats across the border of the two tables (libdeflate's block
headers), one-code and empty distance tables, HLIT = HDIST = 29, empty blocks, stored blocks after bit-unaligned ones.
zlib's inflate is the reference for the writer; the writer's own description says which features the corpus holds.  Near
misses of those streams stay rejected.  And the framing of long-read files, one-record members and foreign gzip headers
(the file shapes of tests/test_bam_shapes_gpu.py) against the Python restatement.  No GPU."""
import os
import subprocess
import zlib
from collections import Counter

import numpy as np
import pytest

import _deflate_writer as dw
from gffx_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "bgzf_check")


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "bgzf_check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def corpus():
    return dw.corpus()


def _zlib_inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    assert d.eof and d.unused_data == b""  # the stream ends, and ends with the last byte
    return out


def test_the_writer_equals_zlib(corpus):
    assert len(corpus) >= len(dw.directed_cases()) + 300
    for name, m, data, _ in corpus:
        assert len(m) <= 65536 and len(data) <= 65536, name
        assert _zlib_inflate(m[18:-8]) == data, name
    for name, m, data in dw.stripe_edge_members():
        assert _zlib_inflate(m[18:-8]) == data and len(m) <= 65536, name
    rng = np.random.default_rng(4)
    for k, data in enumerate((b"", b"a", b"ab" * 32768, rng.integers(0, 256, 65280, dtype=np.uint8).tobytes(),
                              bytes(rng.integers(65, 69, 65536, dtype=np.uint8)), b"A" * 65536)):
        m = dw.compress_member(data, k)
        assert _zlib_inflate(m[18:-8]) == data and len(m) <= 65536, k


def test_the_corpus_holds_every_feature(corpus):
    """Counted from the writer's description of each member: no decoder is asked."""
    total = Counter()
    for _, _, _, feat in corpus:
        total += feat
    missing = [f for f in dw.FEATURES if total[f] < 1]
    assert not missing, "the corpus lacks: " + "; ".join(missing)
    random_only = Counter()
    for name, _, _, feat in corpus:
        if name.startswith("random"):
            random_only += feat
    # the random members by themselves reach the long codes and the joined headers too (not only the directed cases)
    for f in ("used 15-bit literal/length code", "used distance code longer than 9 bits", "repeat 18 across the table border",
              "stored after a bit-unaligned Huffman block"):
        assert random_only[f] >= 1, f


def test_host_decoder_equals_the_writer(tool, tmp_path, corpus):
    src, dst = tmp_path / "corpus.gz", tmp_path / "corpus.out"
    src.write_bytes(b"".join(m for _, m, _, _ in corpus) + synth.BGZF_EOF)
    r = _run(tool, "inflate", src, dst)
    starts = np.cumsum([0] + [len(m) for _, m, _, _ in corpus])
    bad = [name for (name, _, _, _), at in zip(corpus, starts) if r.stdout.rstrip().endswith(" offset %d" % at)]
    assert r.returncode == 0, (bad, r.stdout)  # (the member at the offset the tool names)
    got, at = dst.read_bytes(), 0
    for name, _, data, _ in corpus:
        assert got[at:at + len(data)] == data, name
        at += len(data)
    assert at == len(got)
    edges = dw.stripe_edge_members()
    src.write_bytes(b"".join(m for _, m, _ in edges))
    assert _run(tool, "inflate", src, dst).returncode == 0
    assert dst.read_bytes() == b"".join(d for _, _, d in edges)


def test_member_header_variants_on_the_host(tool, tmp_path):
    data = b"other writers' gzip headers " * 30
    raw = dw.deflate(dw.compress(data, 1))[0]
    members = [dw.member(raw, data, **v) for v in dw.HEADER_VARIANTS.values()]
    assert len({len(m) for m in members}) > 3
    src, dst = tmp_path / "h.gz", tmp_path / "h.out"
    src.write_bytes(b"".join(members) + synth.BGZF_EOF)
    assert _run(tool, "inflate", src, dst).returncode == 0
    assert dst.read_bytes() == data * len(members)


def _near_misses():
    """{name: (valid blocks, the same with one field changed)}"""
    rng = np.random.default_rng(2)
    ll = dw.spread(dw.random_complete(40, 9, rng), list(range(90, 126)) + [256, 257, 258, 259], 286)
    dl = dw.spread([1, 2, 2], [0, 1, 2], 30)
    items = list(bytes(rng.integers(90, 126, 80, dtype=np.uint8))) + [(3, 1), (4, 2), (5, 3)]
    seq = ll + dl  # HLIT = HDIST = 29
    plain = [(v, 0) for v in seq]
    good = dw.dynamic(ll, dl, items, "none", trim=False)
    out = {}
    out["two-code incomplete distance table"] = (good, dw.dynamic(ll, dw.spread([1, 2], [0, 1], 30), items[:81], "none", trim=False))
    bad_ll = list(ll)
    bad_ll[259] = 0
    out["incomplete literal table"] = (good, dw.dynamic(bad_ll, dl, items[:82], "none", trim=False))
    out["HLIT = 30"] = (good, dw.dynamic(ll + [0], dl, items, "none", trim=False))
    out["repeat past HLIT + HDIST"] = (dw.dynamic(ll, dl, items, "none", trim=False, header_ops=plain[:-11] + [(18, 0)]),
                                       dw.dynamic(ll, dl, items, "none", trim=False, header_ops=plain[:-10] + [(18, 0)]))
    ll0 = [0, 0, 0] + ll[3:]
    out["repeat-16 first"] = (dw.dynamic(ll0, dl, items, "none", trim=False, header_ops=[(17, 0)] + plain[3:]),
                              dw.dynamic(ll0, dl, items, "none", trim=False, header_ops=[(16, 0)] + plain[3:]))
    no_eob = list(ll)
    no_eob[260], no_eob[256] = ll[256], 0
    out["no end-of-block length"] = (good, dw.dynamic(no_eob, dl, items, "none", trim=False))
    out["distance one past the output"] = (dw.fixed([97, 98, (3, 2)]), dw.fixed([97, (3, 2)]))
    return out


def test_near_misses_stay_rejected(tool, tmp_path):
    """One-field changes of valid members.  zlib refuses each; so must the decoder, with a status and no sanitizer report.
    (CPU only: invalid streams are never sent to the GPU by this suite's new modules.)"""
    src, dst = tmp_path / "m.gz", tmp_path / "m.out"
    for name, (good, bad) in _near_misses().items():
        raw, data = dw.deflate([good])
        assert _zlib_inflate(raw) == data, name
        src.write_bytes(dw.member(raw, data))
        r = _run(tool, "inflate", src, dst)
        assert r.returncode == 0 and dst.read_bytes() == data, (name, r.stdout)
        raw, data = dw.deflate([bad], check=False)
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(raw)
        src.write_bytes(dw.member(raw, data))
        r = _run(tool, "inflate", src, dst)
        assert r.returncode == 3 and r.stdout.startswith("status "), (name, r.returncode, r.stdout)
        assert "CRC32" not in r.stdout and "ISIZE" not in r.stdout, (name, r.stdout)  # refused as a stream, not by the footer


REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]


def _check_framing(tool, path, hb, recs, per_chunk):
    r = _run(tool, "bam", path, *([per_chunk] if per_chunk else []))
    assert r.returncode == 0, r.stdout[-500:]
    lines = r.stdout.splitlines()
    assert lines[0] == "header %d %d" % (hb, len(REFS))
    assert len(lines) - 1 == len(recs)
    for line, (_, tid, pos, flag, cigar) in zip(lines[1:], recs):
        kind, t, s, e, f = line.split()
        keep = not (flag & 4) and tid >= 0 and pos >= 0
        assert kind == ("keep" if keep else "skip") and int(t) == tid and int(f) == flag, line
        if keep:
            assert (int(s), int(e)) == (pos, min(synth.bam_end(pos, cigar), 0xFFFFFFFF)), line


@pytest.fixture(scope="module")
def long_reads():
    return synth.bam_long_read_records(400, seed=3, refs=REFS)


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
@pytest.mark.parametrize("headers", ["htslib", "foreign"])
def test_framing_of_long_read_files(tool, tmp_path, long_reads, layout, headers):
    """Records of one block, one block + 1, two blocks, 0.3 MB and 1 MB back to back in the middle of the file: the carry grows
    over many chunks of 1, 2 or 7 members."""
    path = tmp_path / "long.bam"
    header = synth.bam_header(REFS)
    if headers == "htslib":
        synth.write_bam(str(path), header, [r[0] for r in long_reads], layout=layout, level=1)
    else:
        path.write_bytes(dw.foreign_bam(header, [r[0] for r in long_reads], layout))
    for per in (None, 1, 2, 7):
        _check_framing(tool, path, len(header), long_reads, per)


def test_framing_of_a_file_ending_inside_a_long_record(tool, tmp_path, long_reads):
    sizes = [len(r[0]) for r in long_reads]
    second = next(i for i in range(1, len(sizes)) if sizes[i] == sizes[i - 1] == 1_000_000)  # of two 1 MB records in a row
    stream = synth.bam_header(REFS) + b"".join(r[0] for r in long_reads[:second + 1])
    cut = stream[:-400_000]
    path = tmp_path / "cut.bam"
    path.write_bytes(b"".join(synth.bgzf_member(cut[i:i + synth.BGZF_BLOCK], 1) for i in range(0, len(cut), synth.BGZF_BLOCK)) + synth.BGZF_EOF)
    for per in (None, 1, 7):
        r = _run(tool, "bam", path, *([per] if per else []))
        assert r.returncode == 3 and "unfinished record (600000 bytes)" in r.stdout, (per, r.stdout[-300:])


def test_framing_of_one_record_members_and_small_blocks(tool, tmp_path):
    """One record per member with the header in a member of its own; the spanning layout cut every 4096 bytes and the aligned one
    with 256-byte blocks, where most segments do not begin with a record."""
    recs = synth.bam_test_records(6000, seed=8, refs=REFS, big=False)
    header = synth.bam_header(REFS)
    path = tmp_path / "small.bam"
    path.write_bytes(b"".join(synth.bgzf_member(b, 1) for b in [header] + [r[0] for r in recs]) + synth.BGZF_EOF)
    for per in (None, 1, 2, 7):
        _check_framing(tool, path, len(header), recs, per)
    for layout, block in (("spanning", 4096), ("aligned", 256)):
        synth.write_bam(str(path), header, [r[0] for r in recs], layout=layout, level=1, block=block)
        for per in (None, 1, 2, 7):
            _check_framing(tool, path, len(header), recs, per)
