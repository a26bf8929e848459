"""The BGZF / DEFLATE / BAM-record decoder shared by the host and k_bgzf_inflate / k_bam_rows (device/bgzf_core.hpp), built
for the host under AddressSanitizer + UndefinedBehaviorSanitizer (tools/bgzf_check.cpp): equal to zlib on every level and
strategy, corrupt members rejected with a status and no sanitizer report, record framing and bam_endpos equal to a Python
restatement on both block layouts.  No GPU.  tests/test_deflate_streams_cpu.py adds the streams zlib's encoder does not write
(15-bit codes, libdeflate-style block headers) and the framing of long-read files."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from gffx_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "bgzf_check")


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "bgzf_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _corpora():
    rng = np.random.default_rng(7)
    words = [b"gene", b"exon", b"\t", b"ID=", b";", b"\n"] + [b"%d" % i for i in range(40)]
    return {"random": rng.integers(0, 256, 150000, dtype=np.uint8).tobytes(),
            "text": b"".join(words[i] for i in rng.integers(0, len(words), 30000)),
            "runs": b"".join(bytes([int(rng.integers(0, 3))]) * int(rng.integers(1, 500)) for _ in range(500))}


@pytest.mark.parametrize("level,strategy", [(0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FILTERED), (6, zlib.Z_HUFFMAN_ONLY),
                                            (6, zlib.Z_RLE), (6, zlib.Z_FIXED)])
def test_inflate_equals_zlib(tool, tmp_path, level, strategy):
    for name, data in _corpora().items():
        src, dst = tmp_path / (name + ".gz"), tmp_path / (name + ".out")
        pieces = [data[i:i + synth.BGZF_BLOCK] for i in range(0, len(data), synth.BGZF_BLOCK)]
        src.write_bytes(b"".join(synth.bgzf_member(p, level, strategy) for p in pieces) + synth.BGZF_EOF)
        r = _run(tool, "inflate", src, dst)
        assert r.returncode == 0, (name, r.stdout)
        assert dst.read_bytes() == data, name


def test_empty_member_and_isize_65536(tool, tmp_path):
    for data in (b"", b"ACGT" * 16384):
        src, dst = tmp_path / "a.gz", tmp_path / "a.out"
        src.write_bytes(synth.bgzf_member(data) + synth.bgzf_member(data, 1))
        assert _run(tool, "inflate", src, dst).returncode == 0
        assert dst.read_bytes() == data + data


def _member_with(raw: bytes, data_len: int, crc: int) -> bytes:
    total = 18 + len(raw) + 8
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + raw + struct.pack("<II", crc, data_len)


def test_corrupt_members_are_rejected_with_a_status(tool, tmp_path):
    data = b"the quick brown fox jumps over the lazy dog " * 40
    good = synth.bgzf_member(data)
    raw = good[18:-8]
    crc = zlib.crc32(data)
    cases = {
        "btype3": (_member_with(b"\x07" + raw[1:], len(data), crc), "block type 3"),
        # dynamic block, HCLEN 4: code-length code of four lengths 1,1,1,1 (over-subscribed)
        "codes": (_member_with(bytes([0x05, 0x00, 0x00, 0x49, 0x92, 0x24]) + b"\x00" * 8, len(data), crc), "Huffman code lengths"),
        # fixed block: literal 'a', then length 3 at distance 4 (only one byte written so far)
        "far": (_member_with(_fixed_block([("lit", ord("a")), ("match", 3, 4), ("eob",)]), 4, 0), "distance too far"),
        "isize": (_member_with(raw, len(data) + 1, crc), "ISIZE"),
        "crc": (_member_with(raw, len(data), crc ^ 1), "CRC32"),
        "bsize": (good[:16] + struct.pack("<H", 10) + good[18:], "BSIZE"),
    }
    for name, (blob, msg) in cases.items():
        src = tmp_path / (name + ".gz")
        src.write_bytes(blob)
        r = _run(tool, "inflate", src, tmp_path / "x.out")
        assert r.returncode == 3 and r.stdout.startswith("status "), (name, r.stdout)
        if msg:
            assert msg in r.stdout, (name, r.stdout)


def _fixed_block(items) -> bytes:
    """A final fixed-Huffman DEFLATE block from literal / match / end items (RFC 1951 §3.2.6)."""
    out, acc, n = bytearray(), 0, 0

    def put(v, k, msb=False):
        nonlocal acc, n
        if msb:
            v = int(format(v, "0%db" % k)[::-1], 2)
        acc |= v << n
        n += k

    def sym(s):
        if s < 144:
            put(0x30 + s, 8, True)
        elif s < 256:
            put(0x190 + s - 144, 9, True)
        elif s < 280:
            put(s - 256, 7, True)
        else:
            put(0xC0 + s - 280, 8, True)

    put(1, 1)
    put(1, 2)
    for it in items:
        if it[0] == "lit":
            sym(it[1])
        elif it[0] == "match":
            sym(257 + it[1] - 3)  # lengths 3..10 have no extra bits
            put(it[2] - 1, 5, True)  # distances 1..4 have no extra bits
        else:
            sym(256)
    while n > 0:
        out.append(acc & 0xFF)
        acc >>= 8
        n -= 8
    return bytes(out)


def test_truncation_at_every_byte_and_fuzzed_members(tool, tmp_path):
    src = tmp_path / "m.gz"
    src.write_bytes(synth.bgzf_member(_corpora()["text"][:3000], 6))
    r = _run(tool, "truncate", src)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout
    multi = tmp_path / "multi.gz"
    c = _corpora()
    multi.write_bytes(synth.bgzf_member(c["text"][:20000], 6) + synth.bgzf_member(c["runs"][:20000], 9, zlib.Z_RLE) +
                      synth.bgzf_member(c["random"][:3000], 0) + synth.bgzf_member(c["text"][:5000], 6, zlib.Z_FIXED))
    for seed in (1, 2):
        r = _run(tool, "fuzz", multi, 4000, seed)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout


REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]


@pytest.mark.parametrize("layout", ["aligned", "spanning"])
@pytest.mark.parametrize("per_chunk", [None, 1, 3])
@pytest.mark.parametrize("header_text", [0, 150000])
def test_framing_and_endpos_equal_the_restatement(tool, tmp_path, layout, per_chunk, header_text):
    """The device's framing (frame_guess on every member, frame_fix proving or walking the chain, the unfinished record
    carried from chunk to chunk) on chunks of 1, 3 or all members, with a header of one block or of three."""
    recs = synth.bam_test_records(1500, seed=9, refs=REFS, big=True)
    path = tmp_path / "x.bam"
    text = b"@CO\t" + b"x" * header_text
    hb = synth.write_bam(str(path), synth.bam_header(REFS, text), [r[0] for r in recs], layout=layout, flush_header=not header_text)
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


def test_malformed_records_are_rejected(tool, tmp_path):
    hdr = synth.bam_header(REFS)
    ok = synth.bam_record(0, 5, 0, [(0, 10)], b"a")
    bad = {"short": struct.pack("<i", 20) + b"\x00" * 20,
           "no_name": ok[:12] + b"\x00" + ok[13:],
           "cigar_beyond": ok[:16] + struct.pack("<H", 500) + ok[18:],
           "tid": ok[:4] + struct.pack("<i", 7) + ok[8:]}
    for name, rec in bad.items():
        path = tmp_path / (name + ".bam")
        synth.write_bam(str(path), hdr, [ok, rec, ok])
        r = _run(tool, "bam", path)
        assert r.returncode == 3 and "malformed" in r.stdout, (name, r.stdout)


def test_a_file_ending_inside_a_record_is_rejected(tool, tmp_path):
    stream = synth.bam_header(REFS) + b"".join(r[0] for r in synth.bam_test_records(300, seed=2, refs=REFS, big=False))
    cut = stream[:-10]
    path = tmp_path / "cut.bam"
    path.write_bytes(b"".join(synth.bgzf_member(cut[i:i + 20000]) for i in range(0, len(cut), 20000)) + synth.BGZF_EOF)
    for per in (None, 1, 2):
        r = _run(tool, "bam", path, *([per] if per else []))
        assert r.returncode == 3 and "unfinished record" in r.stdout, (per, r.stdout[-300:])


def test_file_front_end_on_whole_cut_and_unmarked_streams(tool, tmp_path):
    """host/bgzf_file.hpp, what bam.cpp and sam.cpp open a BGZF file with: the member directory, the EOF-marker test, the
    header inflated member by member until it is complete, and the runs of members fed per call -- on a stream whose header
    spans three members, cut at every member boundary, cut inside a member, and without the EOF member."""
    recs = synth.bam_test_records(300, seed=3, refs=REFS, big=False)
    path = tmp_path / "x.bam"
    hb = synth.write_bam(str(path), synth.bam_header(REFS, b"@CO\t" + b"x" * 150000), [r[0] for r in recs], flush_header=False)
    data = path.read_bytes()
    off, at = [], 0
    while at < len(data):
        off.append(at)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    off.append(len(data))
    n = len(off) - 1
    isize = [struct.unpack_from("<I", data, off[i + 1] - 4)[0] for i in range(n)]
    in_header = next(k for k in range(1, n + 1) if sum(isize[:k]) >= hb)  # members the header needs
    assert in_header == 3 and n >= 4

    def front(*args):
        r = _run(tool, "front", path, *args)
        return r.returncode, r.stdout.splitlines()

    rc, out = front()
    assert rc == 0 and out == ["members %d eof 1" % n, "header ok %d %d inflated %d" % (hb, len(REFS), sum(isize[:3])),
                               "chunks %d bytes %d" % (n, len(data))], out
    rc, out = front(len(data), len(data))  # one run takes all members
    assert rc == 0 and out[2] == "chunks 1 bytes %d" % len(data), out
    rc, out = front(len(data), off[2])  # the largest run that fits starts at member 0; every run is whole members
    assert rc == 0 and int(out[2].split()[1]) < n, out
    for k in range(n + 1):  # cut at every member boundary: sound members, a header that is complete or not
        rc, out = front(off[k])
        want = "header ok %d %d inflated %d" % (hb, len(REFS), sum(isize[:3])) if k >= 3 else "header truncated 0 0 inflated %d" % sum(isize[:k])
        assert rc == 0 and out == ["members %d eof %d" % (k, k == n), want, "chunks %d bytes %d" % (k, off[k])], (k, out)
    for k in range(n):  # cut inside a member: refused with the member's offset, read inside the bytes that are there
        for cut in {off[k] + 1, off[k] + 17, (off[k] + off[k + 1]) // 2, off[k + 1] - 1}:
            rc, out = front(cut)
            assert rc == 3 and out[0].startswith("status ") and out[0].endswith("offset %d" % off[k]), (k, cut, out)
    rc, out = front(off[n - 1])  # without the EOF member: the same members but the last, no marker
    assert rc == 0 and out[0] == "members %d eof 0" % (n - 1) and out[1].startswith("header ok"), out
