"""k_bgzf_inflate on valid streams that zlib's encoder does not write (tests/_deflate_writer.py; the same corpus as
tests/test_deflate_streams_cpu.py, where zlib's inflate vouches for the writer): the device build of bgzf_core.hpp, the LDS
staging and the wave CRC must give the writer's bytes, byte for byte.  Output sizes at the CRC stripe edges, other writers' gzip
member headers, and a BAM file whose blocks were compressed by the writer.  Valid streams only."""
import os
import subprocess

import numpy as np
import pytest

import _deflate_writer as dw
from gffx_amd import engine, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
REFS = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]
REF_SEQ = [0, 0xFFFFFFFF, 1]  # chrU is not in the index


@pytest.fixture(scope="module")
def corpus():
    return dw.corpus()


def _first_difference(got, want, names, sizes):
    """Which member's output differs first (for the message)."""
    at = 0
    for name, n in zip(names, sizes):
        if got[at:at + n] != want[at:at + n]:
            return name
        at += n
    return "length %d != %d" % (len(got), len(want))


def test_directed_streams_inflate_to_the_writers_bytes(corpus):
    directed = [c for c in corpus if not c[0].startswith("random")]
    assert len(directed) == len(dw.directed_cases())
    want = b"".join(d for _, _, d, _ in directed)
    got = engine.bgzf_inflate(b"".join(m for _, m, _, _ in directed) + synth.BGZF_EOF)
    assert got == want, _first_difference(got, want, [c[0] for c in directed], [len(c[2]) for c in directed])


def test_random_streams_inflate_to_the_writers_bytes(corpus):
    rnd = [c for c in corpus if c[0].startswith("random")]
    assert len(rnd) >= 300
    want = b"".join(d for _, _, d, _ in rnd)
    got = engine.bgzf_inflate(b"".join(m for _, m, _, _ in rnd) + synth.BGZF_EOF)  # one launch, hundreds of different members
    assert got == want, _first_difference(got, want, [c[0] for c in rnd], [len(c[2]) for c in rnd])


def test_output_sizes_at_the_crc_stripe_edges():
    """Lane i checks bytes [i * S, (i + 1) * S) with S = ceil(n / 64): a wrong stripe bound is a CRC failure of a valid member."""
    edges = dw.stripe_edge_members()
    assert sorted({len(d) for _, _, d in edges}) == sorted(dw.STRIPE_SIZES) and len(edges) == 3 * len(dw.STRIPE_SIZES)
    want = b"".join(d for _, _, d in edges)
    got = engine.bgzf_inflate(b"".join(m for _, m, _ in edges))
    assert got == want, _first_difference(got, want, [e[0] for e in edges], [len(e[2]) for e in edges])


def test_member_header_variants():
    data = [b"member %d of another writer; " % i * (20 + i) for i in range(len(dw.HEADER_VARIANTS))]
    members = [dw.member(dw.deflate(dw.compress(d, i))[0], d, **v) for i, (d, v) in enumerate(zip(data, dw.HEADER_VARIANTS.values()))]
    blob = b"".join(members) + synth.BGZF_EOF
    assert engine.bgzf_members(blob) == list(np.cumsum([0] + [len(m) for m in members])) + [len(blob)]
    assert engine.bgzf_inflate(blob) == b"".join(data)


def _table(data, head):
    lines = data.split(b"\n")
    assert lines[0] == head and lines[-1] == b""
    return sorted(lines[1:-1])


def test_a_bam_file_compressed_by_the_writer(tmp_path):
    recs = synth.bam_test_records(400, seed=3, refs=REFS, big=False)
    header = synth.bam_header(REFS)
    want = synth.bam_rows_definition(recs, REF_SEQ)
    roots = synth.gencode_like_roots(300, seed=1, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=1)
    assert subprocess.run([GFFX, "index", "-i", gff], timeout=300).returncode == 0
    bed = str(tmp_path / "same.bed")
    synth.write_bed(bed, want, [n for n, _ in synth.SMALL2])
    want_tsv = str(tmp_path / "want.tsv")
    rc, msg = ob.depth_run(gff, bed, want_tsv)
    assert rc == 0, msg
    head = b"id\tchr\tstart\tend\tdepth"
    want_rows = _table(open(want_tsv, "rb").read(), head)
    assert len(want_rows) > 10
    for layout, block in (("aligned", synth.BGZF_BLOCK), ("spanning", 9000)):
        data = dw.foreign_bam(header, [r[0] for r in recs], layout, block, seed=7, deflater=dw.compress)
        for chunk in (0, 1):
            got = engine.bam_rows(data, REF_SEQ, len(header), chunk)
            assert got.shape == want.shape and np.array_equal(got, want), (layout, chunk)
        path = str(tmp_path / ("w_%s.bam" % layout))
        open(path, "wb").write(data)
        out = str(tmp_path / "got.tsv")
        r = subprocess.run([GFFX, "depth", "-i", gff, "-s", path, "-o", out], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert _table(open(out, "rb").read(), head) == want_rows, layout
