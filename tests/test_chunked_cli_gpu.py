"""`gffx intersect` and `gffx depth` with chunks and batches of a few rows (GFFX_CHUNK_BYTES, GFFX_DEPTH_BATCH_ROWS): the second
chunk's code -- GFFX_OUT_BITMAP_KEEP, the reuse of a ring slot and of a staging buffer, devices whose share of a chunk is
empty, the keep_all store Join B reads, the finish(1 - k) overlap and the round robin of `depth` -- with a chunk boundary after
every few rows of a 3000-row file.  Output == the oracle's and == the run with the knob unset, for every size and --gpus N
(logical devices beyond the visible ones share a GPU).  Every run is a fresh process."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from gffx_amd import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
CHUNK, BATCH = "GFFX_CHUNK_BYTES", "GFFX_DEPTH_BATCH_ROWS"
NAMES = [n for n, _ in synth.SMALL2]
TIMEOUT = 120  # seconds per CLI run (one takes well under a second once HIP is up)


def _run(cmd, knobs=None):
    env = {k: v for k, v in os.environ.items() if k not in (CHUNK, BATCH, "GFFX_CHUNK_MB")}
    env.update(knobs or {})
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    assert r.returncode == 0, (cmd, knobs, r.stderr[-600:])
    return r


def _index(gff):
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT).returncode == 0


def _bed_text(rows, junk=True, crlf=False):
    """BED text of the rows; junk: a comment first and in the middle, a row on an unknown seqid, a row of two fields.  The last
    line has no line ending."""
    lines = ["%s\t%d\t%d" % (NAMES[c], s, e) for c, s, e in rows.tolist()]
    if junk:
        lines.insert(2 * len(lines) // 3, "# a comment in the middle")
        lines.insert(len(lines) // 2, "chr1\t7")
        lines.insert(len(lines) // 3, "chrUn\t1\t2")
        lines.insert(0, "# header")
    return ("\r\n" if crlf else "\n").join(lines).encode()


def _chunks(text, chunk_bytes):
    """The chunks `gffx intersect` cuts: chunk_bytes, then on to the end of the line."""
    n, pos = 0, 0
    while True:
        z = min(len(text), pos + chunk_bytes)
        if z < len(text):
            nl = text.find(b"\n", z)
            z = len(text) if nl < 0 else nl + 1
        n, pos = n + 1, z
        if pos >= len(text):
            return n


# ------------------------------------------------------------------------------------------------------------- intersect
FLAG_SETS = {"e": (["-e"], dict(mode=2, entire_group=True)), "c": (["-c"], dict(mode=0)),
             "CI": (["-C", "-I"], dict(mode=1, invert=True)), "OT": (["-O", "-T", "exon,gene"], dict(mode=2, types="exon,gene"))}


@pytest.fixture(scope="module")
def intersect_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunked_intersect")
    roots = synth.gencode_like_roots(400, seed=13, chroms=synth.SMALL2)
    gff = str(d / "s.gff")
    synth.write_gff3(gff, roots, seed=13, quirks=True)
    _index(gff)
    rows = synth.synth_bed(3000, seed=14, chroms=synth.SMALL2, width=(20, 40000), edge_frac=0.25, roots=roots)
    bed, bed_crlf = str(d / "q.bed"), str(d / "q_crlf.bed")
    open(bed, "wb").write(_bed_text(rows))
    open(bed_crlf, "wb").write(_bed_text(rows[:600], crlf=True))
    return dict(dir=d, gff=gff, bed=bed, bed_crlf=bed_crlf, roots=roots)


def _intersect(inp, bed, flags, gpus, chunk_bytes, tag):
    out, sj = str(inp["dir"] / ("got_%s.gff" % tag)), str(inp["dir"] / ("stats_%s.json" % tag))
    _run([GFFX, "intersect", "-i", inp["gff"], "-b", bed, "-o", out, "--gpus", str(gpus), "--stats-json", sj] + flags,
         None if chunk_bytes is None else {CHUNK: str(chunk_bytes)})
    return open(out, "rb").read(), json.load(open(sj))


def _oracle_intersect(inp, bed, kw, tag):
    want = str(inp["dir"] / ("want_%s.gff" % tag))
    rc, msg = ob.intersect_run(inp["gff"], want, bed=bed, **kw)
    assert rc == 0, msg
    return open(want, "rb").read()


@pytest.mark.parametrize("name", list(FLAG_SETS))
def test_intersect_bytes_do_not_depend_on_the_chunk_size(intersect_inputs, name):
    """64 bytes: two or three rows per chunk and some with none (a comment, the short row), ~375 reuses of every slot, and with
    three devices at least one without a row in every chunk (the shard plan is made per chunk, over position buckets);
    997 and 4096: a boundary at no special place."""
    inp, (flags, kw) = intersect_inputs, FLAG_SETS[name]
    want = _oracle_intersect(inp, inp["bed"], kw, name)
    assert len(want) > 0
    base = {}
    for gpus in (1, 3):
        for chunk_bytes in (None, 64, 997, 4096):
            got, st = _intersect(inp, inp["bed"], flags, gpus, chunk_bytes, name)
            assert got == want, (name, gpus, chunk_bytes)
            dev = st["devices"]
            assert len(dev) == gpus == st["counts"]["gpus"]
            sums = (st["counts"]["regions"], sum(d["regions"] for d in dev), sum(d["kept_pairs"] for d in dev))
            if chunk_bytes is None:
                base[gpus] = sums
                assert sums[0] == sums[1] == 3000 and sums[2] > 0
            assert sums == base[gpus] == base[1], (name, gpus, chunk_bytes)


def test_intersect_crlf_bed_in_small_chunks(intersect_inputs):
    inp = intersect_inputs
    flags, kw = FLAG_SETS["e"]
    want = _oracle_intersect(inp, inp["bed_crlf"], kw, "crlf")
    assert len(want) > 0
    for gpus in (1, 3):
        for chunk_bytes in (None, 64, 997):
            got, st = _intersect(inp, inp["bed_crlf"], flags, gpus, chunk_bytes, "crlf")
            assert got == want and st["counts"]["regions"] == 600, (gpus, chunk_bytes)


def test_intersect_wide_rows_in_small_chunks(tmp_path):
    """The 700 wide + 150 narrow rows of test_cli_gpu.py's wide-form test, 2048 bytes at a time: every chunk's sample decides for
    its own rows."""
    roots = synth.gencode_like_roots(3000, seed=21, chroms=synth.SMALL2)
    gff = str(tmp_path / "w.gff")
    synth.write_gff3(gff, roots, seed=21)
    _index(gff)
    rows = np.concatenate([synth.synth_bed(700, seed=22, chroms=synth.SMALL2, width=(20000, 600000)),
                           synth.synth_bed(150, seed=23, chroms=synth.SMALL2, width=(1, 3000), edge_frac=0.3, roots=roots)])
    rows = rows[np.random.default_rng(5).permutation(len(rows))]
    text = _bed_text(rows, junk=False)
    bed = str(tmp_path / "wide.bed")
    open(bed, "wb").write(text)
    n_chunks = _chunks(text, 2048)
    assert n_chunks >= 8
    inp = dict(dir=tmp_path, gff=gff)
    for name in ("e", "c"):
        flags, kw = FLAG_SETS[name]
        want = _oracle_intersect(inp, bed, kw, name)
        got, st = _intersect(inp, bed, flags, 1, 2048, name)
        assert got == want and len(want) > 0, name
        assert st["counts"]["regions"] == len(rows)
        if name == "e":  # (overlap mode; four rows in five are wide, so more than one chunk is mostly wide: the knob took effect)
            assert 2 <= st["counts"]["wide_form_passes"] <= n_chunks, (st["counts"], n_chunks)


@pytest.mark.parametrize("value", ["0", "-5", "12x", ""], ids=["zero", "negative", "trailing_x", "empty"])
def test_a_garbage_chunk_size_is_ignored(intersect_inputs, value):
    inp = intersect_inputs
    flags, kw = FLAG_SETS["c"]
    want, st_want = _intersect(inp, inp["bed"], flags, 1, None, "plain")
    out, sj = str(inp["dir"] / "got_garbage.gff"), str(inp["dir"] / "stats_garbage.json")
    _run([GFFX, "intersect", "-i", inp["gff"], "-b", inp["bed"], "-o", out, "--stats-json", sj] + flags, {CHUNK: value})
    st = json.load(open(sj))
    assert open(out, "rb").read() == want and len(want) > 0
    assert st["counts"] == st_want["counts"] and st["devices"] == st_want["devices"] and st["knobs"] == st_want["knobs"]


# ------------------------------------------------------------------------------------------------------------- depth
def _rows(data):
    lines = data.split(b"\n")
    assert lines[0] == b"id\tchr\tstart\tend\tdepth" and lines[-1] == b""
    return sorted(lines[1:-1])


@pytest.fixture(scope="module")
def depth_inputs(tmp_path_factory):
    """The inputs of test_depth_gpu.py::test_depth_cli_rows_equal_the_oracle (its seed 2: a GFF with quirks), 4000 rows; and the
    first 150 of them."""
    d = tmp_path_factory.mktemp("chunked_depth")
    seed = 2
    roots = synth.gencode_like_roots(300, seed=seed, chroms=synth.SMALL2)
    gff = str(d / "s.gff")
    synth.write_gff3(gff, roots, seed=seed, quirks=True)
    _index(gff)
    regions = synth.synth_bed(4000, seed=seed + 10, chroms=synth.SMALL2, width=(1, 60000), edge_frac=0.1, roots=roots)
    junk = ["# header\n", "chrZ\t1\t2\n", "chr1\t7\n", "\n", "chr1 5 9 name\n", "chr1\t3\tx\n"]
    out = dict(dir=d, gff=gff, roots=roots)
    for key, n in (("all", 4000), ("150", 150)):
        bed, want = str(d / ("q%s.bed" % key)), str(d / ("want%s.tsv" % key))
        synth.write_bed(bed, regions[:n], NAMES, extra_lines=junk)
        rc, msg = ob.depth_run(gff, bed, want)
        assert rc == 0, msg
        out[key] = (bed, _rows(open(want, "rb").read()), open(_depth(out, bed, 1, None)[0], "rb").read())
        assert len(out[key][1]) > 20
    return out


def _depth(inp, source, gpus, batch_rows, verbose=False):
    out = str(inp["dir"] / "got.tsv")
    r = _run([GFFX, "depth", "-i", inp["gff"], "-s", source, "-o", out, "--gpus", str(gpus)] + (["-v"] if verbose else []),
             None if batch_rows is None else {BATCH: str(batch_rows)})
    return out, r.stderr


@pytest.mark.parametrize("batch_rows", [None, 1, 7, 200])
def test_depth_rows_do_not_depend_on_the_batch_size(depth_inputs, batch_rows):
    """1 row per batch (150 rows): every batch is a ring-slot reuse; 7 and 200: hundreds and tens of batches, dealt round robin
    to 1, 2 and 3 devices, each waiting for its batch i - 1 while batch i runs."""
    bed, want_rows, unset = depth_inputs["150" if batch_rows == 1 else "all"]
    assert _rows(unset) == want_rows
    for gpus in (1, 2, 3):
        out, err = _depth(depth_inputs, bed, gpus, batch_rows, verbose=True)
        got = open(out, "rb").read()
        assert _rows(got) == want_rows, (batch_rows, gpus)
        assert _rows(got) == _rows(unset)
        if gpus > 1:
            per_dev = [int(x) for x in re.findall(rb"\[INFO\] device \d+: (\d+) BED rows", err)]
            kept = int(re.search(rb"\[INFO\] (\d+) BED rows kept", err).group(1))
            assert len(per_dev) == gpus and sum(per_dev) == kept
            if batch_rows == 200:
                assert gpus == 2 or min(per_dev) >= 5 * 200, per_dev  # three devices: at least five batches each
            elif batch_rows is None:
                assert per_dev[0] == kept  # (one batch)


def test_depth_bam_source_in_small_batches_on_two_devices(tmp_path):
    refs = [("chr1", 3_000_000), ("chrU", 1000), ("chr2", 2_000_000)]
    roots = synth.gencode_like_roots(300, seed=1, chroms=synth.SMALL2)
    gff = str(tmp_path / "s.gff")
    synth.write_gff3(gff, roots, seed=1)
    _index(gff)
    recs = synth.bam_test_records(3000, seed=5, refs=refs, big=True)
    bam = str(tmp_path / "x.bam")
    synth.write_bam(bam, synth.bam_header(refs), [r[0] for r in recs], layout="spanning")
    rows = synth.bam_rows_definition(recs, [0, 0xFFFFFFFF, 1])  # chrU is not in the index
    bed = str(tmp_path / "same.bed")
    synth.write_bed(bed, rows, NAMES)
    want = str(tmp_path / "want.tsv")
    rc, msg = ob.depth_run(gff, bed, want)
    assert rc == 0, msg
    want_rows = _rows(open(want, "rb").read())
    assert len(want_rows) > 10
    inp = dict(dir=tmp_path, gff=gff)
    for batch_rows in (None, 300):
        out, _ = _depth(inp, bam, 2, batch_rows)
        assert _rows(open(out, "rb").read()) == want_rows, batch_rows


@pytest.mark.parametrize("value", ["0", "-5", "12x", ""], ids=["zero", "negative", "trailing_x", "empty"])
def test_a_garbage_batch_size_is_ignored(depth_inputs, value):
    bed, want_rows, unset = depth_inputs["all"]
    out, _ = _depth(depth_inputs, bed, 1, value)
    got = open(out, "rb").read()
    assert got == unset and _rows(got) == want_rows
