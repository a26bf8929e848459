"""`gffx enrich` end to end on the hand-written GFF of tests/_annotate_definition.py and a hand-written BED
(tests/_enrich_definition.py): with -g lengths that force every placement the table and the --perms file are the hand-written
bytes; with the default lengths they are the definition's -- --perms byte for byte, the table's integer columns byte for byte
and its floats to what %.6g keeps --, from q.bed, from q.bed.gz (bgzipped: the device reader), with GFFX_BED_DEVICE=1, with
chunks of 200 bytes, with -t 1 and -t 16; another seed gives another --perms file; usage errors exit 2."""
import os
import subprocess

import numpy as np
import pytest

import _annotate_definition as ad
import _enrich_definition as ed
from gffx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
KNOBS = ("GFFX_BED_DEVICE", "GFFX_BED_CHUNK_BYTES", "GFFX_CHUNK_BYTES", "GFFX_CHUNK_MB", "GFFX_LINE_TABLE")
TIMEOUT = 120
TYPES = ",".join(ad.LAYER_NAMES)
DEFAULT_LEN = [700, 20]  # the largest end of a line of chrA and of chrB in ad.GFF


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    d = tmp_path_factory.mktemp("enrich_cli")
    gff = str(d / "hand.gff")
    open(gff, "w").write(ad.GFF)
    r = subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr
    bed = str(d / "q.bed")
    open(bed, "wb").write(ed.BED)
    open(bed + ".gz", "wb").write(b"".join(synth.bgzf_member(ed.BED[i:i + 40]) for i in range(0, len(ed.BED), 40)) + synth.BGZF_EOF)
    genome = str(d / "genome.txt")
    open(genome, "wb").write(ed.GENOME)
    return dict(dir=d, gff=gff, bed=bed, genome=genome, n=0)


def _run(inp, args, knobs=None, bed=None, out=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs or {})
    inp["n"] += 1
    perms = str(inp["dir"] / ("perms%d.tsv" % inp["n"]))
    cmd = [GFFX, "enrich", "-i", inp["gff"], "-b", bed or inp["bed"], "-T", TYPES, "--perms", perms] + list(args) + (["-o", out] if out else [])
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=TIMEOUT)
    errors = [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")]
    warns = [ln for ln in r.stderr.splitlines() if ln.startswith(b"[WARN]")]
    table = open(out, "rb").read() if out and os.path.exists(out) else r.stdout
    return r.returncode, errors, warns, table, open(perms, "rb").read() if os.path.exists(perms) else None


def test_the_hand_written_bytes_with_forced_placements(inp):
    for seed in ("0", "987654321"):
        rc, errors, warns, table, perms = _run(inp, ["-n", "2", "-g", inp["genome"], "--seed", seed])
        assert (rc, errors) == (0, []) and table == ed.BY_HAND_TABLE and perms == ed.BY_HAND_PERMS
        assert len(warns) == 1 and warns[0].startswith(b"[WARN] 2 regions are wider than their seqid's length")


def test_the_definition_on_every_route(inp):
    B, R, unplaced = ed.totals(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, DEFAULT_LEN, ed.HAND_REGIONS, 20, 5)
    assert unplaced == 2 and len({tuple(r) for r in B[1:].tolist()}) > 1  # chrA's regions do move now
    want_perms = ed.perms_text(B, R)
    routes = [([], None, None), ([], None, inp["bed"] + ".gz"), ([], {"GFFX_BED_DEVICE": "1"}, None), ([], {"GFFX_CHUNK_BYTES": "200"}, None),
              ([], {"GFFX_CHUNK_BYTES": "1"}, None), ([], {"GFFX_CHUNK_BYTES": "12"}, inp["bed"] + ".gz"), (["-t", "1"], None, None), (["-t", "16"], {"GFFX_LINE_TABLE": "parse"}, None)]
    tables = set()
    for extra, knobs, bed in routes:
        rc, errors, warns, table, perms = _run(inp, ["-n", "20", "--seed", "5"] + extra, knobs, bed)
        assert (rc, errors) == (0, []) and perms == want_perms, (extra, knobs, bed)
        assert ed.table_matches(table, ad.LAYER_NAMES, B, R)
        assert len(warns) == 1 and b"no -g" in warns[0]
        tables.add(table)
    assert len(tables) == 1  # the same bytes on every route
    out = str(inp["dir"] / "out.tsv")
    assert _run(inp, ["-n", "20", "--seed", "5"], out=out)[3] == next(iter(tables))
    # -n 1: sd and z are nan
    B1, R1, _ = ed.totals(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, DEFAULT_LEN, ed.HAND_REGIONS, 1, 5)
    rc, errors, _, table, perms = _run(inp, ["-n", "1", "--seed", "5"])
    assert (rc, errors) == (0, []) and perms == ed.perms_text(B1, R1) and ed.table_matches(table, ad.LAYER_NAMES, B1, R1)
    assert all(ln.split(b"\t")[4:6] == [b"nan", b"nan"] for ln in table.splitlines()[1:])
    assert np.array_equal(B1, B[:2])


def test_g_against_the_default_lengths(inp):
    genome = str(inp["dir"] / "default.txt")
    open(genome, "wb").write(b"chrA\t700\nchrB\t20\n")
    a = _run(inp, ["-n", "20", "--seed", "5", "-g", genome])
    b = _run(inp, ["-n", "20", "--seed", "5"])
    assert a[0] == b[0] == 0 and a[3] == b[3] and a[4] == b[4]
    longer = str(inp["dir"] / "longer.txt")
    open(longer, "wb").write(b"chrA\t5000\nchrB\t100\n")
    B, R, unplaced = ed.totals(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, [5000, 100], ed.HAND_REGIONS, 20, 5)
    rc, errors, warns, table, perms = _run(inp, ["-n", "20", "--seed", "5", "-g", longer])
    assert (rc, errors, warns) == (0, [], []) and unplaced == 0 and perms == ed.perms_text(B, R) and perms != b[4]
    assert ed.table_matches(table, ad.LAYER_NAMES, B, R)


def test_another_seed_gives_another_perms_file(inp):
    a = _run(inp, ["-n", "20", "--seed", "5"])
    b = _run(inp, ["-n", "20", "--seed", "6"])
    c = _run(inp, ["-n", "20"])  # the default seed is 0
    B, R, _ = ed.totals(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, DEFAULT_LEN, ed.HAND_REGIONS, 20, 0)
    assert a[0] == b[0] == c[0] == 0 and a[4] != b[4] and c[4] == ed.perms_text(B, R) and c[4] != a[4]
    assert a[4].split(b"\n")[0] == b[4].split(b"\n")[0]  # the observed row does not depend on the seed


def test_usage_errors_and_their_exit_status(inp):
    def usage(args, what):
        r = subprocess.run([GFFX, "enrich", "-i", inp["gff"]] + args, capture_output=True, timeout=TIMEOUT)
        assert r.returncode == 2 and what in r.stderr and b"Usage: gffx enrich" in r.stderr and r.stdout == b"", r.stderr

    usage(["-b", inp["bed"], "-T", TYPES], b"--permutations <N>")
    usage(["-b", inp["bed"], "-T", TYPES, "-n", "0"], b"1 to 1048576 are possible")
    usage(["-b", inp["bed"], "-n", "5"], b"--types <T1,T2,...>")
    usage(["-T", TYPES, "-n", "5"], b"--bed <BED>")
    usage(["-b", inp["bed"], "-T", TYPES, "-n", "5", "-r", "chrA:1-5"], b"-r")
    rc, errors, _, _, _ = _run(inp, ["-n", "5", "-g", str(inp["dir"] / "missing.txt")])
    assert rc == 1 and len(errors) == 1 and b"Cannot open genome file" in errors[0]
    rc, errors, _, _, _ = _run(inp, ["-n", "5"], bed=str(inp["dir"] / "missing.bed"))
    assert rc == 1 and len(errors) == 1
