"""`gffx extract` without a GPU: the rules the kernels of device/ids.hip share with the host (device/ids_core.hpp: name hash,
compare and lookup, the bounded parent chase, the line slices and the keep test), built for the host under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/extract_check.cpp) and compared with the Python restatement (tests/_extract_oracle.py); and
what the command line decides before it asks for a device."""
import os
import shutil
import subprocess

import pytest

import _extract_oracle as xo
from _extract_cases import FILTER_LINES, FILTER_NAMES, FILTER_PRT, FILTER_REQUESTED, TYPE_CASES, edge_names, edge_queries
from gffx_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "extract_check")
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "extract_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def _lookup(tool, tmp_path, names, queries, hash_bits=None):
    """(slots, fids) of `extract_check lookup`, checked against the restatement on the way"""
    assert all(b"\n" not in n for n in names + queries)
    (tmp_path / "names.txt").write_bytes(b"".join(n + b"\n" for n in names))
    (tmp_path / "queries.txt").write_bytes(b"".join(q + b"\n" for q in queries))
    out = _run(tool, "lookup", tmp_path / "names.txt", tmp_path / "queries.txt", *([] if hash_bits is None else [hash_bits]))
    idx = xo.fts_index(names)
    got = [int(x) for x in out[1:]]
    assert got == [idx.get(q, -1) for q in queries]
    return int(out[0].split()[1]), got


def test_lookup_long_names_and_prefixes(tool, tmp_path):
    names = edge_names()
    queries = edge_queries(names)
    slots, got = _lookup(tool, tmp_path, names, queries)
    assert slots == 64 and got[:len(names)] == list(range(len(names)))
    idx = xo.fts_index(names)
    assert got[queries.index(b"gen")] == -1 and got[queries.index(b"gene")] == idx[b"gene"]  # a prefix that is / is not a name


def test_the_last_of_identical_names_wins(tool, tmp_path):
    _, got = _lookup(tool, tmp_path, [b"cds0"] * 1000, [b"cds0", b"cds", b"cds00"])
    assert got == [999, -1, -1]
    names = [b"id%d" % (i % 7) for i in range(50)]
    _, got = _lookup(tool, tmp_path, names, [b"id%d" % i for i in range(8)])
    assert got == [49, 43, 44, 45, 46, 47, 48, -1]


@pytest.mark.parametrize("hash_bits", [0, 3])
def test_every_name_on_few_probe_chains(tool, tmp_path, hash_bits):
    names = [b"feature%04d" % i for i in range(300)]
    names[17] = names[200] = b"twice"
    queries = names + [b"feature0300", b"feature", b""] + [b"miss%d" % i for i in range(50)] + [b"end"]
    slots, got = _lookup(tool, tmp_path, names, queries, hash_bits)
    assert slots == 1024 and got[17] == 200 and got[0] == 0 and got[299] == 299
    assert got == _lookup(tool, tmp_path, names, queries)[1]  # the hook changes no result


def test_a_table_of_exactly_a_power_of_two(tool, tmp_path):
    names = [b"n%d" % i for i in range(4096)]
    slots, _ = _lookup(tool, tmp_path, names, names[::37] + [b"n4096", b"n"])
    assert slots == 8192
    assert _lookup(tool, tmp_path, [b"one"], [b"one", b"on"])[0] == 2
    assert _lookup(tool, tmp_path, [b"a", b"b"], [b"b", b"a", b"c"])[0] == 4


def test_parent_chase(tool, tmp_path):
    # fids 0..50: a chain of depth 50 under root 0; 51: a root of its own; 52 -> 51; 53: parent >= n; 54 -> 53;
    # 55 <-> 56: a 2-cycle; 57 -> 58 -> 59 -> 57: a 3-cycle; 60 -> 57 runs into it
    prt = [0] + list(range(50)) + [51, 51, 1000, 53, 56, 55, 58, 59, 57, 57]
    n = len(prt)
    fids = list(range(n)) + [n, n + 1, 2**32 - 1]
    (tmp_path / "prt.txt").write_text("".join("%d\n" % p for p in prt))
    (tmp_path / "fids.txt").write_text("".join("%d\n" % f for f in fids))
    out = _run(tool, "chase", tmp_path / "prt.txt", tmp_path / "fids.txt")
    got = [int(ln.split()[0]) for ln in out]
    want = [xo.resolve_root(prt, f) for f in fids]
    assert got == [-1 if w == xo.NONE else w for w in want]
    assert got[:51] == [0] * 51 and got[51] == 51 and got[52] == 51  # depth 0, 1 and 50
    assert got[53] == -1 and got[54] == -1                            # a parent >= n, reached directly and through a child
    assert got[55:61] == [-1] * 6                                     # the cycles come back invalid (within n steps: the run ended)
    assert got[61:] == [-1, -1, -1]                                   # a fid >= n


@pytest.mark.parametrize("types", TYPE_CASES)
def test_line_filter(tool, tmp_path, types):
    for root, keep_ids in ((0, {"b", "x"}), (4, {"other", "dup"})):
        (tmp_path / "text.gff").write_bytes(b"".join(l for l, _ in FILTER_LINES))
        (tmp_path / "names.txt").write_bytes(b"".join(n + b"\n" for n in FILTER_NAMES))
        (tmp_path / "prt.txt").write_text("".join("%d\n" % p for p in FILTER_PRT))
        (tmp_path / "queries.txt").write_bytes(b"".join(q + b"\n" for q in FILTER_REQUESTED))
        extra = [] if types is None else ["-T", types]
        got = [int(x) for x in _run(tool, "filter", tmp_path / "text.gff", tmp_path / "names.txt", tmp_path / "prt.txt",
                                    tmp_path / "queries.txt", root, *extra)]
        allow = xo.split_types(types)
        assert got == [int(xo.keeps_line(l, keep_ids, allow)) for l, _ in FILTER_LINES], (types, root)
        if types is None and root == 0:
            assert got == [k for _, k in FILTER_LINES]
        if types == ",":
            assert not any(got)  # -T given, nothing allowed
        if types == " exon , CDS,,\t" and root == 0:
            assert sum(got) == sum(k for _, k in FILTER_LINES) - 2  # less the `gene` and the ` exon` line


# ---- the command line ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indexed(tmp_path_factory, golden_dir):
    d = tmp_path_factory.mktemp("extract_cli")
    gff = str(d / "t.gff")
    shutil.copy(os.path.join(golden_dir, "appendix_e.gff"), gff)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True).returncode == 0
    (d / "names.txt").write_text("e1\n")
    return gff, str(d / "names.txt")


def test_exactly_one_of_feature_id_and_feature_file(indexed):
    gff, names = indexed
    r = subprocess.run([GFFX, "extract", "-i", gff], capture_output=True)
    assert r.returncode == 2 and b"--feature-file <FEATURE_FILE>|--feature-id <FEATURE_ID>" in r.stderr and b"Usage: gffx extract" in r.stderr
    r = subprocess.run([GFFX, "extract", "-i", gff, "-f", "e1", "-F", names], capture_output=True)
    assert r.returncode == 2 and b"cannot be used with" in r.stderr
    r = subprocess.run([GFFX, "extract", "-f", "e1"], capture_output=True)
    assert r.returncode == 2 and b"--input <FILE>" in r.stderr
    r = subprocess.run([GFFX, "extract", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--feature-file" in r.stdout and b"--entire_group" in r.stdout
    assert b"extract" in subprocess.run([GFFX, "help"], capture_output=True).stdout


def test_a_missing_index_file_is_named(indexed, tmp_path):
    gff = str(tmp_path / "t.gff")
    shutil.copy(indexed[0], gff)
    for ext in (".gof", ".prt", ".sqs", ".atn", ".a2f", ".rit", ".rix"):
        shutil.copy(indexed[0] + ext, gff + ext)
    r = subprocess.run([GFFX, "extract", "-i", gff, "-f", "e1"], capture_output=True)
    assert r.returncode == 1 and b'Missing index file(s): [".fts"]' in r.stderr and r.stdout == b""


def test_damaged_side_cars_and_name_lists_are_refused_on_the_host(indexed, tmp_path):
    gff = str(tmp_path / "t.gff")
    for ext in ("", ".gof", ".fts", ".prt", ".sqs", ".atn", ".a2f", ".rit", ".rix"):
        shutil.copy(indexed[0] + ext, gff + ext)
    with open(gff + ".prt", "ab") as f:
        f.write(b"\x00")
    r = subprocess.run([GFFX, "extract", "-i", gff, "-f", "e1"], capture_output=True)
    assert r.returncode == 1 and r.stderr == b"Error: Corrupted PRT: not aligned to u32\n"
    shutil.copy(indexed[0] + ".prt", gff + ".prt")
    with open(gff + ".fts", "ab") as f:
        f.write(b"\xff\xfe\n")
    r = subprocess.run([GFFX, "extract", "-i", gff, "-f", "e1"], capture_output=True)
    assert r.returncode == 1 and b"FTS contains invalid UTF-8 at byte" in r.stderr
    shutil.copy(indexed[0] + ".fts", gff + ".fts")
    (tmp_path / "bad.txt").write_bytes(b"e1\n\xff\n")
    r = subprocess.run([GFFX, "extract", "-i", gff, "-F", str(tmp_path / "bad.txt")], capture_output=True)
    assert r.returncode == 1 and b"valid UTF-8" in r.stderr
    r = subprocess.run([GFFX, "extract", "-i", gff, "-F", str(tmp_path / "no_such_list.txt")], capture_output=True)
    assert r.returncode == 1 and b"Cannot open feature list" in r.stderr


@pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
def test_no_cpu_fallback_without_a_gpu(indexed):
    for extra in ([], ["-e"], ["-T", "exon"]):
        r = subprocess.run([GFFX, "extract", "-i", indexed[0], "-f", "e1"] + extra, capture_output=True)
        assert r.returncode == 1 and b"no HIP device" in r.stderr and r.stdout == b"", r.stderr
