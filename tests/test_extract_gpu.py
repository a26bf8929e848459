"""`gffx extract` on the GPU: the ID table, the lookup with the parent chase and the line filter of device/ids.hip through
engine.FeatureIds, and the command's output bytes, all equal to the Python restatement (tests/_extract_oracle.py).  No test
here feeds a parent cycle: the bound of the chase is checked on the host (tests/test_extract_cpu.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _extract_oracle as xo
import _index_cases as ic
from _extract_cases import (FILTER_LINES, FILTER_NAMES, FILTER_PRT, FILTER_REQUESTED, REUSE_SIZES, TYPE_CASES, edge_names, edge_queries,
                            refused_chunks)
from gffx_amd import _ffi, engine, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
NONE = xo.NONE


def forest(n, seed, bad=0):
    """parent words without a cycle: every parent is the fid itself (a root) or a smaller fid; `bad` of them are >= n"""
    rng = np.random.Generator(np.random.PCG64(seed))
    prt = np.arange(n, dtype=np.int64)
    child = rng.random(n) < 0.8
    child[0] = False
    prt[child] = (rng.random(int(child.sum())) * np.flatnonzero(child)).astype(np.int64)
    if bad:
        prt[rng.choice(n, size=bad, replace=False)] = n + rng.integers(0, 5, size=bad)
    return prt.astype(np.uint32)


def roots_of(prt):
    """prt.rs:54-72 for every fid of such a forest, in one ascending pass (a parent's root is known before its children's)"""
    n = len(prt)
    root = np.full(n, NONE, dtype=np.uint32)
    for f, p in enumerate(prt.tolist()):
        root[f] = f if p == f else (NONE if p >= n else root[p])
    return root


def expect(names, prt, queries):
    idx = xo.fts_index(names)
    root = roots_of(prt)
    fids = np.array([idx.get(q, NONE) for q in queries], dtype=np.uint32).reshape(-1)
    roots = np.array([NONE if f == NONE or f >= len(prt) else root[f] for f in fids.tolist()], dtype=np.uint32).reshape(-1)
    return fids, roots


def check_resolve(names, prt, queries, hash_bits=None):
    want_f, want_r = expect(names, prt, queries)
    ids = engine.FeatureIds.from_arrays(names, prt, hash_bits=hash_bits)
    try:
        assert ids.n == len(names)
        assert ids.options() == ({} if hash_bits is None else {"hash_bits": hash_bits})
        got_f, got_r = ids.resolve(queries)
        assert np.array_equal(got_f, want_f) and np.array_equal(got_r, want_r)
        assert np.array_equal(ids.requested_fids(), np.unique(want_f[want_f != NONE]))
        assert np.array_equal(ids.unique_roots(), np.unique(want_r[want_r != NONE]))
    finally:
        ids.close()
    return want_f, want_r


def test_roots_of_is_the_restated_chase():
    prt = forest(3000, seed=3, bad=40)
    root = roots_of(prt)
    assert [xo.resolve_root(prt.tolist(), f) for f in range(0, 3000, 7)] == root[::7].tolist()
    assert (root == NONE).sum() >= 40 and (root != NONE).sum() > 1000


@pytest.mark.parametrize("n", [1, 2, 4096])
def test_resolve_small_tables(n):
    names = [b"n%d" % i for i in range(n)]
    prt = forest(n, seed=n)
    queries = names + [b"n", b"n%d" % n, b"", b"N0"] + names[::-1] + names[:3] * 2
    f, _ = check_resolve(names, prt, queries)
    assert f[:n].tolist() == list(range(n)) and f[n:n + 4].tolist() == [NONE] * 4
    check_resolve(names, prt, [])  # nq = 0


def test_resolve_long_names_and_prefixes():
    names = edge_names()
    prt = forest(len(names), seed=5)
    f, _ = check_resolve(names, prt, edge_queries(names))
    assert f[:len(names)].tolist() == list(range(len(names)))


@pytest.fixture(scope="module")
def big():
    n = 100_003
    rng = np.random.Generator(np.random.PCG64(21))
    names = [b"transcript:ENST%011d.%d" % (i * 7919 % 10**9, i % 13) for i in range(n)]
    for i in rng.choice(n, size=n // 10, replace=False).tolist():  # 10 % of the lines re-use another line's ID (CDS rows)
        names[i] = names[int(rng.integers(0, n))]
    prt = forest(n, seed=22, bad=500)
    pick = rng.integers(0, n, size=200_000)
    queries = [names[i] for i in pick.tolist()]
    for i in range(0, 200_000, 9):  # misses, some of them prefixes of stored names
        queries[i] = queries[i][:-1] if i % 2 else b"missing%d" % i
    return names, prt, queries


def test_resolve_100003_names_200000_queries(big):
    names, prt, queries = big
    f, r = check_resolve(names, prt, queries)
    assert (f == NONE).sum() > 10_000 and ((f != NONE) & (r == NONE)).sum() > 100  # misses, and parents >= n
    assert len(set(names)) < len(names) - 5000


def test_two_builds_of_a_table_give_identical_results(big):
    names, prt, queries = big
    out = []
    for _ in range(2):
        ids = engine.FeatureIds.from_arrays(names, prt)
        out.append(ids.resolve(queries[:50_000]) + (ids.requested_fids(), ids.unique_roots()))
        ids.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("hash_bits,n", [(0, 300), (3, 5000)])
def test_every_name_on_few_probe_chains(hash_bits, n):
    names = [b"feature%05d" % i for i in range(n)]
    names[17] = names[n - 100] = b"twice"
    prt = forest(n, seed=n)
    queries = names + [b"feature", b"feature%05d" % n, b""] + [b"miss%d" % i for i in range(200)]
    f, _ = check_resolve(names, prt, queries, hash_bits=hash_bits)
    assert f[17] == n - 100
    check_resolve(names, prt, queries)


def test_bitmaps_accumulate_until_reset():
    names = [b"id%d" % i for i in range(1000)]
    prt = forest(1000, seed=8, bad=20)
    root = roots_of(prt)
    ids = engine.FeatureIds.from_arrays(names, prt)
    a, b = list(range(0, 400)), list(range(300, 900, 3))
    ids.resolve([names[i] for i in a] + [b"nope"])
    assert np.array_equal(ids.requested_fids(), np.array(a, dtype=np.uint32))
    ids.resolve([names[i] for i in b])
    both = np.unique(np.array(a + b, dtype=np.uint32))
    assert np.array_equal(ids.requested_fids(), both)
    want_roots = np.unique(root[both])
    assert np.array_equal(ids.unique_roots(), want_roots[want_roots != NONE])
    ids.reset()
    assert len(ids.requested_fids()) == 0 and len(ids.unique_roots()) == 0
    ids.resolve([names[5]])
    assert ids.requested_fids().tolist() == [5]
    ids.close()


def test_invalid_parents_and_more_parent_words_than_names():
    names = [b"a", b"b", b"c", b"d"]
    prt = np.array([0, 0, 9, 2, 4, 4], dtype=np.uint32)  # c's parent is >= n; d hangs under c; two more words than names
    ids = engine.FeatureIds.from_arrays(names, prt)
    f, r = ids.resolve([b"d", b"c", b"b", b"a", b"e"])
    assert f.tolist() == [3, 2, 1, 0, NONE] and r.tolist() == [NONE, NONE, 0, 0, NONE]
    assert ids.unique_roots().tolist() == [0] and ids.requested_fids().tolist() == [0, 1, 2, 3]
    ids.close()
    ids = engine.FeatureIds.from_arrays(names, np.array([0, 0], dtype=np.uint32))  # fewer words than names: fids 2, 3 are >= n
    assert ids.resolve(names)[1].tolist() == [0, 0, NONE, NONE]
    ids.close()


# ---- the line filter ----------------------------------------------------------------------------------------------------
def offsets(lines):
    return np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64)


@pytest.fixture(scope="module")
def filter_ids():
    ids = engine.FeatureIds.from_arrays(FILTER_NAMES, FILTER_PRT)
    ids.resolve(FILTER_REQUESTED)
    yield ids
    ids.close()


KEEP_OF_ROOT = {0: {"b", "x"}, 4: {"other", "dup"}}


def allowed(types):
    a = xo.split_types(types)
    return None if a is None else sorted(a)


@pytest.mark.parametrize("types", TYPE_CASES)
def test_line_classes(filter_ids, types):
    lines = [l for l, _ in FILTER_LINES]
    text = b"".join(lines)
    for root, keep_ids in KEEP_OF_ROOT.items():
        got = filter_ids.filter_lines(text, offsets(lines), [root] * len(lines), allowed(types))
        assert got.tolist() == [int(xo.keeps_line(l, keep_ids, xo.split_types(types))) for l in lines], (types, root)
        if types is None and root == 0:
            assert got.tolist() == [k for _, k in FILTER_LINES]
    # the two blocks' lines in one call, alternating
    both = lines[:-1] * 2 + lines[-1:]
    roots = [(0, 4)[i % 2] for i in range(len(both))]
    got = filter_ids.filter_lines(b"".join(both), offsets(both), roots, allowed(types))
    assert got.tolist() == [int(xo.keeps_line(l, KEEP_OF_ROOT[r], xo.split_types(types))) for l, r in zip(both, roots)]


def test_chunks_that_end_exactly_at_a_line_end(filter_ids):
    lines = [l for l, _ in FILTER_LINES]
    whole = [k for _, k in FILTER_LINES]
    assert filter_ids.filter_lines(b"", offsets([]), []).tolist() == []
    for cut in range(1, len(lines)):
        got = []
        for part in (lines[:cut], lines[cut:]):
            got += filter_ids.filter_lines(b"".join(part), offsets(part), [0] * len(part)).tolist()
        assert got == whole, cut


def test_one_line_of_a_megabyte(filter_ids):
    nine = b"c\ts\texon\t1\t2\t.\t+\t.\t"
    long_note = b"Note=" + b"A" * (1 << 20)
    lines = [nine + long_note + b";ID=x\n", nine + b"ID=" + b"x" * (1 << 20) + b"\n", nine + b"ID=b;" + long_note + b"\n",
             b"c\ts\t" + b"T" * (1 << 20) + b"\t1\t2\t.\t+\t.\tID=b\n"]
    got = filter_ids.filter_lines(b"".join(lines), offsets(lines), [0] * 4)
    assert got.tolist() == [1, 0, 1, 1] == [int(xo.keeps_line(l, KEEP_OF_ROOT[0], None)) for l in lines]
    assert filter_ids.filter_lines(b"".join(lines), offsets(lines), [0] * 4, ["exon"]).tolist() == [1, 0, 1, 0]


def test_filter_lines_refusals_on_a_live_handle(filter_ids):
    for rc, message, want in refused_chunks(_ffi.lib().gffx_hip_ids_filter_lines, "gffx_hip_ids_filter_lines", filter_ids._h):
        assert rc == -1 and message == want
    lines = [l for l, _ in FILTER_LINES]
    assert filter_ids.filter_lines(b"".join(lines), offsets(lines), [0] * len(lines)).tolist() == [k for _, k in FILTER_LINES]


def test_a_handle_filters_chunks_of_65_1_0_and_65_lines():
    ids = engine.FeatureIds.from_arrays(FILTER_NAMES, FILTER_PRT)
    ids.resolve(FILTER_REQUESTED)
    pool = [l for l, _ in FILTER_LINES][:-1] * 4  # (without the line that has no newline)
    for n in REUSE_SIZES:
        lines, roots = pool[:n], [(0, 4)[i % 2] for i in range(n)]
        got = ids.filter_lines(b"".join(lines), offsets(lines), roots)
        assert got.tolist() == [int(xo.keeps_line(l, KEEP_OF_ROOT[r], None)) for l, r in zip(lines, roots)], n
        assert n != 65 or 0 < got.sum() < n
    ids.close()


@pytest.mark.parametrize("hash_bits", [-1, 0, 2])
def test_the_last_row_of_an_id_and_the_first_row_of_a_value(hash_bits):
    """the same 258 strings, two insert blocks, with the pairs (0, 256) and (255, 257) equal: as IDs the LAST row of a string
    is its fid (the table keeps the largest), as attribute values they are numbered by their FIRST row (it keeps the smallest)"""
    k = 1
    names = ["s%03d" % i for i in range(256 + k + 1)]
    names[256], names[256 + k] = names[0], names[255]
    ids = engine.FeatureIds.from_arrays(names, np.arange(len(names), dtype=np.uint32), hash_bits=None if hash_bits < 0 else hash_bits)
    fids, _ = ids.resolve(names)
    ids.close()
    idx = xo.fts_index([n.encode() for n in names])
    assert fids.tolist() == [idx[n.encode()] for n in names] and fids[0] == 256 and fids[255] == 256 + k and fids[1] == 1
    text = b"".join(ic.gene_line(i, id_=n, name=n) + b"\n" for i, n in enumerate(names))
    kind, want = ic.oracle_outcome(text, "gene_name", ic.DEFAULT_SKIP)
    assert kind == "ok" and want.a2f[256] == 0 and want.a2f[256 + k] == 255 and len(want.atn) == 256 and want.fid[0] == 256
    g = engine.gff_index(text, "gene_name", ic.DEFAULT_SKIP, hash_bits=hash_bits)
    try:
        assert g.built().astuple() == ic.built_tuple(want)
    finally:
        g.close()


# ---- the command --------------------------------------------------------------------------------------------------------
def run_cli(gff, names=None, feature_id=None, entire_group=False, types=None, env=None, extra=()):
    cmd = [GFFX, "extract", "-i", gff] + (["-F", names] if names else ["-f", feature_id])
    if entire_group:
        cmd.append("-e")
    if types is not None:
        cmd += ["-T", types]
    return subprocess.run(cmd + list(extra), capture_output=True, env=env)


def warned(stderr, missing):
    """the names that were not found are reported once, in the order of their first appearance -- or not at all"""
    lines = [ln for ln in stderr.split(b"\n") if b"feature IDs not found" in ln]
    return lines == ([b"[WARN] %d feature IDs not found: %s" % (len(missing), xo.rust_debug_list(missing).encode())] if missing else [])


def test_appendix_e_known_answers_through_the_cli(tmp_path, golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "appendix_e_extract.json")))
    gff = str(tmp_path / "t.gff")
    shutil.copy(os.path.join(golden_dir, fx["gff"]), gff)
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    data = open(gff, "rb").read()
    by_key = {k: l + b"\n" for k, l in zip(fx["line_order"], data.split(b"\n")[:-1])}
    for case in fx["cases"]:
        a = case["args"]
        lst = None
        if "feature_list" in a:
            lst = str(tmp_path / "names.txt")
            open(lst, "w").write("".join(n + "\n" for n in a["feature_list"]))
        r = run_cli(gff, lst, a.get("feature_id"), bool(a.get("entire_group")), a.get("types"))
        assert r.returncode == case["exit"], (case, r.stderr)
        assert r.stdout == b"".join(by_key[k] for k in case["stdout"]), case
        assert warned(r.stderr, case["missing"]), (case, r.stderr)


TYPES = (None, "exon", "gene, CDS,,nonexistent")


@pytest.fixture(scope="module", params=[(31, False), (32, True)], ids=["plain", "crlf"])
def synth_gff(request, tmp_path_factory):
    seed, crlf = request.param
    d = tmp_path_factory.mktemp("extract_synth")
    gff = str(d / "s.gff")
    synth.write_gff3(gff, synth.gencode_like_roots(400, seed=seed, chroms=synth.SMALL2), seed=seed, quirks=True, crlf=crlf)
    assert subprocess.run([GFFX, "index", "-i", gff]).returncode == 0
    data = open(gff, "rb").read()
    B = xo.build_index(data)
    reused = sorted({i for i in B.ids if B.ids.count(i) > 1 and i.startswith("gene")})
    multi = [i for i in B.ids if i.startswith("multi")]
    orphan = [i for i in B.ids if i.startswith("orphan")]
    assert reused and multi and orphan
    return d, gff, data, B, [reused[0], multi[0], orphan[0]]


def name_list(B, special, k, seed):
    uniq = list(dict.fromkeys(B.ids))
    if k is None:
        picked = uniq
    else:
        rng = np.random.Generator(np.random.PCG64(seed))
        picked = [uniq[i] for i in rng.choice(len(uniq), size=k, replace=False).tolist()]
    return special + ["no_such_id", "gene", "gene000001x"] + picked


def write_list(path, names):
    # as a user's file: a blank line, blanks around a name, a name twice, CRLF on one line
    rows = [names[0], "", "  " + names[1] + "\t"] + names[2:] + [names[0], names[-1] + "\r"]
    open(path, "wb").write("".join(r + "\n" for r in rows).encode())


def check_all_flags(gff, data, B, names, lst, env=None):
    for eg in (False, True):
        for types in TYPES:
            want, missing, invalid = xo.extract_run(data, B, list(dict.fromkeys(names)), eg, types)
            assert not invalid
            r = run_cli(gff, lst, None, eg, types, env=env)
            assert r.returncode == 0, r.stderr
            assert r.stdout == want, (eg, types, len(r.stdout), len(want))
            assert warned(r.stderr, missing), r.stderr


@pytest.mark.parametrize("k", [1, 50, None], ids=["1", "50", "all"])
def test_all_flag_combinations_equal_the_restatement(synth_gff, k):
    d, gff, data, B, special = synth_gff
    names = name_list(B, special, k, seed=7)
    lst = str(d / ("names_%s.txt" % k))
    write_list(lst, names)
    check_all_flags(gff, data, B, names, lst)
    want, _, _ = xo.extract_run(data, B, list(dict.fromkeys(names)), False, None)
    assert len(want) > 0


def test_without_the_all_line_image_and_in_small_chunks(synth_gff, tmp_path):
    d, gff0, data, B, special = synth_gff
    gff = str(tmp_path / "s.gff")
    for ext in ("", ".gof", ".fts", ".prt", ".sqs", ".atn", ".a2f", ".rit", ".rix"):  # (no .lall, no .lsoa)
        shutil.copy(gff0 + ext, gff + ext)
    names = name_list(B, special, 50, seed=9)
    lst = str(tmp_path / "names.txt")
    write_list(lst, names)
    check_all_flags(gff, data, B, names, lst)
    r = run_cli(gff, lst, None, False, None, extra=["-v"])
    assert r.returncode == 0 and b"line boundaries from the text" in r.stderr
    # chunks of one line each (boundaries from the image), and chunks that end exactly where the first kept line ends (from the text)
    want, _, _ = xo.extract_run(data, B, list(dict.fromkeys(names)), False, None)
    first = len(want.split(b"\n")[0]) + 1
    for budget, g in ((1, gff0), (first, gff)):
        r = run_cli(g, lst, None, False, None, env=dict(os.environ, GFFX_EXTRACT_CHUNK_BYTES=str(budget)))
        assert r.returncode == 0 and r.stdout == want, budget


def test_single_ids_an_output_file_and_the_stats(synth_gff, tmp_path):
    d, gff, data, B, special = synth_gff
    for fid, eg in [(special[0], True)] + [(f, False) for f in special + ["no_such_id"]]:
        want, missing, _ = xo.extract_run(data, B, [fid], eg, None)
        r = run_cli(gff, None, fid, eg, None)
        assert r.returncode == 0 and r.stdout == want and warned(r.stderr, missing), fid
    stats = str(tmp_path / "stats.json")
    out = str(tmp_path / "out.gff")
    r = run_cli(gff, None, special[0], False, None, extra=["-o", out, "--stats-json", stats])
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == xo.extract_run(data, B, [special[0]], False, None)[0]
    js = json.load(open(stats))
    assert js["command"] == "extract" and js["counts"]["names"] == 1 and js["counts"]["unique_roots"] == 1


def test_a_line_longer_than_a_chunk(tmp_path):
    """a GFF whose second line is a megabyte long, filtered in chunks of 4 KiB"""
    big = (b"c\ts\tgene\t1\t9\t.\t+\t.\tID=g1\n" b"c\ts\tmRNA\t1\t9\t.\t+\t.\tID=t1;Parent=g1;Note=" + b"A" * (1 << 20) + b"\n"
           b"c\ts\texon\t1\t3\t.\t+\t.\tID=e1;Parent=t1\n")
    p = str(tmp_path / "big.gff")
    open(p, "wb").write(big)
    assert subprocess.run([GFFX, "index", "-i", p]).returncode == 0
    Bb = xo.build_index(big)
    for names in (["t1"], ["e1", "t1"], ["g1"]):
        lst = str(tmp_path / "n.txt")
        open(lst, "w").write("".join(n + "\n" for n in names))
        r = run_cli(p, lst, None, False, None, env=dict(os.environ, GFFX_EXTRACT_CHUNK_BYTES="4096"))
        assert r.returncode == 0 and r.stdout == xo.extract_run(big, Bb, names, False, None)[0], names


def test_from_files_reads_the_index_the_command_reads(synth_gff):
    d, gff, data, B, special = synth_gff
    ids = engine.FeatureIds.from_files(gff)
    assert ids.n == len(B.ids)
    uniq = list(dict.fromkeys(B.ids))
    f, r = ids.resolve(uniq + ["no_such_id"])
    idx = xo.fts_index(B.ids)
    assert f.tolist() == [idx[u] for u in uniq] + [NONE]
    assert r.tolist() == [xo.resolve_root(B.prt, idx[u]) for u in uniq] + [NONE]
    ids.close()
