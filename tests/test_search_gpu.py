"""`gffx search` on the GPU: the exact and the DFA match of every `.atn` value, the fid / root resolution with the (class, root)
pair set and the value filter of device/search.hip through engine.AttrSearch, and the command's output bytes, all equal to the
Python restatement (tests/_search_oracle.py; Python's re.search is the regex oracle).  No test here feeds a parent cycle: the
bound of the chase is checked on the host (tests/test_extract_cpu.py)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _search_cases as sc
import _search_oracle as so
from _extract_cases import REUSE_SIZES, refused_chunks
from gffx_amd import _ffi, engine, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
NONE = so.NONE


def matched(values, wanted, **kw):
    a = engine.AttrSearch.from_arrays(values, [], [], **kw)
    try:
        a.match(wanted)
        return a.matched_aids().tolist()
    finally:
        a.close()


# ---- exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4096])
def test_exact_small_tables(n):
    values = ["G%d" % i for i in range(n)]
    wanted = values[::3] + ["G", "G%d" % n, "", "g0"] + values[:2]
    want = so.match_aids(values, wanted, False)
    assert matched(values, wanted) == want and len(want) == len(values[::3]) + (1 if n > 1 else 0)
    assert matched(values, []) == []                        # an empty list
    assert matched(values, ["nope", "G", "G0x"]) == []      # all miss, prefixes and extensions of stored values among them
    assert matched(values, values) == list(range(n))


@pytest.mark.parametrize("hash_bits", [0, 3])
def test_exact_on_few_probe_chains_with_duplicates(hash_bits):
    values = ["name%04d" % (i % 200) for i in range(700)]  # every string three or four times
    wanted = ["name0007", "name0199", "name0200", "name", "name0007"]
    want = so.match_aids(values, wanted, False)
    assert len(want) == 4 + 3
    a = engine.AttrSearch.from_arrays(values, [], [], hash_bits=hash_bits)
    assert a.options() == {"hash_bits": hash_bits}
    a.match(wanted)
    assert a.matched_aids().tolist() == want
    a.match(["name0001"])  # matches accumulate until reset
    assert a.matched_aids().tolist() == sorted(want + so.match_aids(values, ["name0001"], False))
    a.reset()
    assert a.matched_aids().tolist() == []
    a.close()


def test_one_value_of_a_megabyte():
    big = "A" * (1 << 20)
    values = ["x", big, big[:-1], "y", big]
    assert matched(values, [big]) == [1, 4]
    assert matched(values, [big[:-1], "y"]) == [2, 3]
    a = engine.AttrSearch.from_arrays(values, [], [])
    assert a.match_regex(engine.compile_regex(["^A{255}A*$"])) == ["k_attr_match_dfa<lds>"]
    assert a.matched_aids().tolist() == [1, 2, 4]
    a.close()


# ---- DFA ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """the corpus of tests/test_search_cpu.py, every pattern of it: (patterns, values, want[pattern][value], the DFA of every
    pattern compiled alone under a cap none of them reaches)"""
    pats, values = sc.corpus()
    want = [[bool(re.search(p, v)) for v in values] for p in pats]
    dfas = [engine.compile_regex([p], 65535) for p in pats]
    return pats, values, want, dfas


@pytest.mark.parametrize("path", [None, "lds", "global"])
def test_dfa_corpus_against_re_search(corpus, path):
    pats, values, want, dfas = corpus
    a = engine.AttrSearch.from_arrays(values, [], [], dfa_path=path)
    assert a.options() == ({} if path is None else {"dfa_path": path})
    # pattern by pattern, every one; a table beyond the LDS budget takes the global path (and is refused when LDS is forced)
    beyond = 0
    for p, w, c in zip(pats, want, dfas):
        g = c.groups[0]
        fits = 256 + 2 * g["n_states"] * g["n_classes"] <= 65536
        a.reset()
        if path == "lds" and not fits:
            beyond += 1
            with pytest.raises(engine._ffi.GffxHipError):
                a.match_regex(c)
            continue
        assert a.match_regex(c) == ["k_attr_match_dfa<%s>" % ("global" if path == "global" or not fits else "lds")]
        assert a.matched_aids().tolist() == [i for i, m in enumerate(w) if m], p
    assert path != "lds" or beyond < len(pats) // 10
    # ... and twenty at a time as one alternation under the default cap; a pattern too large for it alone leaves the list
    small = []
    for p in pats:
        try:
            engine.compile_regex([p]).close()
            small.append(True)
        except engine.RegexError as e:
            assert "regex too large" in str(e)
            small.append(False)
    assert sum(small) > len(pats) * 0.9
    for k in range(0, len(pats), 20):
        idx = [j for j in range(k, min(k + 20, len(pats))) if small[j]]
        c = engine.compile_regex([pats[j] for j in idx])
        a.reset()
        names = a.match_regex(c)
        assert names == ["k_attr_match_dfa<%s>" % (path or "lds")] * len(c.groups)
        assert a.matched_aids().tolist() == [i for i in range(len(values)) if any(want[j][i] for j in idx)], k
    a.close()


def test_a_table_beyond_the_lds_budget_takes_the_global_path(corpus):
    values = corpus[1]
    p = "[^a]{255}|(ab?){2,3}c"  # 4-byte scalars make it ~ 2000 states: far beyond 64 KiB, compiled under a cap of its own
    c = engine.compile_regex([p], 65535)
    g = c.groups[0]
    assert 256 + 2 * g["n_states"] * g["n_classes"] > 65536
    values = values + ["b" * 255, "😀" * 255, "b" * 254 + "a", "é" * 254]
    a = engine.AttrSearch.from_arrays(values, [], [])
    assert a.match_regex(c) == ["k_attr_match_dfa<global>"]
    assert a.matched_aids().tolist() == so.match_aids(values, [p], True)
    assert len(values) - 4 in a.matched_aids().tolist() and len(values) - 3 in a.matched_aids().tolist()
    a.close()
    a = engine.AttrSearch.from_arrays(values, [], [], dfa_path="lds")  # forced into LDS it is refused, not cut short
    with pytest.raises(engine._ffi.GffxHipError):
        a.match_regex(c)
    a.close()


@pytest.mark.parametrize("cap,groups", [(4096, 1), (4, 2), (3, 3)])
def test_caps_that_force_groups(cap, groups):
    pats = ["ab", "cd", "e", "fg"]
    values = ["ab", "xcdx", "e", "fg", "a", "b", "", "gf", "abcd", "éab", "af"]
    c = engine.compile_regex(pats, cap)
    assert len(c.groups) == groups
    assert [g["first_pattern"] for g in c.groups] == {1: [0], 2: [0, 3], 3: [0, 1, 3]}[groups]
    a = engine.AttrSearch.from_arrays(values, [], [])
    a.match_regex(c)
    assert a.matched_aids().tolist() == so.match_aids(values, pats, True)
    a.close()


@pytest.mark.parametrize("pattern", ["^", "$", "", "^$", "$^"])
def test_anchors_alone_and_the_empty_pattern(pattern):
    values = ["", "a", "é", "ab" * 40]
    a = engine.AttrSearch.from_arrays(values, [], [])
    a.match_regex(engine.compile_regex([pattern]))
    assert a.matched_aids().tolist() == so.match_aids(values, [pattern], True)
    a.close()


# ---- resolve and filter -------------------------------------------------------------------------------------------------------
def forest(n, seed, bad=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    prt = np.arange(n, dtype=np.int64)
    child = rng.random(n) < 0.8
    child[0] = False
    prt[child] = (rng.random(int(child.sum())) * np.flatnonzero(child)).astype(np.int64)
    if bad:
        prt[rng.choice(n, size=bad, replace=False)] = n + rng.integers(0, 5, size=bad)
    return prt.astype(np.uint32)


@pytest.mark.parametrize("n_fid,n_prt", [(3000, 3000), (3000, 2900), (2900, 3000)])
def test_the_four_bitmaps_against_the_oracle(n_fid, n_prt):
    rng = np.random.Generator(np.random.PCG64(n_fid + n_prt))
    values = ["G%d" % (i % 350) for i in range(400)]  # 50 strings twice
    a2f = rng.integers(0, 420, size=n_fid).astype(np.uint32)  # aids >= the value count among them
    a2f[rng.random(n_fid) < 0.3] = NONE
    a2f[a2f == 7] = 8  # aid 7 is carried by no fid
    prt = forest(n_prt, seed=5, bad=60)  # parents >= n; with n_prt < n_fid also fids >= n
    wanted = ["G%d" % i for i in range(0, 350, 5)] + ["G7", "nope"]
    S = so.steps(values, a2f.tolist(), prt.tolist(), wanted, False)
    assert S.bail is None and S.invalid and 7 in S.no_fid_aids
    a = engine.AttrSearch.from_arrays(values, a2f, prt)
    a.match(wanted)
    a.resolve()
    assert a.matched_aids().tolist() == S.aids
    assert a.matched_fids().tolist() == S.fids
    assert a.unique_roots().tolist() == S.roots
    assert a.invalid_fids().tolist() == S.invalid
    a.resolve()  # a second resolve starts from empty results
    assert a.matched_fids().tolist() == S.fids and a.unique_roots().tolist() == S.roots
    a.reset()
    a.resolve()
    assert a.matched_fids().tolist() == [] and a.unique_roots().tolist() == []
    a.close()


def offsets(lines):
    return np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.uint64)


@pytest.fixture(scope="module")
def filter_attrs():
    # aids: 0 TP53, 1 BRCA1, 2 TP53 (a repeated string), 3 EGFR.  fids 0..5; roots 0 and 4 (5's parent is out of range)
    values = ["TP53", "BRCA1", "TP53", "EGFR"]
    a2f = [NONE, 2, 1, NONE, 1, 0]
    prt = [0, 0, 1, 0, 4, 99]
    a = engine.AttrSearch.from_arrays(values, a2f, prt, key="gene_name")
    yield a, values, a2f, prt
    a.close()


@pytest.mark.parametrize("types", [None, "exon", " exon , gene,,", ","])
@pytest.mark.parametrize("wanted", [["TP53"], ["TP53", "BRCA1"], ["BRCA1"]])
def test_line_classes(filter_attrs, types, wanted):
    a, values, a2f, prt = filter_attrs
    a.reset()
    a.match(wanted)
    a.resolve()
    S = so.steps(values, a2f, prt, wanted, False)
    lines = [l for l, _ in sc.VALUE_LINES]
    allow = so.xo.split_types(types)
    for root in (0, 4, 1, NONE):
        got = a.filter_lines(b"".join(lines), offsets(lines), [root] * len(lines), None if allow is None else sorted(allow))
        keep = S.per_root.get(root, set())
        assert got.tolist() == [int(so.xo.keeps_line(l, keep, allow, b"gene_name")) for l in lines], (root, types, wanted)
        if wanted == ["TP53"] and root == 0 and types is None:
            assert got.tolist() == [k for _, k in sc.VALUE_LINES]  # fid 1 carries aid 2, the second TP53: the string keys the set
    assert a.filter_lines(b"", offsets([]), []).tolist() == []


def test_filter_lines_refusals_on_a_live_handle(filter_attrs):
    a, values, a2f, prt = filter_attrs
    for rc, message, want in refused_chunks(_ffi.lib().gffx_hip_attrs_filter_lines, "gffx_hip_attrs_filter_lines", a._h):
        assert rc == -1 and message == want
    a.reset()
    a.match(["TP53"])
    a.resolve()
    lines = [l for l, _ in sc.VALUE_LINES]
    assert a.filter_lines(b"".join(lines), offsets(lines), [0] * len(lines)).tolist() == [k for _, k in sc.VALUE_LINES]


@pytest.mark.parametrize("hash_bits", [None, 0])
def test_a_handle_reused_across_sizes(hash_bits):
    """257 values (two insert blocks, aids 255 and 256 the same string); a wanted table of 1024 slots, then one of 2; chunks of
    65, 1, 0 and 65 lines"""
    values = ["V%03d" % i for i in range(257)]
    values[256] = values[255]
    a2f = list(range(257))
    prt = [f - f % 2 for f in range(257)]  # fid 2 k + 1 hangs under the root 2 k
    a = engine.AttrSearch.from_arrays(values, a2f, prt, hash_bits=hash_bits)
    many = values[0:256:2] + [values[255]] + ["W%d" % i for i in range(171)]
    one = [values[1]]
    assert len(many) == 300 and one[0] not in many
    a.match(many)
    assert a.matched_aids().tolist() == so.match_aids(values, many, False) and a.matched_aids().tolist()[-2:] == [255, 256]
    a.reset()
    a.match(one)
    assert a.matched_aids().tolist() == so.match_aids(values, one, False) == [1]
    a.match([values[255]])
    a.resolve()
    S = so.steps(values, a2f, prt, one + [values[255]], False)
    assert sorted(S.per_root) == [0, 254, 256]
    pool = [sc.NINE + b"ID=e%d;gene_name=%s\n" % (i, values[(1, 255, 2)[i % 3]].encode()) for i in range(65)]
    for n in REUSE_SIZES:
        lines, roots = pool[:n], [(0, 254, 256, 2)[i % 4] for i in range(n)]
        got = a.filter_lines(b"".join(lines), offsets(lines), roots)
        assert got.tolist() == [int(so.xo.keeps_line(l, S.per_root.get(r, set()), None, b"gene_name")) for l, r in zip(lines, roots)], n
        assert n != 65 or 0 < got.sum() < n
    a.close()


# ---- the command ----------------------------------------------------------------------------------------------------------------
def run_cli(gff, attr=None, attr_list=None, regex=False, entire_group=False, types=None, env=None, extra=()):
    cmd = [GFFX, "search", "-i", gff] + (["-A", attr_list] if attr_list else ["-a", attr])
    cmd += (["-r"] if regex else []) + (["-e"] if entire_group else []) + ([] if types is None else ["-T", types])
    return subprocess.run(cmd + list(extra), capture_output=True, env=env)


@pytest.fixture(scope="module")
def synth_gff(tmp_path_factory):
    d = tmp_path_factory.mktemp("search_synth")
    gff = str(d / "s.gff")
    synth.write_gff3(gff, synth.gencode_like_roots(300, seed=41, chroms=synth.SMALL2), seed=41, quirks=True)
    assert subprocess.run([GFFX, "index", "-i", gff, "-a", "gene_name"]).returncode == 0
    data = open(gff, "rb").read()
    B = so.build_index(data)
    name, values = so.load_atn(open(gff + ".atn", "rb").read())
    a2f = so.load_a2f(open(gff + ".a2f", "rb").read())
    assert name == "gene_name" and values == B.atn and a2f == B.a2f
    return d, gff, data, B, values, a2f


FLAGS = [(False, None), (True, None), (False, "exon,CDS"), (True, "gene")]


def check(gff, data, B, values, a2f, patterns, regex, attr=None, attr_list=None, env=None):
    for eg, types in FLAGS:
        want, S = so.search_run(data, B.gof, "gene_name", values, a2f, B.prt, patterns, regex, eg, types)
        assert S.bail is None
        r = run_cli(gff, attr, attr_list, regex, eg, types, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (patterns[:3], regex, eg, types, len(r.stdout), len(want))
    return want


def test_all_flag_combinations_equal_the_restatement(synth_gff):
    d, gff, data, B, values, a2f = synth_gff
    one = values[len(values) // 2]
    assert len(check(gff, data, B, values, a2f, [one], False, attr=one)) >= 0
    rx = "^%s.$" % one[:-1]
    assert so.match_aids(values, [rx], True)
    check(gff, data, B, values, a2f, [rx], True, attr=rx)
    lst = str(d / "list.txt")
    picks = values[::7] + ["nope", values[3]]
    open(lst, "wb").write(("\n  %s\t\n" % picks[0] + "".join(p + "\n" for p in picks[1:]) + picks[2] + "\r\n").encode())
    plist = so.read_attr_list(open(lst, "rb").read())
    assert plist[0] == picks[0] and len(plist) == len(picks) + 1
    check(gff, data, B, values, a2f, plist, False, attr_list=lst)
    rlst = str(d / "rlist.txt")
    open(rlst, "w").write("^G1[0-9]$\ndup$\n^nothing$\nG2.5\n")
    rl = so.read_attr_list(open(rlst, "rb").read())
    check(gff, data, B, values, a2f, rl, True, attr_list=rlst)
    # the hit lines cut into several chunks: the same bytes
    want, S = so.search_run(data, B.gof, "gene_name", values, a2f, B.prt, rl, True, False, None)
    first = len(want.split(b"\n")[0]) + 1
    assert want.count(b"\n") > 3
    for budget in (1, first, 4096):
        r = run_cli(gff, None, rlst, True, False, None, env=dict(os.environ, GFFX_EXTRACT_CHUNK_BYTES=str(budget)),
                    extra=["--stats-json", str(d / "st.json")])
        assert r.returncode == 0 and r.stdout == want, budget
        js = json.load(open(str(d / "st.json")))
        assert js["command"] == "search" and js["counts"]["unique_roots"] == len(S.roots)
        if budget == 1:
            assert js["counts"]["filter_chunks"] == js["counts"]["lines_tested"] > 3
    r = run_cli(gff, None, rlst, True, False, None, extra=["-v"])
    assert r.returncode == 0 and b"[TIMER] [device] table build" in r.stderr and b"k_attr_match_dfa<lds>" in r.stderr


def test_the_three_bails_and_both_warnings(synth_gff, tmp_path):
    d, gff0, data, B, values, a2f = synth_gff
    r = run_cli(gff0, "no_such_gene")
    assert r.returncode == 1 and r.stderr == b"Error: None of the attributes matched.\n" and r.stdout == b""
    import shutil
    gff = str(tmp_path / "s.gff")
    for ext in ("", ".gof", ".fts", ".prt", ".sqs", ".atn", ".a2f", ".rit", ".rix"):
        shutil.copy(gff0 + ext, gff + ext)
    # a value no fid carries: a line appended to .atn
    open(gff + ".atn", "ab").write(b"LONELY\n")
    vals2 = so.load_atn(open(gff + ".atn", "rb").read())[1]
    r = run_cli(gff, "LONELY")
    S = so.steps(vals2, a2f, B.prt, ["LONELY"], False)
    assert S.bail == "No feature IDs (FIDs) resolved from matched attributes." and S.no_fid_aids == [len(values)]
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.split(b"\n")[:-1] == so.warn_lines(S) + [b"Error: " + S.bail.encode()]
    # ... beside one that has fids: a warning, and the run goes on
    lst = str(tmp_path / "l.txt")
    open(lst, "w").write("LONELY\n%s\n" % values[0])
    want, S = so.search_run(data, B.gof, "gene_name", vals2, a2f, B.prt, ["LONELY", values[0]], False, False, None)
    r = run_cli(gff, None, lst)
    assert r.returncode == 0 and r.stdout == want and [ln for ln in r.stderr.split(b"\n") if ln.startswith(b"[WARN]")] == so.warn_lines(S)
    # parents out of range: every fid of values[0] gets one
    prt = list(B.prt)
    fids0 = [f for f, a in enumerate(a2f) if a == 0]
    for f in fids0:
        prt[f] = len(prt) + 5
    open(gff + ".prt", "wb").write(np.array(prt, dtype="<u4").tobytes())
    S = so.steps(vals2, a2f, prt, [values[0]], False)
    assert S.bail == "No valid root features resolved from matched attributes." and S.invalid == fids0
    r = run_cli(gff, values[0])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.split(b"\n")[:-1] == so.warn_lines(S) + [b"Error: " + S.bail.encode()]
    # ... and only some of the matched fids: the warning, and the output of the others
    two = [values[0], values[1]]
    open(lst, "w").write("".join(v + "\n" for v in two))
    want, S = so.search_run(data, B.gof, "gene_name", vals2, a2f, prt, two, False, False, None)
    assert S.invalid == fids0 and S.roots
    r = run_cli(gff, None, lst)
    assert r.returncode == 0 and r.stdout == want and [ln for ln in r.stderr.split(b"\n") if ln.startswith(b"[WARN]")] == so.warn_lines(S)


def test_the_loader_keeps_a_bom_behind_the_header_and_trims_unicode_blanks(synth_gff, tmp_path):
    """core.rs:50-57 through the command: trim() takes U+00A0 and U+3000 off a value line; a BOM is stripped only from lines seen
    before the header, so behind it the BOM stays part of the value"""
    import shutil
    d, gff0, data, B, values, a2f = synth_gff
    gff = str(tmp_path / "s.gff")
    for ext in ("", ".gof", ".fts", ".prt", ".sqs", ".atn", ".a2f", ".rit", ".rix"):
        shutil.copy(gff0 + ext, gff + ext)
    bom, nbsp, ideo = "\ufeff", "\u00a0", "\u3000"
    rows = [bom + "#attribute=gene_name\r", nbsp + values[0] + ideo + " ", bom + values[1]] + values[2:]
    open(gff + ".atn", "wb").write("".join(r + "\n" for r in rows).encode())
    name, vals2 = so.load_atn(open(gff + ".atn", "rb").read())
    assert name == "gene_name" and vals2[0] == values[0] and vals2[1] == bom + values[1] and len(vals2) == len(values)
    for attr in (values[0], bom + values[1], values[1]):
        want, S = so.search_run(data, B.gof, name, vals2, a2f, B.prt, [attr], False, True, None)
        r = run_cli(gff, attr, entire_group=True)
        if S.bail:
            assert attr == values[1] and r.returncode == 1 and r.stderr == b"Error: None of the attributes matched.\n"
        else:
            assert r.returncode == 0 and r.stdout == want and len(want) > 0, attr
