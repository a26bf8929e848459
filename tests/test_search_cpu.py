"""`gffx search` without a GPU: the regex compiler (host/regex_dfa.cpp) and the rules the kernels of device/search.hip share with
the host (device/search_core.hpp: the DFA match loop, the pair set, the line test), built for the host under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/search_check.cpp, a stand-alone program); the same compiler through engine.compile_regex
against Python's re.search; and what the command line decides before it asks for a device."""
import os
import re
import shutil
import subprocess

import pytest

import _search_cases as sc
import _search_oracle as so
from gffx_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "search_check")
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "search_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, env=env, timeout=600)
    assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.decode().splitlines()


def _write(path, items):
    path.write_bytes(b"".join((i if isinstance(i, bytes) else i.encode()) + b"\n" for i in items))
    return path


# ---- the stand-alone program under the sanitizers -------------------------------------------------------------------------------
def test_parser_accept_and_reject_table(tool):
    out = _run(tool, "syntax")
    assert out and out[0].startswith("ok ") and int(out[0].split()[1]) >= 60


FIXED_PATTERNS = ["TP53", "^TP53$", "TP5[0-9]", "^$", "", "$^", "a|", "(ab?){2,3}c", "[^a]{3}", ".{16}", "^.{17}$", "é+", "😀.?→", "x{255}",
                  "(^a|b$)", "a*?b", "(a|b)*c$", "[]a-]+", r"\.\*", "^(?:G[0-9]+|ENSG0*1)$", "[^ -~]", "a{0}b", "(|x)y", "^^a", "a$$"]
FIXED_VALUES = ["", "a", "b", "ab", "abc", "abac", "ababc", "TP53", "TP53BP1", "xTP53", "TP5", "TP59", "é", "éé", "a😀→", "😀x→", "😀xx→", "x" * 254,
                "x" * 255, "x" * 256, "a" * 15, "a" * 16, "a" * 17, "→" * 16, "→" * 17, ".*", "]-a", "G12", "ENSG00001", "ENSG2", "y", "xy", "cab"]


def test_dfa_equals_the_direct_nfa_simulation_and_re_search(tool, tmp_path):
    out = _run(tool, "dfa", _write(tmp_path / "p.txt", FIXED_PATTERNS), _write(tmp_path / "v.txt", FIXED_VALUES[1:]))  # ("" cannot be a line)
    assert len(out) == len(FIXED_PATTERNS)
    for p, row in zip(FIXED_PATTERNS, out):
        assert row == "".join("1" if re.search(p, v) else "0" for v in FIXED_VALUES[1:]), p


@pytest.mark.parametrize("cap,groups", [(2, None), (3, "0:1:3 1:2:3 3:1:3"), (4096, "0:4:5")])
def test_group_splitting_at_state_caps(tool, tmp_path, cap, groups):
    pats = ["ab", "cd", "e", "fg"]
    values = ["ab", "xcdx", "e", "fg", "a", "b", "gf", "abcd", "éab", "af"]
    out = _run(tool, "union", _write(tmp_path / "p.txt", pats), _write(tmp_path / "v.txt", values), cap)
    if groups is None:
        assert out == ['error regex too large: "ab" needs more than 2 DFA states']
        out = _run(tool, "union", _write(tmp_path / "p1.txt", ["a", "b", "[c-e]"]), _write(tmp_path / "v.txt", values), cap)
        assert out[0] == "groups 0:3:2"  # one-scalar patterns need the start state and the accepting one
        assert out[1:] == ["1" if re.search("a|b|[c-e]", v) else "0" for v in values]
        return
    assert out[0] == "groups " + groups
    assert out[1:] == ["1" if any(re.search(p, v) for p in pats) else "0" for v in values]


def test_keep_line_value_on_exact_size_copies(tool, tmp_path):
    values = _write(tmp_path / "atn.txt", ["TP53", "BRCA1", "TP53", "EGFR"])
    matched = _write(tmp_path / "m.txt", ["TP53"])
    for types in (None, "exon", " exon , gene,,", ","):
        allow = so.xo.split_types(types)
        extra = [] if types is None else ["-T", types]
        with_nl = [l for l, _ in sc.VALUE_LINES if l.endswith(b"\n")]
        (tmp_path / "t.gff").write_bytes(b"".join(with_nl))
        got = [int(x) for x in _run(tool, "filter", tmp_path / "t.gff", values, "gene_name", matched, *extra)]
        assert got == [int(so.xo.keeps_line(l, {"TP53"}, allow, b"gene_name")) for l in with_nl], types
        for l, k in sc.VALUE_LINES:
            if not l.endswith(b"\n"):  # the key or the value at the very end of the text
                (tmp_path / "t1.gff").write_bytes(l)
                got1 = [int(x) for x in _run(tool, "filter", tmp_path / "t1.gff", values, "gene_name", matched, *extra)]
                assert got1 == [int(so.xo.keeps_line(l, {"TP53"}, allow, b"gene_name"))]
        if types is None:
            assert got == [k for l, k in sc.VALUE_LINES if l.endswith(b"\n")]


# ---- the compiler through ctypes, against re.search -------------------------------------------------------------------------------
def test_generated_patterns_against_re_search():
    pats, values = sc.corpus()
    assert len(pats) > 300 and {len(v) for v in values} >= {0, 1, 15, 16, 17, 300}
    pairs = 0
    for p in pats:
        c = engine.compile_regex([p], 65535)  # (a cap no pattern of the corpus reaches: no case is left out)
        want = [bool(re.search(p, v)) for v in values]
        assert c.match(values).tolist() == want, p
        pairs += len(values)
        c.close()
    assert pairs > 15000
    # ... and as lists: one alternation, split into groups under a small cap
    for k in range(0, len(pats), 25):
        part = pats[k:k + 25]
        want = [any(re.search(p, v) for p in part) for v in values]
        for cap in (4096, 64):
            try:
                c = engine.compile_regex(part, cap)
            except engine.RegexError as e:
                assert "regex too large" in str(e)
                continue
            assert sum(g["n_patterns"] for g in c.groups) == len(part) and all(g["n_states"] <= cap for g in c.groups)
            assert c.match(values).tolist() == want, (k, cap)


def test_the_default_cap_keeps_a_table_within_64_kib(monkeypatch):
    c = engine.compile_regex(["^(?:G[0-9]+|ENSG0*1)$", "x{200}"])
    assert all(256 + 2 * g["n_states"] * g["n_classes"] <= 65536 for g in c.groups)
    with pytest.raises(engine.RegexError, match="regex too large"):
        engine.compile_regex(["[^a]{255}"])
    monkeypatch.setenv("GFFX_SEARCH_DFA_STATES", "3")
    assert len(engine.compile_regex(["ab", "cd"]).groups) == 2
    with pytest.raises(engine.RegexError, match='regex too large: "abc" needs more than 3 DFA states'):
        engine.compile_regex(["abc"])
    with pytest.raises(engine.RegexError, match=r'unsupported regex syntax at byte 2 of "ab\\d": the escape'):
        engine.compile_regex(["ab\\d"])


def test_host_regex_exports_match_the_header():
    from gffx_amd import _ffi
    src = open(os.path.join(ROOT, "include", "gffx_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gffx_host_regex_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_ffi.HOST_SIGNATURES) and len(declared) == 6
    decl = {m.group(1): m.group(2) for m in re.finditer(r"(gffx_host_regex_[a-z_]+)\s*\(([^;]*)\)\s*;", src)}
    for name, (_res, args) in _ffi.HOST_SIGNATURES.items():
        assert len([a for a in decl[name].split(",") if a.strip()]) == len(args), name  # the same number of parameters
        assert hasattr(_ffi.host_lib(), name)
    L = _ffi.host_lib()  # NULL arguments are refused, not dereferenced
    assert L.gffx_host_regex_compile(1, None, None, 0, None, None, 0) == -1
    assert L.gffx_host_regex_group_info(None, 0, None, None, None, None, None) == -1
    assert L.gffx_host_regex_group_tables(None, 0, None, None) == -1 and L.gffx_host_regex_match(None, 1, None, None, None) == -1
    c = engine.compile_regex(["a"])
    assert L.gffx_host_regex_group_info(c._h, 0, None, None, None, None, None) == -1 and L.gffx_host_regex_match(c._h, 1, None, None, None) == -1
    h, err = _ffi.vp(), __import__("ctypes").create_string_buffer(200)
    assert L.gffx_host_regex_compile(1, None, None, 0, __import__("ctypes").byref(h), err, 200) == -1 and b"NULL" in err.value


def test_deep_nesting_is_refused_by_name():
    assert engine.compile_regex(["(" * 100 + "a" + ")" * 100]).match(["a", "b"]).tolist() == [True, False]
    with pytest.raises(engine.RegexError, match="unsupported regex syntax at byte 100 of .*groups nested more than 100 deep"):
        engine.compile_regex(["(" * 3000 + "a"])


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indexed(tmp_path_factory, golden_dir):
    d = tmp_path_factory.mktemp("search_cli")
    gff = str(d / "t.gff")
    shutil.copy(os.path.join(golden_dir, "appendix_e.gff"), gff)
    assert subprocess.run([GFFX, "index", "-i", gff], capture_output=True).returncode == 0
    (d / "names.txt").write_text("A\n")
    return gff, str(d / "names.txt")


def test_exactly_one_of_attr_and_attr_list(indexed):
    gff, names = indexed
    r = subprocess.run([GFFX, "search", "-i", gff], capture_output=True)
    assert r.returncode == 2 and b"<--attr-list <ATTR_LIST>|--attr <ATTR>>" in r.stderr and b"Usage: gffx search" in r.stderr
    r = subprocess.run([GFFX, "search", "-i", gff, "-a", "A", "-A", names], capture_output=True)
    assert r.returncode == 2 and b"cannot be used with" in r.stderr
    r = subprocess.run([GFFX, "search", "-a", "A"], capture_output=True)
    assert r.returncode == 2 and b"--input <FILE>" in r.stderr
    r = subprocess.run([GFFX, "search", "-i", gff, "-a", "A", "--gpus", "2"], capture_output=True)
    assert r.returncode == 2 and b"--gpus" in r.stderr
    r = subprocess.run([GFFX, "search", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--attr-list" in r.stdout and b"--regex" in r.stdout and b"--entire_group" in r.stdout
    assert b"search" in subprocess.run([GFFX, "help"], capture_output=True).stdout


def test_regex_errors_come_before_the_device(indexed):
    gff, _ = indexed
    r = subprocess.run([GFFX, "search", "-i", gff, "-r", "-a", "^\\w+$"], capture_output=True)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.startswith(b'Error: unsupported regex syntax at byte 1 of "^\\w+$": the escape \'\\w\'')
    r = subprocess.run([GFFX, "search", "-i", gff, "-r", "-a", "[^a]{255}"], capture_output=True)
    assert r.returncode == 1 and r.stderr.startswith(b'Error: regex too large: "[^a]{255}" needs more than')
    r = subprocess.run([GFFX, "search", "-i", gff, "-r", "-a", "abc"], capture_output=True, env=dict(os.environ, GFFX_SEARCH_DFA_STATES="3"))
    assert r.returncode == 1 and r.stderr == b'Error: regex too large: "abc" needs more than 3 DFA states\n'


def test_damaged_side_cars_and_lists_are_refused_on_the_host(indexed, tmp_path):
    gff = str(tmp_path / "t.gff")
    exts = ("", ".gof", ".fts", ".prt", ".sqs", ".atn", ".a2f", ".rit", ".rix")
    for ext in exts:
        shutil.copy(indexed[0] + ext, gff + ext)

    def fails(msg, *args):
        r = subprocess.run([GFFX, "search", "-i", gff] + (list(args) or ["-a", "A"]), capture_output=True)
        assert r.returncode == 1 and msg in r.stderr and r.stdout == b"", r.stderr

    with open(gff + ".a2f", "ab") as f:
        f.write(b"\x00")
    fails(b"Error: Corrupted A2F (" + gff.encode() + b".a2f): length 29 not aligned to u32")
    shutil.copy(indexed[0] + ".a2f", gff + ".a2f")
    open(gff + ".atn", "wb").write(b"A\nB\n")
    fails(b"Error: Missing #attribute=... header in .atn file")
    open(gff + ".atn", "wb").write(b"#attribute=gene_name\nA\n#attribute=x\n")
    fails(b"Error: Multiple #attribute= headers found in .atn file")
    open(gff + ".atn", "wb").write(b"#attribute=gene_name\nA\n\xff\n")
    fails(b"Error: ATN contains invalid UTF-8")
    shutil.copy(indexed[0] + ".atn", gff + ".atn")
    (tmp_path / "bad.txt").write_bytes(b"A\n\xff\n")
    fails(b"valid UTF-8", "-A", str(tmp_path / "bad.txt"))
    fails(b"Cannot open attribute list", "-A", str(tmp_path / "no_such_list.txt"))
    os.remove(gff + ".atn")
    fails(b'Missing index file(s): [".atn"]')


@pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
def test_no_cpu_fallback_without_a_gpu(indexed):
    for extra in ([], ["-e"], ["-T", "exon"], ["-r"]):
        r = subprocess.run([GFFX, "search", "-i", indexed[0], "-a", "A"] + extra, capture_output=True)
        assert r.returncode == 1 and b"no HIP device" in r.stderr and r.stdout == b"", r.stderr
