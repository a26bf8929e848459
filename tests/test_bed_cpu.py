"""The BED text front end shared by the host and k_bed_rows (device/bed_core.hpp: one line in the two dialects, with
gff_core.hpp's UTF-8 rule and sam_core.hpp's names table), built for the host under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/bed_check.cpp): the outcome of every line equal to the hand table and to the Python
restatement, the file shapes a reader meets (no final newline, empty, comments only, a single newline, a 1 MiB line, a 1 MiB
name), names tables of 1, 2 and 5000 names with forced probe chains, and no sanitizer report anywhere.  No GPU."""
import os
import subprocess

import pytest

import _bed_cases as cases
import _bed_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "bed_check")
DIALECTS = [bo.INTERSECT, bo.DEPTH]


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "bed_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _want_lines(text, dialect, names):
    """What `bed_check rows` prints for `text`: it goes on after a malformed line, so every line has its outcome."""
    table = bo.name_table(names)
    out, tally = [], {"lines": 0, "skipped": 0, "no_seq": 0, "kept": 0, "malformed": 0}
    for line in bo.lines_of(text, dialect):
        o = bo.outcome(line, dialect, table)
        tally["lines"] += 1
        if o[0] == "keep":
            out.append("keep %d %d %d" % o[1:])
            tally["kept"] += 1
        elif o[0] == "skip":
            out.append("skip " + o[1])
            tally["no_seq" if o[1] == "noseq" else "skipped"] += 1
        else:
            out.append("malformed " + o[1])
            tally["malformed"] += 1
    out.append("tally %(lines)d %(skipped)d %(no_seq)d %(kept)d %(malformed)d" % tally)
    return out


def _rows(tool, tmp_path, text, dialect, names, tag="in"):
    path = tmp_path / (tag + ".bed")
    path.write_bytes(text)
    nf = tmp_path / (tag + ".names")
    nf.write_bytes(b"".join(n + b"\n" for n in names))
    r = _run(tool, "rows", path, bo.DIALECT_NAME[dialect], "@%s" % nf)
    assert r.returncode == 0, r.stderr[-500:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("dialect", DIALECTS)
def test_every_line_of_the_table_has_its_outcome(tool, tmp_path, dialect):
    exp = cases.expected(dialect)
    text = b"".join(line + b"\n" for line, _ in exp)
    got = _rows(tool, tmp_path, text, dialect, cases.NAMES)
    want = ["keep %d %d %d" % w[1:] if w[0] == "keep" else ("skip " if w[0] == "skip" else "malformed ") + w[1] for _, w in exp]
    assert got[:-1] == want
    assert got == _want_lines(text, dialect, cases.NAMES)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_generated_lines_equal_the_oracle(tool, tmp_path, dialect):
    lines = bo.generate(20000, 11, dialect) + bo.generate(500, 12, bo.INTERSECT, errors=True)
    text = b"".join(ln + b"\n" for ln in lines)
    assert _rows(tool, tmp_path, text, dialect, bo.GEN_NAMES) == _want_lines(text, dialect, bo.GEN_NAMES)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_file_shapes(tool, tmp_path, dialect):
    big = b"x" * (1 << 20)
    shapes = {
        "no_final_newline": b"chr1\t1\t2\nchr10\t3\t4",
        "no_final_newline_cut_utf8": b"chr1\t1\t2\n" + "chrü".encode()[:-1],
        "empty": b"",
        "comments_only": b"#a\n#b\n# c",
        "single_newline": b"\n",
        "newlines": b"\n\n\n",
        "mib_line": b"chr1\t1\t2\t" + big + b"\nchr1\t5\t6\n",
        "mib_line_invalid_end": b"chr1\t1\t2\t" + big + b"\xe2\x82\nchr1\t5\t6\n",
        "mib_name": big + b"\t1\t2\n" + big[:-1] + b"\t1\t2\nchr1\t5\t6\n",
        "mib_digits": b"chr1\t" + b"0" * (1 << 20) + b"7\t9\nchr1\t1\t" + b"9" * (1 << 20) + b"\n",
    }
    names = cases.NAMES + [big]
    for tag, text in shapes.items():
        got = _rows(tool, tmp_path, text, dialect, names, tag)
        assert got == _want_lines(text, dialect, names), tag
    # ... and what the shapes mean, in words
    assert _rows(tool, tmp_path, shapes["empty"], dialect, names) == ["tally 0 0 0 0 0"]
    assert _rows(tool, tmp_path, shapes["mib_name"], dialect, names)[:3] == ["keep 5 1 2", "skip noseq", "keep 0 5 6"]
    assert _rows(tool, tmp_path, shapes["mib_digits"], dialect, names)[0] == "keep 0 7 9"


def _fnv1a(b):
    h = 2166136261
    for c in b:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


@pytest.mark.parametrize("n", [1, 2, 5000])
def test_names_tables_and_probe_chains(tool, tmp_path, n):
    names = [b"n%d" % (i * 7919) for i in range(n)]
    slots = 2
    while slots < 2 * n:
        slots *= 2
    if n == 5000:  # forced chains: 40 more names whose hash falls on one slot, found by search
        home = _fnv1a(names[0]) & (slots - 1)
        i, chain = 0, []
        while len(chain) < 40:
            c = b"c%d" % i
            i += 1
            if _fnv1a(c) & (slots - 1) == home:
                chain.append(c)
        names = names + chain
        while slots < 2 * len(names):
            slots *= 2
        home = _fnv1a(names[0]) & (slots - 1)
        assert sum(_fnv1a(x) & (slots - 1) == home for x in names) >= 20  # (a larger table keeps every second one of them)
    queries = names + [b"", b"n", names[0] + b"x", names[-1][:-1], b"absent", b"\xff\x00\x80"] + [x.upper() for x in names[:50]]
    (tmp_path / "names").write_bytes(b"".join(x + b"\n" for x in names))
    (tmp_path / "queries").write_bytes(b"".join(x + b"\n" for x in queries))
    r = _run(tool, "lookup", tmp_path / "names", tmp_path / "queries")
    assert r.returncode == 0, r.stderr[-500:]
    out = r.stdout.splitlines()
    assert out[0] == "slots %d" % slots
    value = {x: i for i, x in enumerate(names)}
    assert [int(v) for v in out[1:]] == [value.get(q, -1) for q in queries]
    # a name twice is refused
    (tmp_path / "dup").write_bytes(b"a\nb\na\n")
    r = _run(tool, "lookup", tmp_path / "dup", tmp_path / "queries")
    assert r.returncode == 3 and r.stdout.splitlines()[0] == "duplicate 2"


def test_utf8_validator(tool, tmp_path):
    lines = [line for line, _, _ in cases.CASES] + [
        b"\xc2", b"\xc2\x80", b"\xc1\xbf", b"\xe0\x9f\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xed\xa0\x80", b"\xee\x80\x80",
        b"\xf0\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\x80", b"a\xbf",
        b"\xe2\x82\xac", b"\xe2\x82", b"\xe2", b"\xf0\x9f\x98", "žluťoučký kůň 染色体 😀".encode(), b"\x00\x7f",
    ]
    (tmp_path / "u").write_bytes(b"".join(x + b"\n" for x in lines))
    r = _run(tool, "utf8", tmp_path / "u")
    assert r.returncode == 0
    # (the tool cuts at '\n' and drops nothing but an empty rest: the table's empty line stays a line)
    assert [int(v) for v in r.stdout.split()] == [int(bo.utf8_valid(x)) for x in lines]
