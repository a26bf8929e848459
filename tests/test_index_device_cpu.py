"""`gffx index --gpu` without a GPU: the rules of one GFF3 line that k_gff_rows shares with the host (device/gff_core.hpp) and the
host restatement of the finish steps of device/gff.hip, built under AddressSanitizer + UndefinedBehaviorSanitizer
(tools/gff_check.cpp) and compared with hand-worked answers (tests/_index_cases.py) and with the Python restatement of the
reference's index builder (oracle.gffx_oracle_py.build_index); and what the command line decides before it asks for a device."""
import os
import subprocess

import pytest

import _index_cases as ic
from gffx_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "gff_check")
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "gff_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def _unhex(s):
    return None if s == "-" else b"" if s == "." else bytes.fromhex(s)


def _parse_line_result(out: str):
    w = out.split(" ")
    if w[0] == "row":
        return ("row", int(w[1]), int(w[2]), int(w[3]), _unhex(w[4]), _unhex(w[5]), _unhex(w[6]), _unhex(w[7]))
    if w[0] == "skipped_type":
        return ("skipped_type", _unhex(w[1]))
    return out


def _groups():
    """the single-line cases grouped by (key, skip): one run of the tool per group"""
    g = {}
    for c in ic.LINE_CASES:
        g.setdefault((c[2], c[3]), []).append(c)
    return g


def test_single_lines_against_the_hand_worked_table(tool, tmp_path):
    for (key, skip), cases in _groups().items():
        assert all(b"\n" not in c[1] for c in cases)
        p = tmp_path / "lines.gff"
        p.write_bytes(b"".join(c[1] + b"\n" for c in cases))
        out = _run(tool, "lines", p, key, skip)
        assert len(out) == len(cases)
        for c, o in zip(cases, out):
            assert _parse_line_result(o) == c[4], c[0]


def test_single_lines_against_the_python_restatement(tool, tmp_path):
    for name, line, key, skip, want in ic.LINE_CASES:
        kind, b = ic.oracle_outcome(line + b"\n", key, skip)
        if isinstance(want, tuple) and want[0] == "row":
            assert kind == "ok" and len(b.ids) == 1, name
            assert b.ids[0].encode() == want[5], name
            assert b.trees_input == [[(want[1], want[2], 0)]] and b.seqids == [want[4].decode()], name
            assert b.atn == ([want[7].decode()] if want[7] is not None else []), name
            # a Parent is visible only in a second line that bears its name
            if want[6] is not None and b"\t" not in want[6] and b";" not in want[6]:
                two = line + b"\n" + ic.feat(attrs=b"ID=" + want[6]) + b"\n"
                assert ic.oracle_outcome(two, key, skip)[1].prt[0] == 1, name
        elif want in ("BAD_UTF8", "COLUMNS", "DIGITS", "NO_ID"):
            assert (kind, b) == ("error", want), name
        else:
            assert kind == "ok" and b.ids == [], name


def _parse_build(out):
    if out and out[0].startswith("error "):
        w = out[0].split(" ")
        return dict(error=(int(w[1]), w[2]))
    r = dict(ids=[], fid=[], prt=[], a2f=[], atn=[], seqids=[], gof=[], roots=[])
    for ln in out:
        w = ln.split(" ")
        if w[0] == "counts":
            r["counts"] = dict(zip(("lines", "blank", "skipped_type", "zero_end", "rows", "roots", "seqids", "attr_values"), map(int, w[1:])))
        elif w[0] == "row":
            r["ids"].append(_unhex(w[1]).decode())
            r["fid"].append(int(w[2]))
            r["prt"].append(int(w[3]))
            r["a2f"].append(ic.NONE if w[4] == "-1" else int(w[4]))
        elif w[0] == "seqid":
            r["seqids"].append(_unhex(w[1]).decode())
        elif w[0] == "value":
            r["atn"].append(_unhex(w[1]).decode())
        elif w[0] == "gof":
            r["gof"].append(tuple(map(int, w[1:])))
        elif w[0] == "root":
            r["roots"].append(tuple(map(int, w[1:])))
    trees = [[] for _ in r["seqids"]]
    for s, e, f, q in r["roots"]:
        trees[q].append((s, e, f))
    r["trees_input"] = trees
    return r


def _build_tuple(r):
    return (r["ids"], r["fid"], r["prt"], r["a2f"], r["atn"], r["seqids"], r["gof"], r["trees_input"])


@pytest.mark.parametrize("hash_bits", [None, 0, 2])
def test_whole_file_against_the_hand_worked_arrays(tool, tmp_path, hash_bits):
    for fc in ic.FILE_CASES:
        p = tmp_path / "f.gff"
        p.write_bytes(fc["text"])
        got = _parse_build(_run(tool, "build", p, fc["key"], fc["skip"], *([] if hash_bits is None else [hash_bits])))
        for k in ("ids", "fid", "prt", "a2f", "atn", "seqids", "gof", "trees_input", "counts"):
            assert got[k] == fc[k], k
        kind, b = ic.oracle_outcome(fc["text"], fc["key"], fc["skip"])
        assert kind == "ok" and ic.built_tuple(b) == _build_tuple(got)


@pytest.mark.parametrize("hash_bits", [None, 0, 2])
def test_families_against_the_python_restatement(tool, tmp_path, hash_bits):
    # duplicates (the last line wins, the earlier one stays a root with the later fid), children before their gene, values
    # repeated across seqids, type-skipped and blank lines in between; a last line without '\n'
    text = ic.family_file(120, seqs=5, kids=2, dup_every=7, blank_every=9)[:-1]
    p = tmp_path / "fam.gff"
    p.write_bytes(text)
    for key in ("gene_name", "ID", "Parent"):
        got = _parse_build(_run(tool, "build", p, key, ic.DEFAULT_SKIP, *([] if hash_bits is None else [hash_bits])))
        kind, b = ic.oracle_outcome(text, key, ic.DEFAULT_SKIP)
        assert kind == "ok" and ic.built_tuple(b) == _build_tuple(got), key
        assert got["counts"]["rows"] == len(b.ids) and got["counts"]["roots"] == len(b.gof)
    assert any(f != i for i, f in enumerate(b.fid))  # the case has duplicates


def test_the_first_bad_line_ends_the_build(tool, tmp_path):
    good = ic.family_file(5)
    bad = {"BAD_UTF8": ic.feat(attrs="ID=x") + b"\xff", "COLUMNS": b"chr1\tonly", "DIGITS": ic.feat(s="1e3"), "NO_ID": ic.feat(attrs="Name=q")}
    for kind, line in bad.items():
        other = bad["COLUMNS" if kind != "COLUMNS" else "NO_ID"]
        text = good + line + b"\n" + good + other + b"\n"
        p = tmp_path / "bad.gff"
        p.write_bytes(text)
        got = _parse_build(_run(tool, "build", p, "gene_name", ic.DEFAULT_SKIP))
        assert got == dict(error=(len(good), kind))
        assert ic.oracle_outcome(text, "gene_name", ic.DEFAULT_SKIP) == ("error", kind)


# ---- the command line, before it asks for a device -------------------------------------------------------------------------
def test_index_help_names_the_gpu_flags():
    r = subprocess.run([GFFX, "index", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gpu" in r.stdout and "--device" in r.stdout


@pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
def test_gpu_flag_without_a_device_fails_and_writes_nothing(tmp_path):
    gff = tmp_path / "a.gff"
    gff.write_bytes(ic.FILE_1["text"])
    r = subprocess.run([GFFX, "index", "-i", str(gff), "--gpu"], capture_output=True, text=True)
    assert r.returncode != 0 and "no HIP device visible" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.gff"]
    with pytest.raises(engine._ffi.GffxHipError) as ei:
        engine.GffIndexer()
    assert ei.value.code == -2  # GFFX_E_NO_DEVICE


def test_host_index_is_unchanged_by_the_split(tmp_path):
    # the host path's files for the hand-worked file, byte for byte
    fc = ic.FILE_1
    gff = tmp_path / "a.gff"
    gff.write_bytes(fc["text"])
    r = subprocess.run([GFFX, "index", "-i", str(gff)], capture_output=True, text=True, env=dict(os.environ, GFFX_LINE_TABLE="off"))
    assert r.returncode == 0, r.stderr
    rd = lambda s: open(str(gff) + s, "rb").read()  # noqa: E731
    assert rd(".fts") == "".join(i + "\n" for i in fc["ids"]).encode()
    assert rd(".sqs") == "".join(i + "\n" for i in fc["seqids"]).encode()
    assert rd(".atn") == ("#attribute=gene_name\n" + "".join(i + "\n" for i in fc["atn"])).encode()
    import struct
    assert rd(".prt") == struct.pack("<%dI" % len(fc["prt"]), *fc["prt"])
    assert rd(".a2f") == struct.pack("<%dI" % len(fc["a2f"]), *fc["a2f"])
    assert rd(".gof") == b"".join(struct.pack("<IIQQ", *g) for g in fc["gof"])
    assert rd(".rix").startswith(b"[0,") and len(rd(".rit")) > 0
