"""The Python restatement of the two BED dialects (tests/_bed_oracle.py) against the hand-worked table (tests/_bed_cases.py) and
against the host parsers it restates (gffx_host_parse_bed_file, gffx_host_parse_bed_file_chunked: host/bed_parse.cpp;
gffx_host_depth_parse_bed: host/depth.cpp), on the table's error-free lines and on 20 000 generated ones whose condition is
checked first, on the oracle alone.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import _bed_cases as cases
import _bed_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "gffx_amd", "lib", "libgffx_host.so"))
    L.gffx_host_build_index.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.gffx_host_load_tree_index.argtypes = [C.c_char_p, u32p, C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u32p),
                                            C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.gffx_host_parse_bed_file.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(u32p), u64p, C.c_char_p, C.c_size_t]
    L.gffx_host_parse_bed_file_chunked.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(u32p), u64p, C.c_char_p,
                                                   C.c_size_t]
    L.gffx_host_depth_parse_bed.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(u32p), u64p, C.c_char_p, C.c_size_t]
    L.gffx_host_free.argtypes = [C.c_void_p]
    return L


def make_index(host, directory, names):
    """A GFF with one gene on each of `names`, indexed; returns its path and the names in the index's seqid order."""
    gff = os.path.join(str(directory), "names.gff")
    with open(gff, "wb") as f:
        f.write(b"##gff-version 3\n")
        for i, n in enumerate(names):
            f.write(n + b"\tt\tgene\t100\t900\t.\t+\t.\tID=g%d;gene_name=n%d\n" % (i, i))
    e = C.create_string_buffer(2048)
    assert host.gffx_host_build_index(gff.encode(), b"gene_name", b"region", 0, e, len(e)) == 0, e.value
    n = C.c_uint32()
    pco, ps, pe, pf, pn = u32p(), u32p(), u32p(), u32p(), C.c_void_p()
    assert host.gffx_host_load_tree_index(gff.encode(), C.byref(n), C.byref(pco), C.byref(ps), C.byref(pe), C.byref(pf), C.byref(pn), e,
                                          len(e)) == 0, e.value
    order = C.string_at(pn).split(b"\n")
    for p in (pco, ps, pe, pf, pn):
        host.gffx_host_free(p)
    assert sorted(order) == sorted(names)
    return gff, order


def _host_rows(host, fn, gff, bed, *extra):
    e = C.create_string_buffer(4096)
    pr, nr = u32p(), C.c_uint64()
    rc = fn(gff.encode(), bed.encode(), *extra, C.byref(pr), C.byref(nr), e, len(e))
    if rc != 0:
        return None, e.value.decode(errors="replace")
    got = np.ctypeslib.as_array(pr, shape=(max(nr.value, 1), 3))[: nr.value].copy()
    host.gffx_host_free(pr)
    return got, None


def _against_host(host, tmp_path, names, lines, dialect, tag):
    gff, order = make_index(host, tmp_path, names)
    want, counts, err, _ = bo.run(b"".join(ln + b"\n" for ln in lines), dialect, order)
    assert err is None and counts["lines"] == len(lines) == counts["skipped"] + counts["no_seq"] + counts["kept"]
    bed = str(tmp_path / (tag + ".bed"))
    open(bed, "wb").write(b"".join(ln + b"\n" for ln in lines))
    if dialect == bo.DEPTH:
        got, msg = _host_rows(host, host.gffx_host_depth_parse_bed, gff, bed)
        assert msg is None and np.array_equal(got, want)
        return
    got, msg = _host_rows(host, host.gffx_host_parse_bed_file, gff, bed)
    assert msg is None and np.array_equal(got, want)
    for threads, chunk in ((1, 64), (3, 1000), (4, 1 << 20)):
        got, msg = _host_rows(host, host.gffx_host_parse_bed_file_chunked, gff, bed, threads, chunk)
        assert msg is None and np.array_equal(got, want), (threads, chunk)


@pytest.mark.parametrize("dialect", [bo.INTERSECT, bo.DEPTH])
def test_oracle_equals_the_hand_table(dialect):
    table = bo.name_table(cases.NAMES)
    for line, want in cases.expected(dialect):
        assert bo.outcome(line + b"\n" if dialect == bo.DEPTH else line, dialect, table) == want, line[:60]
    # every class the table has to cover occurs
    kinds = {w for _, w in cases.expected(dialect) if w[0] != "keep"}
    for why in bo.SKIP_KINDS[dialect]:
        assert ("skip", why) in kinds, why
    if dialect == bo.INTERSECT:
        assert ("error", "utf8") in kinds and ("error", "coordinate") in kinds
    else:
        assert not any(k[0] == "error" for k in kinds)


@pytest.mark.parametrize("dialect", [bo.INTERSECT, bo.DEPTH])
def test_oracle_equals_the_host_parser_on_the_table(host, tmp_path, dialect):
    lines = [line for line, want in cases.expected(dialect) if want[0] != "error"]
    assert len(lines) >= 40
    _against_host(host, tmp_path, cases.NAMES, lines, dialect, "table")
    # each error of the table, alone in a file: the host parser fails with the oracle's message
    if dialect == bo.INTERSECT:
        gff, order = make_index(host, tmp_path, cases.NAMES)
        for line, want in cases.expected(dialect):
            if want[0] != "error":
                continue
            bed = str(tmp_path / "bad.bed")
            open(bed, "wb").write(b"chr1\t1\t2\n" + line + b"\nchr1\t3\t4\n")
            got, msg = _host_rows(host, host.gffx_host_parse_bed_file, gff, bed)
            assert got is None, line
            assert msg == bo.run(open(bed, "rb").read(), dialect, order)[2], line


def test_the_generator_meets_its_condition():
    for dialect in (bo.INTERSECT, bo.DEPTH):
        bo.check_generated(bo.generate(20000, 11, dialect), dialect)
    bo.check_generated(bo.generate(2000, 12, bo.INTERSECT, errors=True), bo.INTERSECT, errors=True)


@pytest.mark.parametrize("dialect", [bo.INTERSECT, bo.DEPTH])
def test_oracle_equals_the_host_parser_on_generated_lines(host, tmp_path, dialect):
    lines = bo.generate(20000, 11, dialect)
    bo.check_generated(lines, dialect)
    _against_host(host, tmp_path, bo.GEN_NAMES, lines, dialect, "gen")
