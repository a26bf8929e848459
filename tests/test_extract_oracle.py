"""The Python restatement of `gffx extract` (tests/_extract_oracle.py) against answers derived by hand from the seven feature
lines of tests/golden/appendix_e.gff (tests/golden/appendix_e_extract.json), and its small rules one by one.  No GPU."""
import json
import os

import pytest

import _extract_oracle as xo


@pytest.fixture(scope="module")
def fixture(golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "appendix_e_extract.json")))
    gff = open(os.path.join(golden_dir, fx["gff"]), "rb").read()
    by_key = {k: l + b"\n" for k, l in zip(fx["line_order"], gff.split(b"\n")[:-1])}
    return fx, gff, xo.build_index(gff), by_key


def names_of(args):
    if "feature_id" in args:
        return [args["feature_id"]]
    return xo.read_feature_file("".join(n + "\n" for n in args["feature_list"]).encode())


def test_every_case_is_given_with_and_without_entire_group(fixture):
    fx = fixture[0]
    keys = [(json.dumps({k: v for k, v in c["args"].items() if k != "entire_group"}, sort_keys=True), bool(c["args"].get("entire_group")))
            for c in fx["cases"]]
    for k, _ in keys:
        assert (k, False) in keys and (k, True) in keys


def test_hand_derived_answers(fixture):
    fx, gff, B, by_key = fixture
    assert len(fx["cases"]) >= 10
    for case in fx["cases"]:
        a = case["args"]
        out, missing, invalid = xo.extract_run(gff, B, names_of(a), bool(a.get("entire_group")), a.get("types"))
        assert out == b"".join(by_key[k] for k in case["stdout"]), case
        assert missing == case["missing"] and invalid == [], case


def test_name_list_rules():
    data = b"a\r\n  b \n\n\xe2\x80\x83c\xc2\xa0\na\nb\r"  # CRLF, blanks, an empty line, Unicode blanks, duplicates, no final newline
    assert xo.read_feature_file(data) == ["a", "b", "c"]
    assert xo.read_feature_file(b"") == [] and xo.read_feature_file(b"\n\n") == []
    with pytest.raises(UnicodeDecodeError):
        xo.read_feature_file(b"ok\n\xff\xfe\n")


def test_last_line_of_an_id_wins_and_the_chase_is_bounded():
    assert xo.fts_index(["a", "b", "a", "c", "a"]) == {"a": 4, "b": 1, "c": 3}
    prt = [0, 0, 1, 2, 9, 6, 5, 8, 9, 7]  # 0 <- 1 <- 2 <- 3; 4 -> 9 (in range) ...; 5 <-> 6 a 2-cycle; 7 -> 8 -> 9 -> 7 a 3-cycle
    assert [xo.resolve_root(prt, f) for f in (0, 1, 3)] == [0, 0, 0]
    assert all(xo.resolve_root(prt, f) == xo.NONE for f in (4, 5, 6, 7, 8, 9, 10, 2**32 - 1))
    assert xo.resolve_root([0, 7], 1) == xo.NONE  # a parent >= n
    assert xo.resolve_root([], 0) == xo.NONE


def test_line_rules():
    keep = {"b", "x", "y"}
    nine = b"c\ts\texon\t1\t2\t.\t+\t.\t"
    assert xo.keeps_line(nine + b"ID=b;Parent=z\n", keep, None)
    assert not xo.keeps_line(nine + b"geneID=a;ID=b\n", keep, None)  # the FIRST `ID=`: the value is a
    assert xo.keeps_line(nine + b"geneID=x;ID=q\n", keep, None)
    assert xo.keeps_line(nine + b"Parent=z;ID=y", keep, None) and xo.keeps_line(nine + b"ID=y\r\n", keep, None)
    assert not xo.keeps_line(b"#" + nine + b"ID=b\n", keep, None)
    assert not xo.keeps_line(b"c\ts\texon\t1\t2\t.\t+\tID=b\n", keep, None)  # seven TABs
    assert not xo.keeps_line(nine + b"Name=b\n", keep, None)
    assert xo.keeps_line(nine + b"Note=a\tID=b\n", keep, None)  # a TAB inside the attribute field belongs to it
    allow = xo.split_types(" exon , CDS,,\t")
    assert allow == {"exon", "CDS"} and xo.split_types(",") == set()
    assert xo.keeps_line(nine + b"ID=b\n", keep, allow) and not xo.keeps_line(nine.replace(b"exon", b"gene") + b"ID=b\n", keep, allow)
    assert not xo.keeps_line(nine + b"ID=b\n", keep, set())
    assert not xo.keeps_line(b"c\ts\texon", keep, allow)  # two TABs


def test_an_id_that_two_blocks_carry_is_kept_only_in_the_block_of_its_last_line():
    gff = (b"c\ts\tgene\t1\t9\t.\t+\t.\tID=g1\n" b"c\ts\tCDS\t1\t3\t.\t+\t.\tID=dup;Parent=g1\n"
           b"c\ts\tgene\t11\t19\t.\t+\t.\tID=g2\n" b"c\ts\tCDS\t11\t13\t.\t+\t.\tID=dup;Parent=g2\n")
    B = xo.build_index(gff)
    lines = gff.split(b"\n")
    out, missing, invalid = xo.extract_run(gff, B, ["dup"], False, None)
    assert out == lines[3] + b"\n" and not missing and not invalid
    out, _, _ = xo.extract_run(gff, B, ["dup"], True, None)
    assert out == lines[2] + b"\n" + lines[3] + b"\n"
