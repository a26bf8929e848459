"""The Python restatement of `gffx search` (tests/_search_oracle.py) against answers derived by hand from the reference's source
text (tests/golden/appendix_e_search.json): what every other search test compares the product with is pinned here first."""
import json
import os

import pytest

import _search_oracle as so


@pytest.fixture(scope="module")
def fx(golden_dir):
    f = json.load(open(os.path.join(golden_dir, "appendix_e_search.json"), encoding="utf-8"))
    data = open(os.path.join(golden_dir, f["gff"]), "rb").read()
    return f, data, so.build_index(data)


def test_the_index_the_derivations_start_from(fx):
    f, data, B = fx
    assert B.ids == f["fids"] and list(B.prt) == f["prt"] and list(B.a2f) == f["a2f"]
    assert so.atn_bytes("gene_name", B.atn).decode() == f["atn"]
    assert so.load_atn(f["atn"].encode()) == ("gene_name", ["A", "B", "C"])
    assert so.load_a2f(b"".join(a.to_bytes(4, "little") for a in f["a2f"])) == f["a2f"]


def test_known_answers(fx):
    f, data, B = fx
    by_key = {k: l + b"\n" for k, l in zip(f["line_order"], data.split(b"\n")[:-1])}
    seen = set()
    for case in f["cases"]:
        a = case["args"]
        name, values = so.load_atn(case.get("atn", f["atn"]).encode())
        patterns = so.read_attr_list("".join(p + "\n" for p in a["attr_list"]).encode()) if "attr_list" in a else [a["attr"]]
        out, S = so.search_run(data, B.gof, name, values, case.get("a2f", f["a2f"]), case.get("prt", f["prt"]), patterns,
                               bool(a.get("regex")), bool(a.get("entire_group")), a.get("types"))
        assert out == b"".join(by_key[k] for k in case["stdout"]), case
        assert (S.bail is not None) == (case["exit"] == 1) and S.bail == case.get("error"), case
        assert [w.decode() for w in so.warn_lines(S)] == case.get("warn", []), case
        seen.add(case.get("name"))
    assert {"a value shared by two roots", "a value on a child only", "a repeated string and a # value line"} <= seen
    assert any("types" in c["args"] for c in f["cases"])


def test_load_atn_rules():
    bom = b"\xef\xbb\xbf"
    assert so.load_atn(bom + b"#attribute=x\r\n\n a \n#c\n\xc2\xa0b\xc2\xa0\nlast") == ("x", ["a", "b", "last"])
    assert so.load_atn(b"v0\n" + bom + b"v1\n#attribute=n\n" + bom + b"v2\n") == ("n", ["v0", "v1", "﻿v2"])  # a BOM only before the header
    for bad, msg in ((b"a\n", "Missing"), (b"#attribute=a\n#attribute=b\n", "Multiple"), (b"#attribute=a\n\xff\n", "invalid UTF-8")):
        with pytest.raises(ValueError, match=msg):
            so.load_atn(bad)
    with pytest.raises(ValueError, match="Corrupted A2F"):
        so.load_a2f(b"\x00" * 5)
    assert so.read_attr_list(b"a\r\n\n  b \nb\nc") == ["a", "b", "b", "c"]
