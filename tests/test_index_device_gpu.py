"""`gffx index --gpu` on the device: the C-ABI (gffx_hip_gff_*) and engine.GffIndexer against the Python restatement of the
reference's index builder (oracle.gffx_oracle_py.build_index) and the hand-worked arrays of tests/_index_cases.py, and the
command line against the host path of the same binary, file by file, byte for byte.  Every case is a few thousand lines at
most, except the one that crosses 2^16 distinct values."""
import os
import subprocess

import pytest

import _index_cases as ic
from gffx_amd import _ffi, engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
SIDE_CARS = (".fts", ".prt", ".a2f", ".atn", ".sqs", ".gof", ".rit", ".rix")

_oracle_cache = {}


def _oracle(text, key="gene_name", skip=ic.DEFAULT_SKIP):
    k = (text, key, skip)
    if k not in _oracle_cache:
        _oracle_cache[k] = ic.oracle_outcome(text, key, skip)
    return _oracle_cache[k]


def _check(text, key="gene_name", skip=ic.DEFAULT_SKIP, **kw):
    """the device's arrays of `text` equal the restatement's; returns the handle's counts"""
    kind, want = _oracle(text, key, skip)
    assert kind == "ok"
    g = engine.gff_index(text, key, skip, **kw)
    try:
        got = g.built()
        for name, a, b in zip(engine.GffBuilt.FIELDS, got.astuple(), ic.built_tuple(want)):
            assert a == b, "%s differs (%r)" % (name, kw)
        assert got.fid == want.fid
        c = g.counts
        assert (c["rows"], c["roots"], c["seqids"], c["attr_values"]) == (len(want.ids), len(want.gof), len(want.seqids), len(want.atn))
        assert c["lines"] == text.count(b"\n") + (0 if text.endswith(b"\n") or not text else 1)
        assert c["lines"] == c["blank"] + c["skipped_type"] + c["zero_end"] + c["rows"]
        return c
    finally:
        g.close()


def test_single_lines_of_the_hand_worked_table():
    for name, line, key, skip, want in ic.LINE_CASES:
        g = engine.GffIndexer(key, skip)
        try:
            if want in ("BAD_UTF8", "COLUMNS", "DIGITS", "NO_ID"):
                with pytest.raises(_ffi.GffxHipError):
                    g.feed(line + b"\n")
                    g.finish()
                assert g.error() == (0, want), name
                continue
            g.feed(line + b"\n")
            g.finish()
            c, b = g.counts, g.built()
            if isinstance(want, tuple) and want[0] == "row":
                assert b.ids == [want[5].decode()] and b.seqids == [want[4].decode()], name
                assert b.trees_input == [[(want[1], want[2], 0)]] and b.prt == [0], name
                assert b.atn == ([want[7].decode()] if want[7] is not None else []), name
                assert g.warn_rows().tolist() == ([0] if want[3] else []), name
            else:
                tally = want[0] if isinstance(want, tuple) else want
                assert c["rows"] == 0 and c[tally] == 1 and b.gof == [], name
                assert g.skipped_lines().tolist() == ([0] if tally == "skipped_type" else []), name
        finally:
            g.close()


@pytest.mark.parametrize("hash_bits", [-1, 0, 2])
def test_hand_worked_file(hash_bits):
    fc = ic.FILE_1
    g = engine.gff_index(fc["text"], fc["key"], fc["skip"], hash_bits=hash_bits)
    try:
        b = g.built()
        for k in engine.GffBuilt.FIELDS:
            assert getattr(b, k) == fc[k], k
        assert g.counts == fc["counts"]
        assert g.fts() == "".join(i + "\n" for i in fc["ids"]).encode()
    finally:
        g.close()


# ---- a. tile shapes ------------------------------------------------------------------------------------------------------------
def _tile_text(prefix: bytes) -> bytes:
    out = bytearray(prefix)
    n = [0]

    def line_to(end):  # a feature line whose '\n' is byte end - 1
        n[0] += 1
        base = ic.gene_line(n[0], "chr%d" % (n[0] % 3), name="pad")
        assert end - len(out) - 1 >= len(base)
        out.extend(base + b"x" * (end - len(out) - 1 - len(base)) + b"\n")

    def long_line(length):
        n[0] += 1
        base = ic.gene_line(n[0], "chr1", name="long")
        out.extend(base + b";note=" + b"y" * (length - len(base) - 7) + b"\n")

    t = 4096
    line_to(t + len(prefix))   # its '\n' at 4095 (4096 / 4097 with a prefix of one / two bytes)
    out.extend(b"\n" * 64)     # tile 1: 64 line ends, then the start of a line that ends in tile 2 (1 line end there)
    long_line(5000)
    line_to(3 * t + len(prefix))
    out.extend(b"\n" * 65)     # 65 line ends
    long_line(5000)
    line_to(5 * t + len(prefix))
    out.extend(b"#\n" * 100 + b"\n" * 40)  # 140 line ends in 240 bytes
    long_line(9000)            # ... and a tile without any
    for i in range(40):
        out.extend(ic.gene_line(1000 + i, "chr2", parent="f1", name="N%d" % (i % 7)) + b"\n")
    return bytes(out)


@pytest.mark.parametrize("prefix", [b"", b"\n", b"#\n"])
def test_tile_shapes(prefix):
    text = _tile_text(prefix)
    assert text[4095 + len(prefix)] == 0x0A
    _check(text)
    _check(text, chunk_bytes=4096)
    _check(text[:-1], chunk_bytes=4097)


# ---- b. long lines ---------------------------------------------------------------------------------------------------------------
def test_a_64_kib_attribute_column_and_a_line_of_a_megabyte():
    short = ic.family_file(30)
    col = ic.feat(attrs="ID=big;gene_name=" + "v" * 65536 + ";Parent=g3")
    mega = ic.feat(attrs="ID=mega;note=" + "z" * (1 << 20) + ";gene_name=tail;Parent=g2")
    text = short + col + b"\n" + short[:0] + mega + b"\n" + ic.gene_line(77, parent="mega", name="tail") + b"\n"
    c = _check(text)
    assert c["rows"] == 30 * 3 + 3
    _check(text, chunk_bytes=100000)  # both lines are longer than a pass


# ---- c. chunk splits ---------------------------------------------------------------------------------------------------------
FAMILY = ic.family_file(40, seqs=4, kids=2, dup_every=5, blank_every=6)


@pytest.mark.parametrize("chunk", [32, 100, 4096])
def test_chunks_end_inside_every_column(chunk):
    _check(FAMILY, chunk_bytes=chunk)           # (32: every line is longer than a chunk)
    _check(FAMILY[:-1], chunk_bytes=chunk)      # a last line without '\n'
    _check(FAMILY, chunk_bytes=chunk, feed_bytes=chunk + 7)


def test_feeds_cut_anywhere_and_empty_feeds():
    kind, want = _oracle(FAMILY)
    g = engine.GffIndexer(chunk_bytes=256)
    try:
        g.feed(b"")
        at = 0
        for step in (1, 2, 3, 5, 300, 1, 0, 1000, 7, len(FAMILY)):
            g.feed(FAMILY[at:at + step])
            at += step
        g.feed(b"")
        g.finish()
        assert g.built().astuple() == ic.built_tuple(want)
    finally:
        g.close()


def test_an_empty_file_and_a_file_of_comments():
    for text in (b"", b"##gff-version 3\n# a\n\n#b", b"\n\n\n"):
        g = engine.gff_index(text, chunk_bytes=8)
        try:
            b, c = g.built(), g.counts
            assert b.astuple() == ([], [], [], [], [], [], [], []) and g.gof() == b"" and g.fts() == b""
            assert c["rows"] == 0 and c["lines"] == c["blank"] == text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
        finally:
            g.close()


# ---- d. the finish steps across chunks -------------------------------------------------------------------------------------------
def test_partners_in_different_chunks():
    # the child, its later parent, the duplicate of that parent's ID and the second use of a seqid and of a value: each more than a chunk apart
    filler = b"".join(ic.gene_line(100 + i, "chrF", name="fill%d" % (i % 3)) + b"\n" for i in range(20))
    text = (ic.gene_line(1, "chrA", parent="p", name="V") + b"\n" + filler + ic.gene_line(2, "chrB", id_="p", name="W") + b"\n" + filler +
            ic.gene_line(3, "chrA", id_="p", name="V") + b"\n" + filler + ic.gene_line(4, "chrB", parent="f1", name="W") + b"\n")
    for chunk in (64, 200, 0):
        _check(text, chunk_bytes=chunk)


def test_257_seqids():
    text = b"".join(ic.gene_line(i, "s%03d" % ((i * 7) % 257), name="n%d" % (i % 300)) + b"\n" for i in range(600))
    assert _check(text, chunk_bytes=1000)["seqids"] == 257


def test_70000_rows_with_66000_values():
    text = b"".join(ic.feat("c%d" % (i % 5), "gene", str(i + 1), str(i + 5), "ID=f%d;gene_name=v%d" % (i, i % 66000)) + b"\n" for i in range(70000))
    c = _check(text, chunk_bytes=1 << 20)
    assert (c["rows"], c["attr_values"]) == (70000, 66000)


def test_hash_bits_give_equal_results():
    text = ic.family_file(60, seqs=7, kids=1, dup_every=4)
    for hb in (0, 2, -1):
        _check(text, hash_bits=hb, chunk_bytes=512)


# ---- e. errors ---------------------------------------------------------------------------------------------------------------------
BAD = {"BAD_UTF8": ic.feat(attrs="ID=x") + b"\xff", "COLUMNS": b"chr1\tonly", "DIGITS": ic.feat(s="1e3"), "NO_ID": ic.feat(attrs="Name=q")}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_one_bad_line_behind_good_ones(kind):
    good = ic.family_file(12)
    text = good + BAD[kind] + b"\n" + good
    assert _oracle(text) == ("error", kind)
    for chunk in (256, 0):
        g = engine.GffIndexer(chunk_bytes=chunk)
        try:
            with pytest.raises(_ffi.GffxHipError):
                g.feed(text)
                g.finish()
            assert g.error() == (len(good), kind)
            # the handle stays failed and copies nothing out
            with pytest.raises(_ffi.GffxHipError) as e1:
                g.feed(b"\n")
            with pytest.raises(_ffi.GffxHipError) as e2:
                g.finish()
            assert str(e1.value) == str(e2.value) and kind in str(e1.value)
            assert _ffi.lib().gffx_hip_gff_n_rows(g._h) == 0 and _ffi.lib().gffx_hip_gff_fts_bytes(g._h) == 0
            with pytest.raises(_ffi.GffxHipError):
                g.fts()
            with pytest.raises(_ffi.GffxHipError):
                g.prt()
        finally:
            g.close()


def test_the_earlier_of_two_bad_lines_whatever_the_chunking():
    good = ic.family_file(6)
    for first, second in (("NO_ID", "COLUMNS"), ("DIGITS", "BAD_UTF8"), ("BAD_UTF8", "NO_ID"), ("COLUMNS", "DIGITS")):
        text = good + BAD[first] + b"\n" + BAD[second] + b"\n" + good + BAD[second]
        for chunk in (48, 4096, 0):
            g = engine.GffIndexer(chunk_bytes=chunk)
            try:
                with pytest.raises(_ffi.GffxHipError):
                    g.feed(text)
                    g.finish()
                assert g.error() == (len(good), first), (first, second, chunk)
            finally:
                g.close()


# ---- f. the command line against the host path --------------------------------------------------------------------------------
CLI_TEXT = (ic.family_file(50, seqs=4, kids=2, dup_every=6, blank_every=5) +
            ic.feat("chr9", "gene", "5", "50", "ID=w1;gene_name=two words;x=1") + b"\n" +
            ic.feat("chr9", "note", "5", "50", "ID=n1") + b"\n" +
            ic.feat("chr9", "mRNA", "5", "50", "ID=w2;Parent=w1;gene_name=a,b") + b"\n")


def _index_both(tmp_path, text, args=(), env=None, name="t.gff"):
    """`gffx index` and `gffx index --gpu` on copies of the text in two directories: (host run, device run, host path, device path)"""
    out = []
    for sub, extra in (("host", []), ("gpu", ["--gpu"])):
        d = tmp_path / sub
        d.mkdir(exist_ok=True)
        p = d / name
        p.write_bytes(text)
        os.utime(p, ns=(10 ** 18, 10 ** 18))  # (the key of .lsoa / .lall holds the text's size and mtime)
        r = subprocess.run([GFFX, "index", "-i", str(p)] + list(args) + extra, capture_output=True, env=dict(os.environ, **(env or {})))
        out.append((r, str(p)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _same_files(a, b, suffixes):
    for s in suffixes:
        assert os.path.exists(a + s) and os.path.exists(b + s), s
        assert open(a + s, "rb").read() == open(b + s, "rb").read(), s


def _lall_same(a, b):
    _same_files(a, b, (".lsoa", ".lall"))  # built after the side-cars, from the text and .gof, exactly as today


@pytest.mark.parametrize("args,env", [(["-v"], None), (["-a", "ID"], None), (["-s", "mRNA,,note", "-v"], None),
                                      ([], {"GFFX_INDEX_CHUNK_BYTES": "64"})])
def test_cli_side_cars_equal_the_host_paths(tmp_path, args, env):
    rh, rg, ph, pg = _index_both(tmp_path, CLI_TEXT, args, env)
    assert rh.returncode == 0 and rg.returncode == 0, rg.stderr
    _same_files(ph, pg, SIDE_CARS)
    _lall_same(ph, pg)
    pick = lambda b, w: [ln for ln in b.split(b"\n") if ln.startswith(w)]  # noqa: E731
    assert pick(rh.stdout, b"skip comment feature") == pick(rg.stdout, b"skip comment feature")
    assert pick(rh.stderr, b"[WARN] Attribute") == pick(rg.stderr, b"[WARN] Attribute")
    if "-v" in args:
        assert len(pick(rg.stdout, b"skip comment feature")) > 0
    if not args or args == ["-v"]:
        assert len(pick(rg.stderr, b"[WARN] Attribute")) == 2


@pytest.mark.parametrize("fixture", ["appendix_e.gff", "rit_fixture.gff"])
def test_cli_golden_files(tmp_path, golden_dir, fixture):
    text = open(os.path.join(golden_dir, fixture), "rb").read()
    rh, rg, ph, pg = _index_both(tmp_path, text, name=fixture)
    assert rh.returncode == 0 and rg.returncode == 0, rg.stderr
    _same_files(ph, pg, SIDE_CARS)
    _lall_same(ph, pg)


@pytest.mark.parametrize("kind", sorted(BAD))
def test_cli_errors_equal_the_host_paths(tmp_path, kind):
    text = ic.family_file(8) + BAD[kind] + b"\n" + ic.family_file(3) + BAD["COLUMNS" if kind != "COLUMNS" else "NO_ID"] + b"\n"
    rh, rg, ph, pg = _index_both(tmp_path, text, env={"GFFX_INDEX_CHUNK_BYTES": "512"})
    assert rh.returncode != 0 and rg.returncode == rh.returncode
    assert rg.stderr == rh.stderr and rg.stderr != b""
    assert sorted(os.listdir(os.path.dirname(pg))) == ["t.gff"]  # nothing is written


def test_intersect_and_extract_over_the_device_built_index(tmp_path):
    rh, rg, ph, pg = _index_both(tmp_path, CLI_TEXT)
    assert rh.returncode == 0 and rg.returncode == 0, rg.stderr
    for cmd in (["intersect", "-r", "chr1:1-3000"], ["extract", "-f", "t4_1"]):
        outs = [subprocess.run([GFFX, cmd[0], "-i", p] + cmd[1:], capture_output=True) for p in (ph, pg)]
        assert outs[0].returncode == 0 and outs[1].returncode == 0, outs[1].stderr
        assert outs[0].stdout == outs[1].stdout and len(outs[0].stdout) > 0
