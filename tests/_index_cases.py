"""Inputs and hand-worked answers of the `gffx index --gpu` tests (tests/test_index_device_cpu.py, test_index_device_gpu.py): single
lines with the outcome the reference's line loop (index_builder/core.rs:71-138) gives them, whole files with the arrays of
core.rs:141-203 written out, and the generators of the larger GPU cases.  The expected values here are worked by hand from
the rules; oracle.gffx_oracle_py.build_index is the second, independent reference."""
import dataclasses

from oracle import gffx_oracle_py as opy

DEFAULT_SKIP = "remark,note,comment,region,gap,assembly_gap,contig,scaffold,source"
NONE = 0xFFFFFFFF


def L(*cols) -> bytes:
    return b"\t".join(c if isinstance(c, bytes) else c.encode() for c in cols)


def feat(seq="chr1", ty="gene", s="10", e="20", attrs="ID=g1;gene_name=A", src="src") -> bytes:
    return L(seq, src, ty, s, e, ".", "+", ".", attrs)


def row(start, end, id_, seq=b"chr1", parent=None, attr=None, warn=0):
    return ("row", start, end, warn, seq, id_, parent, attr)


NBSP = " ".encode()
IDSP = "　".encode()

# (name, line without '\n', attribute key, skip string, expected): expected is a status name or row(...)
LINE_CASES = [
    ("plain", feat(), "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),
    ("empty", b"", "gene_name", DEFAULT_SKIP, "blank"),
    ("comment", b"# ID=x", "gene_name", DEFAULT_SKIP, "blank"),
    ("comment_with_bad_utf8", b"#\xff\xfe", "gene_name", DEFAULT_SKIP, "blank"),  # '#' is tested before UTF-8
    ("white_space_only", b" \t" + NBSP + IDSP + b"\r", "gene_name", DEFAULT_SKIP, "blank"),
    ("leading_tab_trimmed", b"\t" + feat(), "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),  # 10 raw fields, 9 after the trim
    ("trailing_tab_trimmed", feat() + b"\t", "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),
    ("empty_last_column_trimmed_away", L("chr1", "src", "gene", "10", "20", ".", "+", ".", ""), "gene_name", DEFAULT_SKIP, "COLUMNS"),
    ("leading_nbsp_and_tab", NBSP + b"\t" + feat(), "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),
    ("trailing_nbsp", feat(attrs="ID=g1") + NBSP, "gene_name", DEFAULT_SKIP, row(9, 20, b"g1")),
    ("eight_columns", L("chr1", "src", "gene", "10", "20", ".", "+", "ID=g1"), "gene_name", DEFAULT_SKIP, "COLUMNS"),
    ("ten_columns", feat() + b"\textra", "gene_name", DEFAULT_SKIP, "COLUMNS"),
    ("trailing_cr", feat() + b"\r", "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),
    ("hash_after_spaces_is_no_comment", b"  #comment", "gene_name", DEFAULT_SKIP, "COLUMNS"),
    ("plus_in_start", feat(s="+12"), "gene_name", DEFAULT_SKIP, row(11, 20, b"g1", attr=b"A")),
    ("plus_alone", feat(s="+"), "gene_name", DEFAULT_SKIP, "DIGITS"),
    ("minus", feat(s="-1"), "gene_name", DEFAULT_SKIP, "DIGITS"),
    ("empty_start", feat(s=""), "gene_name", DEFAULT_SKIP, "DIGITS"),
    ("two_to_the_32", feat(s="4294967296", e="4294967297"), "gene_name", DEFAULT_SKIP, "DIGITS"),
    ("largest_u32", feat(s="1", e="4294967295"), "gene_name", DEFAULT_SKIP, row(0, 4294967295, b"g1", attr=b"A")),
    ("leading_zeros", feat(s="0000000000012", e="0000000000000000000020"), "gene_name", DEFAULT_SKIP, row(11, 20, b"g1", attr=b"A")),
    ("end_zero", feat(s="5", e="0"), "gene_name", DEFAULT_SKIP, "zero_end"),
    ("end_zero_before_the_id_check", feat(s="5", e="0", attrs="x=1"), "gene_name", DEFAULT_SKIP, "zero_end"),
    ("start_after_end", feat(s="20", e="10"), "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),
    ("start_zero", feat(s="0", e="5"), "gene_name", DEFAULT_SKIP, row(0, 5, b"g1", attr=b"A")),
    ("end_zero_swapped_would_be_start", feat(s="0", e="0"), "gene_name", DEFAULT_SKIP, "zero_end"),
    ("geneID_matches_ID", feat(attrs="geneID=x;ID=y"), "gene_name", DEFAULT_SKIP, row(9, 20, b"x")),
    ("empty_id_goes_on", feat(attrs="ID=;ID=z"), "gene_name", DEFAULT_SKIP, row(9, 20, b"z")),
    ("id_at_the_very_end_is_empty", feat(attrs="x=1;ID="), "gene_name", DEFAULT_SKIP, "NO_ID"),
    ("no_id", feat(attrs="Name=x"), "gene_name", DEFAULT_SKIP, "NO_ID"),
    ("id_in_column_1", feat(seq="ID=c", attrs="Name=x"), "gene_name", DEFAULT_SKIP, row(9, 20, b"c", seq=b"ID=c")),
    ("id_ended_by_u3000", feat(attrs=b"ID=g1" + IDSP + b"x;gene_name=A"), "gene_name", DEFAULT_SKIP, row(9, 20, b"g1", attr=b"A")),
    ("id_ended_by_space", feat(attrs="ID=g 1;Parent=p q"), "gene_name", DEFAULT_SKIP, row(9, 20, b"g", parent=b"p")),
    ("parent_comma_list", feat(attrs="ID=t1;Parent=a,b"), "gene_name", DEFAULT_SKIP, row(9, 20, b"t1", parent=b"a,b")),
    ("key_inside_column_2", feat(src="gene_name=src", attrs="ID=g;gene_name=A"), "gene_name", DEFAULT_SKIP,
     row(9, 20, b"g", attr=b"src\tgene\t10\t20\t.\t+\t.\tID=g")),
    ("value_with_space", feat(attrs="ID=g;gene_name=A b;x=1"), "gene_name", DEFAULT_SKIP, row(9, 20, b"g", attr=b"A b", warn=1)),
    ("value_with_comma", feat(attrs="ID=g;gene_name=A,b"), "gene_name", DEFAULT_SKIP, row(9, 20, b"g", attr=b"A,b", warn=1)),
    ("value_runs_to_the_end", feat(attrs="ID=g;gene_name=A　b"), "gene_name", DEFAULT_SKIP, row(9, 20, b"g", attr="A　b".encode())),
    ("key_is_ID", feat(attrs="ID=g 1"), "ID", DEFAULT_SKIP, row(9, 20, b"g", attr=b"g 1", warn=1)),
    ("truncated_utf8_at_the_end", feat(attrs="ID=g1") + b"\xe3\x80", "gene_name", DEFAULT_SKIP, "BAD_UTF8"),
    ("overlong_utf8_at_the_end", feat(attrs="ID=g1") + b"\xc0\xaf", "gene_name", DEFAULT_SKIP, "BAD_UTF8"),
    ("surrogate", feat(attrs="ID=g1;x=") + b"\xed\xa0\x80", "gene_name", DEFAULT_SKIP, "BAD_UTF8"),
    ("four_byte_char", feat(attrs="ID=g\U0001F600;x=1"), "gene_name", DEFAULT_SKIP, row(9, 20, "g\U0001F600".encode())),
    ("bad_utf8_before_columns", b"chr1\t\xff", "gene_name", DEFAULT_SKIP, "BAD_UTF8"),
    ("skipped_type", feat(ty="region", s="x"), "gene_name", DEFAULT_SKIP, ("skipped_type", b"region")),  # before the digits
    ("skip_list_is_not_trimmed", feat(ty="gene"), "gene_name", "exon, gene", row(9, 20, b"g1", attr=b"A")),
    ("skip_list_with_empty_member", feat(ty=""), "gene_name", "a,,b", ("skipped_type", b"")),
    ("empty_type_not_in_list", feat(ty=""), "gene_name", "a,b", row(9, 20, b"g1", attr=b"A")),
    ("empty_skip_string_is_one_empty_member", feat(ty=""), "gene_name", "", ("skipped_type", b"")),
]

# ---- whole files: (name, text, key, hash_bits to try, expected Built fields) ----------------------------------------------
_F1 = b"".join(x + b"\n" for x in [
    b"##gff-version 3",
    feat("chr1", "gene", "100", "200", "ID=g1;gene_name=A"),            # row 0: an earlier duplicate of g1 -> fid 3; has no Parent -> root
    feat("chr1", "mRNA", "100", "200", "ID=t1;Parent=g1;gene_name=A"),  # row 1: Parent g1 -> 3
    feat("chr2", "exon", "100", "150", "ID=e1;Parent=t2;gene_name=B"),  # row 2: Parent names a LATER line (row 5); chr2 first seen on a non-root
    feat("chr3", "gene", "300", "400", "ID=g1;gene_name=C"),            # row 3: the last g1: root, seqid chr3 numbered 1
    feat("chr1", "region", "1", "1000", "ID=r1"),                       # skipped by type
    feat("chr3", "gene", "500", "600", "ID=s1;Parent=s1;gene_name=A"),  # row 4: Parent is the row's own ID -> root
    feat("chr2", "mRNA", "100", "200", "ID=t2;Parent=nowhere"),         # row 5: Parent unseen -> root; chr2 numbered 2 here
    feat("chr1", "gene", "7", "0", "ID=z"),                             # end == 0: skipped
    feat("chr1", "CDS", "120", "110", "ID=c1;Parent=g1,t1;gene_name=B"),  # row 6: a comma list finds nothing -> root
])
_off1 = [0]
for _ln in _F1.split(b"\n")[:-1]:
    _off1.append(_off1[-1] + len(_ln) + 1)
_rows1 = [1, 2, 3, 4, 6, 7, 9]  # the lines that are rows
FILE_1 = dict(
    text=_F1, key="gene_name", skip=DEFAULT_SKIP,
    ids=["g1", "t1", "e1", "g1", "s1", "t2", "c1"],
    fid=[3, 1, 2, 3, 4, 5, 6],
    prt=[3, 3, 5, 3, 4, 5, 6],
    a2f=[0, 0, 1, 2, 0, NONE, 1],
    atn=["A", "B", "C"],
    seqids=["chr1", "chr3", "chr2"],
    # roots: rows 0 (fid 3!), 3, 4, 5, 6
    gof=[(3, 0, _off1[1], _off1[4]), (3, 1, _off1[4], _off1[6]), (4, 1, _off1[6], _off1[7]), (5, 2, _off1[7], _off1[9]),
         (6, 0, _off1[9], len(_F1))],
    trees_input=[[(99, 200, 3), (109, 120, 6)], [(299, 400, 3), (499, 600, 4)], [(99, 200, 5)]],
    counts=dict(lines=10, blank=1, skipped_type=1, zero_end=1, rows=7, roots=5, seqids=3, attr_values=3),
)
FILE_CASES = [FILE_1]


def built_tuple(b):
    """the eight fields of an oracle Built or an engine GffBuilt, comparable"""
    if dataclasses.is_dataclass(b):
        return (b.ids, b.fid, b.prt, b.a2f, b.atn, b.seqids, b.gof, b.trees_input)
    return b.astuple()


def oracle_outcome(text: bytes, key: str, skip: str):
    """("ok", Built) or ("error", kind) from the Python restatement"""
    try:
        return "ok", opy.build_index(text, key, skip)
    except UnicodeDecodeError:
        return "error", "BAD_UTF8"
    except ValueError as e:
        m = str(e)
        if m.startswith("Invalid GFF line"):
            return "error", "COLUMNS"
        if m.startswith("Missing ID"):
            return "error", "NO_ID"
        if m.startswith("invalid digit") or m.startswith("number too large"):
            return "error", "DIGITS"
        raise


# ---- generators of the GPU cases ---------------------------------------------------------------------------------------------
def gene_line(i: int, seq: str = "chr1", parent=None, name=None, ty="gene", id_=None) -> bytes:
    a = "ID=%s" % (id_ if id_ is not None else "f%d" % i)
    if parent is not None:
        a += ";Parent=%s" % parent
    if name is not None:
        a += ";gene_name=%s" % name
    return feat(seq, ty, str(10 * i + 1), str(10 * i + 9), a)


def family_file(n_genes: int, seqs: int = 3, kids: int = 2, dup_every: int = 0, blank_every: int = 0) -> bytes:
    """genes with `kids` children each; every dup_every-th gene repeats an earlier gene's ID; children of odd genes come
    BEFORE their gene (a Parent that names a later line)"""
    out = [b"##gff-version 3"]
    for g in range(n_genes):
        seq = "chr%d" % (g % seqs)
        gid = "g%d" % (g - dup_every if dup_every and g % dup_every == dup_every - 1 and g >= dup_every else g)
        gene = feat(seq, "gene", str(100 * g + 1), str(100 * g + 90), "ID=%s;gene_name=N%d" % (gid, g % 50))
        ch = [feat(seq, "mRNA", str(100 * g + 1 + k), str(100 * g + 50 + k), "ID=t%d_%d;Parent=%s;gene_name=N%d" % (g, k, gid, g % 50))
              for k in range(kids)]
        out += (ch + [gene]) if g % 2 else ([gene] + ch)
        if blank_every and g % blank_every == 0:
            out += [b"", b"# note", feat(seq, "region", "1", "5", "ID=r%d" % g)]
    return b"\n".join(out) + b"\n"
