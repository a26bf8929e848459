"""The hand-worked table of the BED tests: one line (without its newline; the depth dialect reads it with one appended), and
what each dialect makes of it, worked out by hand from the rules in device/bed_core.hpp -- not computed.
K(seq, start, end): kept.  S(why): skipped.  E(kind): an error (intersect only; depth has none)."""

NAMES = [b"chr1", b"chr10", b"chrX", "chrü".encode(), b"L" * 1024]  # seqid 0 .. 4; chr1 is a prefix of chr10
LONG = NAMES[4]


def K(seq, start, end):
    return ("keep", seq, start, end)


def S(why):
    return ("skip", why)


def E(kind):
    return ("error", kind)


# (line, intersect, depth)
CASES = [
    # plain rows, signs, limits, zeros
    (b"chr1\t10\t20", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1\t+5\t9", K(0, 5, 9), K(0, 5, 9)),
    (b"chr1\t+0\t+1", K(0, 0, 1), K(0, 0, 1)),
    (b"chr1\t0\t4294967295", K(0, 0, 4294967295), K(0, 0, 4294967295)),
    (b"chr1\t0\t4294967296", E("coordinate"), S("coordinate")),
    (b"chr1\t1\t99999999999", E("coordinate"), S("coordinate")),
    (b"chr1\t0000000000001\t2", K(0, 1, 2), K(0, 1, 2)),
    (b"chr1\t00\t01", K(0, 0, 1), K(0, 0, 1)),
    (b"chr1\t\t5", S("fewfields"), S("fewfields")),  # an empty field is no field: two fields
    (b"chr1\t-1\t5", E("coordinate"), S("coordinate")),
    (b"chr1\t1e3\t5000", E("coordinate"), S("coordinate")),
    (b"chr1\t1_0\t50", E("coordinate"), S("coordinate")),
    (b"chr1\t+\t5", E("coordinate"), S("coordinate")),
    (b"chr1\t5\t+", E("coordinate"), S("coordinate")),
    (b"chr1\t++5\t9", E("coordinate"), S("coordinate")),
    (b"chr1\t0x10\t32", E("coordinate"), S("coordinate")),
    (b"chr1\t\xef\xbc\x91\t5", E("coordinate"), S("coordinate")),  # a fullwidth digit one: valid UTF-8, no digit
    # separators: \x0C and \r split only in intersect, \x0B in neither
    (b"chr1\x0c10\x0c20", K(0, 10, 20), S("fewfields")),
    (b"chr1\r10\r20", K(0, 10, 20), S("fewfields")),
    (b"chr1\x0b10\x0b20", S("fewfields"), S("fewfields")),
    (b"chr1 10 20", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1   10 \t 20  extra", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1\t10\t20\textra\tcols", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1\t10\t20 ", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1\t1\x0c\t2", K(0, 1, 2), S("coordinate")),  # depth: field 2 is "1\x0c", and only field 3 is trimmed
    (b"chr1\r\t1\t2", K(0, 1, 2), S("noseq")),         # depth: the name is "chr1\r"
    # the tail of field 3: depth trims Unicode White_Space, intersect splits on its four blanks only
    (b"chr1\t10\t20\x0c", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1\t10\t20\r", K(0, 10, 20), K(0, 10, 20)),  # CRLF
    (b"chr1\t10\t20\r\r", K(0, 10, 20), K(0, 10, 20)),
    (b"chr1\t10\t20\x0b", E("coordinate"), K(0, 10, 20)),
    (b"chr1\t10\t20\xc2\xa0", E("coordinate"), K(0, 10, 20)),      # NBSP
    (b"chr1\t10\t20\xc2\x85", E("coordinate"), K(0, 10, 20)),      # U+0085
    (b"chr1\t10\t20\xe2\x80\xa8", E("coordinate"), K(0, 10, 20)),  # U+2028
    (b"chr1\t10\t20\xe3\x80\x80", E("coordinate"), K(0, 10, 20)),  # U+3000
    (b"chr1\t1\t\xc2\xa0", E("coordinate"), S("coordinate")),      # nothing is left of field 3
    # blanks in front, comments, short lines
    (b" chr1\t10\t20", K(0, 10, 20), K(0, 10, 20)),
    (b"\tchr1\t10\t20", K(0, 10, 20), K(0, 10, 20)),
    (b" #x\t1\t2", S("noseq"), S("noseq")),  # the first byte is a blank: no comment, the name is "#x"
    (b"#chr1\t10\t20", S("comment"), S("comment")),
    (b"#", S("comment"), S("comment")),
    (b"", S("empty"), S("fewfields")),  # depth reads "\n": one field
    (b"chr1\t10", S("fewfields"), S("fewfields")),
    (b"chr1", S("fewfields"), S("fewfields")),
    (b"\t\t", S("fewfields"), S("fewfields")),
    (b"   ", S("fewfields"), S("fewfields")),
    # names
    (b"chrZ\tx\t5", S("noseq"), S("coordinate")),  # unknown name and bad coordinate: each dialect stops at its first rule
    (b"chrZ\t1\t5", S("noseq"), S("noseq")),
    (b"CHR1\t1\t2", S("noseq"), S("noseq")),
    (b"chr10\t1\t2", K(1, 1, 2), K(1, 1, 2)),
    (b"chr\t1\t2", S("noseq"), S("noseq")),
    (b"chr100\t1\t2", S("noseq"), S("noseq")),
    (b"chrX\t3\t4", K(2, 3, 4), K(2, 3, 4)),
    ("chrü\t3\t4".encode(), K(3, 3, 4), K(3, 3, 4)),
    (LONG + b"\t1\t2", K(4, 1, 2), K(4, 1, 2)),
    (LONG[:-1] + b"\t1\t2", S("noseq"), S("noseq")),
    (LONG + b"L\t1\t2", S("noseq"), S("noseq")),
    # start against end
    (b"chr1\t5\t5", K(0, 5, 5), S("nointerval")),
    (b"chr1\t7\t3", K(0, 7, 3), S("nointerval")),
    (b"chr1\t4294967295\t4294967295", K(0, 4294967295, 4294967295), S("nointerval")),
    # UTF-8: intersect validates the whole line first, depth the three fields only
    (b"chr1\t1\t2\ta\tb\tc\t\xff", E("utf8"), K(0, 1, 2)),  # column 7
    (b"chr\xff1\t1\t2", E("utf8"), S("fieldutf8")),
    (b"chr1\t1\xff\t2", E("utf8"), S("fieldutf8")),
    (b"chr1\t1\t2\xff", E("utf8"), S("fieldutf8")),
    (b"chr1\t1\t2\t\xc0\xaf", E("utf8"), K(0, 1, 2)),          # an overlong '/'
    (b"chr1\t1\t2\t\xed\xa0\x80", E("utf8"), K(0, 1, 2)),      # a surrogate
    (b"chr1\t1\t2\t\xf4\x90\x80\x80", E("utf8"), K(0, 1, 2)),  # U+110000
    (b"chr1\t1\t2\t\xe2\x82", E("utf8"), K(0, 1, 2)),          # a sequence cut at the line's end
    (b"chr1\t1\t2\xe2\x82", E("utf8"), S("fieldutf8")),        # the same in field 3
    (b"chr1\t\xff", E("utf8"), S("fewfields")),                # fewer than 3 fields AND invalid: UTF-8 is checked first
    (b"\xff", E("utf8"), S("fewfields")),
    (b"#\xff", S("comment"), S("comment")),                    # ... but after the comment test
]
assert len(CASES) >= 60


def expected(dialect: int):
    return [(line, i if dialect == 0 else d) for line, i, d in CASES]
