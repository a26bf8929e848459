"""A Python restatement of the two BED dialects (device/bed_core.hpp; the host parsers host/bed_parse.cpp and host/depth.cpp
are the specification): one line -> outcome, row and tally; a whole text -> rows, tallies and the first error.  Written
against Python's own UTF-8 decoder, regular expressions and str methods, not against the C++ code.  Also the line generator
of the BED tests and its condition."""
import re

import numpy as np

INTERSECT, DEPTH = 0, 1
DIALECT_NAME = {INTERSECT: "intersect", DEPTH: "depth"}

# Rust's char::is_whitespace (Unicode White_Space), what str::trim_end cuts
WHITE_SPACE = "".join(map(chr, [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) +
                          [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))
_NUMBER = re.compile(rb"\+?[0-9]+")
_FIELDS = {INTERSECT: re.compile(rb"[^ \t\x0c\r\n]+"), DEPTH: re.compile(rb"[^ \t]+")}
SKIP_KINDS = {INTERSECT: ("empty", "comment", "fewfields", "noseq"),
              DEPTH: ("comment", "fewfields", "fieldutf8", "coordinate", "nointerval", "noseq")}
ERROR_KINDS = ("utf8", "coordinate")


def utf8_valid(b: bytes) -> bool:
    try:
        b.decode("utf-8")  # strict: overlong forms, surrogates and > U+10FFFF are refused
        return True
    except UnicodeDecodeError:
        return False


def parse_u32(b: bytes):
    """lexical_core::parse::<u32> and str::parse::<u32>: [+]digits, the whole field, <= 2^32 - 1; None otherwise."""
    if not _NUMBER.fullmatch(b):
        return None
    digits = b.lstrip(b"+").lstrip(b"0") or b"0"
    if len(digits) > 10:  # (and no conversion of a megabyte of digits)
        return None
    v = int(digits)
    return v if v <= 0xFFFFFFFF else None


def outcome(line: bytes, dialect: int, names: dict):
    """("keep", seq, start, end) | ("skip", why) | ("error", kind).  line: INTERSECT without its newline, DEPTH with it."""
    if not line:
        return ("skip", "empty")
    if line[:1] == b"#":
        return ("skip", "comment")
    if dialect == INTERSECT and not utf8_valid(line):
        return ("error", "utf8")
    f = _FIELDS[dialect].findall(line)
    if len(f) < 3:
        return ("skip", "fewfields")
    if dialect == INTERSECT:
        if f[0] not in names:
            return ("skip", "noseq")
        s, e = parse_u32(f[1]), parse_u32(f[2])
        if s is None or e is None:
            return ("error", "coordinate")
        return ("keep", names[f[0]], s, e)
    if not all(utf8_valid(x) for x in f[:3]):
        return ("skip", "fieldutf8")
    s, e = parse_u32(f[1]), parse_u32(f[2].decode("utf-8").rstrip(WHITE_SPACE).encode("utf-8"))
    if s is None or e is None:
        return ("skip", "coordinate")
    if s >= e:
        return ("skip", "nointerval")
    if f[0] not in names:
        return ("skip", "noseq")
    return ("keep", names[f[0]], s, e)


def lines_of(text: bytes, dialect: int):
    """The lines as the readers cut them: at every newline; a non-empty rest after the last one is the last line."""
    parts = text.split(b"\n")
    rest = parts.pop()
    out = [p + b"\n" for p in parts] if dialect == DEPTH else parts
    if rest:
        out.append(rest)
    return out


def error_message(kind: str, line: bytes) -> str:
    if kind == "utf8":
        return "invalid utf-8 sequence in BED line"
    return 'lexical parse error: invalid BED coordinate in "%s"' % line.decode("utf-8")


def name_table(names) -> dict:
    return {(n if isinstance(n, bytes) else n.encode()): i for i, n in enumerate(names)}


def run(text: bytes, dialect: int, names):
    """(rows (n, 3) uint32, counts, error message or None, outcomes).  After the first error nothing more is read."""
    table = name_table(names)
    rows, outs = [], []
    counts = {"lines": 0, "skipped": 0, "no_seq": 0, "kept": 0}
    for line in lines_of(text, dialect):
        o = outcome(line, dialect, table)
        outs.append(o)
        if o[0] == "error":
            return np.array(rows, np.uint32).reshape(-1, 3), counts, error_message(o[1], line), outs
        counts["lines"] += 1
        if o[0] == "keep":
            counts["kept"] += 1
            rows.append(o[1:])
        else:
            counts["no_seq" if o[1] == "noseq" else "skipped"] += 1
    return np.array(rows, np.uint32).reshape(-1, 3), counts, None, outs


# ---- the generated lines ---------------------------------------------------------------------------------------------------
GEN_NAMES = [b"chr1", b"chr2", b"chr10", b"chrX", "chrü".encode(), b"scaffold_000123"]

_ODD_OK = [  # lines no dialect calls an error, by what they exercise
    b"", b"#comment\t1\t2", b"# ", b"chr1\t5", b"chr1", b"\t \t", b"chrZ\t1\t5", b"chr\t1\t5", b"chr100\t1\t5", b"chrZ\tx\t5",
    b"chrZ\t5\t-1", b"chr1\t5\t5", b"chr2\t9\t3", b"chr1\t1\x0c\t2", b"chr1\x0c1\x0c2", b"chr1\r1\r2", b"chr2\t1\t2\r",
    b"chr2\t1\t2\x0c", b" chr10\t+1\t0002", b"chrX 1 2 x y", b"chr1\t4294967294\t4294967295", b"chr1\x0b1\x0b2", b"chr1\r\t1\t2",
]
_ODD_DEPTH_ONLY = [  # errors of INTERSECT that DEPTH only skips or keeps
    b"chr\xff1\t1\t2", b"chr1\t1\xff\t2", b"chr1\t1\t2\xff", b"chr1\t1\t2\tn\xc0\xaf", b"chr1\t1\t2\t\xed\xa0\x80", b"chr1\t1\t2\xe2\x82",
    b"chr1\tx\t2", b"chr1\t1\t4294967296", b"chr1\t-1\t2", b"chr1\t1\t2\xc2\xa0", b"chr1\t1\t2\x0b", b"chr1\t1\t2\xe2\x80\xa8",
]


def generate(n: int, seed: int, dialect: int, errors: bool = False) -> list:
    """n lines (without newline).  At least half are plain rows of GEN_NAMES; the rest cycle through the odd ones.  DEPTH, where
    nothing is an error, also gets the lines INTERSECT calls errors; errors=True gives INTERSECT those too."""
    rng = np.random.Generator(np.random.PCG64(seed))
    odd = _ODD_OK + (_ODD_DEPTH_ONLY if dialect == DEPTH or errors else [])
    out = []
    for i in range(n):
        if rng.random() < 0.7:
            s = int(rng.integers(0, 1 << int(rng.integers(1, 32))))
            e = s + int(rng.integers(1, 100000))
            sep = b"\t" if rng.random() < 0.9 else b" "
            tail = (b"", b"", b"", b"\tname\t0\t+", b"\r")[int(rng.integers(0, 5))]
            out.append(GEN_NAMES[int(rng.integers(0, len(GEN_NAMES)))] + sep + b"%d" % s + sep + b"%d" % min(e, 0xFFFFFFFF) + tail)
        else:
            out.append(odd[int(rng.integers(0, len(odd)))])
    return out


def check_generated(lines, dialect: int, errors: bool = False) -> None:
    """The generator's condition, on the oracle alone."""
    table = name_table(GEN_NAMES)
    outs = [outcome(ln + b"\n" if dialect == DEPTH else ln, dialect, table) for ln in lines]
    if errors:
        for kind in ERROR_KINDS:
            assert any(o == ("error", kind) for o in outs), kind
        return
    assert not any(o[0] == "error" for o in outs)
    assert 2 * sum(o[0] == "keep" for o in outs) >= len(lines)
    for why in SKIP_KINDS[dialect]:
        assert sum(o == ("skip", why) for o in outs) >= 20, why
