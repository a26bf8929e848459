"""Shared cases of the `gffx search` tests: a seeded generator of patterns inside the regex subset, the values they are
matched against, and lines for the value filter."""
import random

SCALARS = ["a", "b", "c", "A", "0", "1", "-", "_", ".", " ", "é", "ß", "→", "中", "😀"]
LITERALS = ["a", "b", "c", "A", "0", "1", "_", " ", "é", "→", "😀", r"\.", r"\+", r"\*", r"\?", r"\(", r"\)", r"\|", r"\[", r"\]",
            r"\{", r"\}", r"\^", r"\$", r"\-", r"\\", "]", "}"]
CLASSES = ["[abc]", "[^abc]", "[a-c]", "[^a-c0-1]", "[]a]", "[^]a]", "[a-]", "[-a]", "[a^]", "[A-Za-z_]", "[0-9]", r"[\]\-\\]", "[ -~]", "[^ -~]",
           "[.]", r"[a\-c]"]
GROUP_QUANTS = ["?", "{2}", "{0,1}", "{1,2}", "??"]
QUANTS = ["*", "+", "?", "{0}", "{1}", "{2}", "{0,1}", "{1,3}", "{2,}", "{0,}", "*?", "+?", "??", "{1,2}?", "{3}"]


def gen_pattern(rng: random.Random, depth: int = 0) -> str:
    def atom():
        k = rng.random()
        if k < 0.45:
            return rng.choice(LITERALS)
        if k < 0.6:
            return "."
        if k < 0.8:
            return rng.choice(CLASSES)
        if depth < 2:
            return ("(?:" if rng.random() < 0.4 else "(") + gen_pattern(rng, depth + 1) + ")"
        return rng.choice(LITERALS)

    def piece():
        a = atom()
        if rng.random() < 0.35:
            # an unbounded or lazy quantifier only on a one-scalar atom: re.search, the oracle, backtracks -- a starred group
            # around starred atoms costs it exponential time on a value of 300 scalars (the DFA does not care)
            a += rng.choice(GROUP_QUANTS if a[0] == "(" else QUANTS)
        return a

    def branch():
        n = rng.choice([0, 1, 1, 2, 2, 3, 4]) if depth else rng.choice([1, 1, 2, 3, 4, 5])
        s = "".join(piece() for _ in range(n))
        if rng.random() < 0.12:
            s = "^" + s
        if rng.random() < 0.12:
            s = s + "$"
        return s

    return "|".join(branch() for _ in range(rng.choice([1, 1, 1, 2, 3])))


def gen_value(rng: random.Random, length: int) -> str:
    """`length` scalars: ASCII and 2-, 3- and 4-byte ones, never "\\n" """
    return "".join(rng.choice(SCALARS) for _ in range(length))


def corpus(seed: int = 20, n_patterns: int = 300, per_length: int = 8):
    """(patterns, values): the values have 0, 1, 15, 16, 17 and 300 scalars"""
    rng = random.Random(seed)
    patterns = [gen_pattern(rng) for _ in range(n_patterns)] + ["", "^", "$", "^$", "$^", "a|", "|", "(|a)b", "^a*$", "(a|b)*c$", "é+", ".{16}", "^.{17}$",
                                                                "[^a]{255}", "x{255}", "(ab?){2,3}c", "a{2}", "(^a|b$)", "😀.?→"]
    values = []
    for length in (0, 1, 15, 16, 17, 300):
        for _ in range(1 if length == 0 else per_length):
            values.append(gen_value(rng, length))
    values += ["a", "ab", "abc", "aab", "b", "éé", "😀→", "😀a→", "x" * 255, "x" * 254, "abab", "abbc", "ababc", "a" * 300]
    return patterns, values


NINE = b"c\ts\texon\t1\t2\t.\t+\t.\t"
# (line, kept for the key gene_name when {"TP53"} is the set of the line's root and no -T is given)
VALUE_LINES = [
    (NINE + b"ID=e1;gene_name=TP53\n", 1),
    (NINE + b"gene_name=TP53;ID=e1\n", 1),
    (NINE + b"ID=e1;gene_name=TP53\r\n", 1),                 # CRLF
    (NINE + b"ID=e1;gene_name=TP53", 1),                      # the key at the very end, no line ending
    (NINE + b"ID=e1;gene_name=", 0),                          # an empty value at the very end
    (NINE + b"gene_name=;ID=e1\n", 0),                        # an empty value
    (NINE + b"xgene_name=TP53;gene_name=BRCA1\n", 1),         # the first `gene_name=` is inside xgene_name= (a byte search)
    (NINE + b"xgene_name=BRCA1;gene_name=TP53\n", 0),
    (NINE + b"ID=e1;gene_name=TP5\n", 0),                     # a prefix of a value
    (NINE + b"ID=e1;gene_name=TP533\n", 0),
    (NINE + b"ID=e1;gene_name=BRCA1\n", 0),                   # a value of the table, another class
    (NINE + b"ID=e1;gene_name=nowhere\n", 0),                 # no value of the table
    (b"c\ts\texon\t1\t2\t.\t+\tgene_name=TP53\n", 0),         # fewer than 8 TABs
    (b"#" + NINE + b"gene_name=TP53\n", 0),
    (b"c\ts\tgene\t1\t2\t.\t+\t.\tgene_name=TP53\n", 1),
    (b"\n", 0),
    (NINE + b"gene_name=TP53;gene_name=BRCA1\n", 1),
]
