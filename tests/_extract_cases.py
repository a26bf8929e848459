"""TEST INFRASTRUCTURE ONLY -- the inputs that tests/test_extract_cpu.py (the host build of device/ids_core.hpp) and
tests/test_extract_gpu.py (the kernels of device/ids.hip) both run: names at the lengths where a compare changes its path,
and one line of every class the line filter tells apart."""

LENGTHS = (1, 15, 16, 17, 255, 70000)


def edge_names():
    """names of the lengths at which an 8- or 16-byte compare changes its path, pairs that differ only in the last byte,
    and names that are prefixes of others"""
    names = []
    for n in LENGTHS:
        base = bytes(65 + (i * 7 + n) % 26 for i in range(n))
        names += [base, base[:-1] + b"#"]
    names += [b"gene1", b"gene10", b"gene100", b"gene", b"ab", b"abc"]
    return names


def edge_queries(names):
    return names + [n[:-1] for n in names if len(n) > 1] + [n + b"x" for n in names[:6]] + [b"nope", b"GENE1", b"a"] + names[::-1]


NINE = b"c\ts\texon\t1\t2\t.\t+\t.\t"
FILTER_NAMES = [b"g", b"b", b"a", b"x", b"other", b"dup", b"dup"]
FILTER_PRT = [0, 0, 0, 0, 4, 0, 4]      # `other` is a root of its own; the last `dup` belongs to it
FILTER_REQUESTED = [b"b", b"x", b"other", b"dup", b"not_there"]
FILTER_LINES = [                        # (line, kept without -T)
    (b"c\ts\texon\t1\t2\t.\t+\tID=b\n", 0),          # seven TABs
    (NINE + b"Name=b;Parent=g\n", 0),                 # no `ID=`
    (NINE + b"geneID=a;ID=b\n", 0),                   # the first `ID=` gives a, which was not requested
    (NINE + b"geneID=x;ID=q\n", 1),                   # ... and here x, which was
    (NINE + b"Parent=g;ID=b\n", 1),                   # the ID ends the line without ';'
    (NINE + b"ID=x;Parent=g\r\n", 1),                 # CRLF
    (NINE + b"ID=x\r\n", 1),                          # ... where the '\r' would otherwise be part of the value
    (b"#" + NINE + b"ID=b\n", 0),                     # a '#' line
    (b"##gff-version 3\n", 0),
    (b"\n", 0),
    (NINE + b"Note=1\tID=b;x=\t\n", 1),               # a TAB inside the attribute field
    (NINE + b"ID=other\n", 0),                        # requested, but its root is not this block's
    (NINE + b"ID=dup\n", 0),                          # the LAST dup line belongs to the other root
    (NINE + b"ID=bb\n", 0), (NINE + b"ID=\n", 0), (NINE + b"ID=g\n", 0),  # in the table or not, never requested
    (NINE.replace(b"exon", b"gene") + b"ID=b\n", 1),
    (NINE.replace(b"exon", b" exon") + b"ID=b\n", 1),
    (b"c\ts\texon\n", 0),                             # two TABs
    (NINE + b"ID=x", 1),                              # the last line has no newline
]
TYPE_CASES = [None, " exon , CDS,,\t", ",", "gene", "exon,gene"]


def refused_chunks(fn, who, handle):
    """the four chunks the front half of a filter_lines call refuses, through fn (gffx_hip_ids_filter_lines or
    gffx_hip_attrs_filter_lines of _ffi.lib()) on a live handle: [(return code, last error, the message it has to be)]"""
    import numpy as np
    from gffx_amd import _ffi
    text = np.frombuffer(b"abcdef\n", np.uint8).copy()
    cases = [([0, 4, 2], 0, None, "line_off is not ascending at 1"),
             ([0, len(text) + 1], 0, None, "the last line ends at 8, the text has 7 bytes"),
             ([0, len(text)], 65537, [0] * 65538, "65537 type names (at most 65536)"),
             ([0, len(text)], 2, [0, 3, 1], "type_off is not ascending at 1")]
    out = []
    for line_off, n_types, type_off, message in cases:
        lo = np.array(line_off, np.uint64)
        n = len(lo) - 1
        root, keep = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        to = None if type_off is None else np.array(type_off, np.uint32)
        rc = fn(handle, text.ctypes.data_as(_ffi.u8p), len(text), n, lo.ctypes.data_as(_ffi.u64p), root.ctypes.data_as(_ffi.u32p), 0, n_types,
                text.ctypes.data_as(_ffi.u8p), None if to is None else to.ctypes.data_as(_ffi.u32p), keep.ctypes.data_as(_ffi.u8p))
        out.append((rc, _ffi.lib().gffx_hip_last_error().decode(), "%s: %s" % (who, message)))
    return out


REUSE_SIZES = (65, 1, 0, 65)  # lines per call on one handle: past the wave edge at 64, one, none, and 65 again
