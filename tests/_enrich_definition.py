"""The definition of `gffx enrich` restated in Python integers, its statistics, and a hand-written example.

A finished class map of T layers over n_seq seqids (tests/_annotate_definition.py), a length L[c] per seqid, regions (c, qs, qe)
numbered by their global row i, N permutations and a 64-bit seed.  All arithmetic mod 2^64:
    GOLD = 0x9E3779B97F4A7C15;  mix64 = the splitmix64 finalizer;  key(p) = mix64(seed + GOLD * p);
    r(p, i) = mix64(key(p) + GOLD * (i + 1))
Row 0 of the totals is the observed data.  In row p = 1 .. N a region with qs >= qe is empty (class T, no bases), one with
w = qe - qs > L[c] is unplaceable and stays (counted once in ``unplaced``), any other lies at [s', s' + w) with
s' = (r(p, i) * (L[c] - w + 1)) >> 64.  B[p][k] = the sum of bases_k, R[p][k] = the regions whose class is k.

``totals``        places with Python integers and answers every row with ``_annotate_definition.sparse``.
``totals(fast=True)``  the same placement; a row's answers come from ``piece_counts``: the overlap of every region with every
                  piece of its seqid as one numpy matrix, summed per class -- no search and no running sum, for the cases
                  where ``sparse`` (a Python loop over regions x pieces) would take minutes.  tests/test_enrich_cpu.py holds
                  the two against each other.
"""
import math

import numpy as np

import _annotate_definition as ad

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
MAX_PERMS = 1 << 20
MIX_VECTORS = [(1, 0xE220A8397B1DCDAF), (2, 0x6E789E6AA1B965F4), (3, 0x06C45D188009454F)]  # n -> mix64(GOLD * n)
EMPTY, UNPLACEABLE, PLACED = 0, 1, 2


def mix64(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def key(seed, p):
    return mix64(seed + GOLD * p)


def draw(seed, p, i):
    return mix64(key(seed, p) + GOLD * (i + 1))


def place(r, L, qs, qe):
    """-> (kind, start) of the region [qs, qe) under the draw r on a seqid of length L."""
    if qs >= qe:
        return EMPTY, qs
    w = qe - qs
    if w > L:
        return UNPLACEABLE, qs
    return PLACED, (r * (L - w + 1)) >> 64


def placed_regions(seq_len, regions, p, seed, first_row=0):
    """The regions of row p (row 0: where they stand), as an int64 array, and how many are unplaceable."""
    q = np.asarray(regions, np.int64).reshape(-1, 3)
    out, unplaced = q.copy(), 0
    for j, (c, qs, qe) in enumerate(q.tolist()):
        kind, s = place(draw(seed, p, first_row + j), int(seq_len[c]), qs, qe)
        unplaced += kind == UNPLACEABLE
        if p and kind == PLACED:
            out[j, 1], out[j, 2] = s, s + (qe - qs)
    return out, unplaced


def piece_counts(n_seq, T, per_seq, regions, block=2048):
    """counts [nq, T + 1] (Python-exact in int64: a count is below 2^32) and the class per region, from the overlap matrix."""
    q = np.asarray(regions, np.int64).reshape(-1, 3)
    counts = np.zeros((len(q), T + 1), np.int64)
    for c in range(n_seq):
        mine = np.flatnonzero((q[:, 0] == c) & (q[:, 1] < q[:, 2]))
        pts = per_seq.get(c, [])
        if not len(mine):
            continue
        if len(pts):
            x = np.array([p for p, _ in pts], np.int64)
            k = np.array([m for _, m in pts], np.int64)
            lo, hi, cls = x[:-1], x[1:], k[:-1]  # the piece [x_j, x_{j+1}) has class k_j; the last point opens "none"
            onehot = (cls[:, None] == np.arange(T)[None, :]).astype(np.int64)
            for at in range(0, len(mine), block):
                m = mine[at:at + block]
                over = np.minimum(hi[None, :], q[m, 2][:, None]) - np.maximum(lo[None, :], q[m, 1][:, None])
                counts[m, :T] = np.maximum(over, 0) @ onehot
        counts[mine, T] = q[mine, 2] - q[mine, 1] - counts[mine, :T].sum(1)
    if len(q) and np.any(q[:, 0] >= n_seq):
        raise ValueError("range")
    has = counts[:, :T] > 0
    best = np.where(has.any(1), has.argmax(1), T)
    return counts, best


def totals(n_seq, T, rows, seq_len, regions, n_perm, seed, first_row=0, fast=False):
    """-> (B, R) as (n_perm + 1, T + 1) uint64 and the number of unplaceable regions."""
    q = np.asarray(regions, np.int64).reshape(-1, 3)
    if len(q) and np.any(q[:, 0] >= n_seq):
        raise ValueError("range")
    per_seq = ad.sparse_map(n_seq, T, rows) if fast else None
    B, R, unplaced = np.zeros((n_perm + 1, T + 1), np.uint64), np.zeros((n_perm + 1, T + 1), np.uint64), 0
    for p in range(n_perm + 1):
        moved, u = placed_regions(seq_len, q, p, seed, first_row)
        if p == 0:
            unplaced = u
        if fast:
            counts, best = piece_counts(n_seq, T, per_seq, moved)
        else:
            counts, best = ad.sparse(n_seq, T, rows, moved)[4:6]
        B[p] = [sum(int(v) for v in counts[:, k]) for k in range(T + 1)]
        R[p] = np.bincount(np.asarray(best, np.int64), minlength=T + 1)
    return B, R, int(unplaced)


def add(a, b):
    """The totals of two runs over the same map, permutations and seed."""
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def same(a, b):
    return (a[0].dtype == b[0].dtype == np.uint64 and a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape
            and np.array_equal(a[1], b[1]) and int(a[2]) == int(b[2]))


# ---- the statistics of one output line ---------------------------------------------------------------------------------------
def stats(X):
    """X[0] observed, X[1 .. N] the permutations (integers) -> (observed, mean, sd, z, fold, n_ge, n_le, p_ge, p_le)."""
    X = [int(v) for v in X]
    N = len(X) - 1
    if len(set(X[1:])) == 1:  # one value in every permutation: mean is that value and sd is 0, exactly
        mean, sd = float(X[1]), (0.0 if N > 1 else math.nan)
    else:
        mean = math.fsum(float(v) for v in X[1:]) / N
        sd = math.sqrt(math.fsum((v - mean) ** 2 for v in X[1:]) / (N - 1))
    z = (X[0] - mean) / sd if N > 1 and sd != 0 else math.nan
    fold = X[0] / mean if mean != 0 else math.nan
    n_ge, n_le = sum(v >= X[0] for v in X[1:]), sum(v <= X[0] for v in X[1:])
    return X[0], mean, sd, z, fold, n_ge, n_le, (n_ge + 1) / (N + 1), (n_le + 1) / (N + 1)


HEADER = "#class\tquantity\tobserved\tmean\tsd\tz\tfold\tn_ge\tn_le\tp_ge\tp_le\n"
INT_COLUMNS, FLOAT_COLUMNS = (0, 1, 2, 7, 8), (3, 4, 5, 6, 9, 10)


def expected_lines(names, B, R):
    """The table's lines as lists of fields: text for class, quantity and the integers, floats (nan among them) for the rest."""
    out = []
    for k, name in enumerate(list(names) + ["none"]):
        for quantity, M in (("bases", B), ("regions", R)):
            s = stats(M[:, k])
            out.append([name, quantity, str(s[0]), s[1], s[2], s[3], s[4], str(s[5]), str(s[6]), s[7], s[8]])
    return out


def table_matches(text, names, B, R, rel=1e-5):
    """The command's table against the definition: header and integer columns byte for byte, floats to ``rel`` (what %.6g
    keeps), nan as text."""
    lines = text.decode().split("\n")
    want = expected_lines(names, B, R)
    if lines[0] + "\n" != HEADER or lines[-1] != "" or len(lines) != len(want) + 2:
        return False
    for got, w in zip(lines[1:-1], want):
        g = got.split("\t")
        if len(g) != 11 or any(g[c] != w[c] for c in INT_COLUMNS):
            return False
        for c in FLOAT_COLUMNS:
            if math.isnan(w[c]):
                if g[c] != "nan":
                    return False
            elif g[c] == "nan" or abs(float(g[c]) - w[c]) > rel * abs(w[c]):
                return False
    return True


def perms_text(B, R):
    """The --perms file: one line per row p: p, the T + 1 bases, the T + 1 region counts."""
    return "".join("%d\t%s\t%s\n" % (p, "\t".join(str(int(v)) for v in B[p]), "\t".join(str(int(v)) for v in R[p])) for p in range(len(B))).encode()


# ---- the example by hand: _annotate_definition's map (layers CDS, exon, gene; two seqids) with lengths that force every
# placement: a region is empty, wider than its seqid, or exactly as wide (span = 1, so s' = 0 whatever the draw) -------------
HAND_LEN = [400, 20]
HAND_REGIONS = np.array([
    [0, 100, 500],   # observed CDS 50, exon 200, gene 150; placed at [0, 400): none 100, gene 50, exon 50 + 150, CDS 50
    [0, 600, 1000],  # observed gene 100, none 300; placed at [0, 400) like the first
    [0, 300, 300],   # empty: class "none", no bases, in every row
    [0, 0, 1000],    # wider than seqid 0: stays.  CDS 50, exon 200, gene 50 + 100 + 100, none 500
    [1, 5, 25],      # observed exon 5, CDS 10, none 5; placed at [0, 20): exon 10, CDS 10
    [1, 0, 30],      # wider than seqid 1: stays.  CDS 10, exon 10, none 10
], np.uint32)
HAND_N_PERM = 2
HAND_B = [[120, 415, 500, 815], [170, 620, 350, 710], [170, 620, 350, 710]]
HAND_R = [[4, 0, 1, 1], [5, 0, 0, 1], [5, 0, 0, 1]]
HAND_UNPLACED = 2


def hand():
    return np.array(HAND_B, np.uint64), np.array(HAND_R, np.uint64), HAND_UNPLACED


# the command's table on the hand example (-g with HAND_LEN, -n 2, any seed), by hand: sd = 0, so z is nan everywhere
BY_HAND_TABLE = (HEADER +
                 "CDS\tbases\t120\t170\t0\tnan\t0.705882\t2\t0\t1\t0.333333\n"
                 "CDS\tregions\t4\t5\t0\tnan\t0.8\t2\t0\t1\t0.333333\n"
                 "exon\tbases\t415\t620\t0\tnan\t0.669355\t2\t0\t1\t0.333333\n"
                 "exon\tregions\t0\t0\t0\tnan\tnan\t2\t2\t1\t1\n"
                 "gene\tbases\t500\t350\t0\tnan\t1.42857\t0\t2\t0.333333\t1\n"
                 "gene\tregions\t1\t0\t0\tnan\tnan\t0\t2\t0.333333\t1\n"
                 "none\tbases\t815\t710\t0\tnan\t1.14789\t0\t2\t0.333333\t1\n"
                 "none\tregions\t1\t1\t0\tnan\t1\t2\t2\t1\t1\n").encode()
BY_HAND_PERMS = b"0\t120\t415\t500\t815\t4\t0\t1\t1\n1\t170\t620\t350\t710\t5\t0\t0\t1\n2\t170\t620\t350\t710\t5\t0\t0\t1\n"
# ... as a BED file for tests/_annotate_definition.GFF (a comment and a line on a seqid nobody knows take no row number)
BED = b"chrA\t100\t500\tpeak\nchrA\t600\t1000\n# a comment\nchrA\t300\t300\nchrUn\t5\t10\nchrA\t0\t1000\nchrB\t5\t25\nchrB\t0\t30\n"
GENOME = b"chrB\t20\t7\t60\t61\nchrA\t400\nchrUn\t1000\n"  # (a .fai's further columns; a name the index does not know)


# ---- cases ----------------------------------------------------------------------------------------------------------------
def random_case(seed, n_seq=3, T=4, n=60, size=2000, nq=50, width=None):
    """A map, lengths at or beyond the map's end and regions of every kind (empty, inverted, wider than the seqid)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, size - 1, n)
    e = np.minimum(s + 1 + rng.integers(0, width or size // 8, n), size)
    rows = np.stack([rng.integers(0, T, n), rng.integers(0, n_seq, n), s, e], 1).astype(np.uint32)
    seq_len = (size + rng.integers(0, size // 4, n_seq)).astype(np.uint32)
    a = rng.integers(0, size, nq)
    w = rng.integers(0, size // 3, nq)
    regions = np.stack([rng.integers(0, n_seq, nq), a, a + w], 1).astype(np.uint32)
    regions[::11, 2] = regions[::11, 1]                      # empty
    regions[5::13, 1], regions[5::13, 2] = 900, 100          # inverted
    regions[7::17, 1], regions[7::17, 2] = 0, 2 * size       # wider than any seqid
    return n_seq, T, rows, seq_len, regions


EDGE_L = 0xFFFFFFFF


def edge_case():
    """The length and width edges: L = 2^32 - 1 with w = 1 and w = L, w = L + 1 (L = 99), L = 0, empty regions, a seqid
    without points.  -> (n_seq, T, rows, seq_len, regions)"""
    rows = np.array([[0, 0, 0, 1 << 31], [1, 0, 1 << 30, EDGE_L], [0, 1, 10, 60], [1, 1, 50, 99], [1, 3, 0, 7]], np.uint32)
    seq_len = np.array([EDGE_L, 99, 12345, 0, EDGE_L], np.uint32)  # (seqid 2 and seqid 4 have no points)
    regions = np.array([
        [0, 5, 6], [0, 123, 124], [0, 0, EDGE_L], [0, EDGE_L - 1, EDGE_L],   # L = 2^32 - 1: w = 1 and w = L
        [1, 0, 99], [1, 0, 100], [1, 20, 21],                                   # w = L, w = L + 1, w = 1
        [2, 100, 300], [2, 0, 12345], [2, 0, 12346],                            # a seqid without points
        [3, 0, 1], [3, 5, 5], [3, 0, 7],                                        # L = 0: whatever is not empty stays
        [4, 1, EDGE_L], [4, 7, 7], [4, 9, 3], [0, 77, 77],                      # no points at full length; empty regions
    ], np.uint32)
    return 5, 2, rows, seq_len, regions


def big_totals_case():
    """Totals above 2^32: eight regions of width 2^31 on a seqid that one layer covers wholly."""
    rows = np.array([[0, 0, 0, EDGE_L]], np.uint32)
    regions = np.array([[0, 17 * j, 17 * j + (1 << 31)] for j in range(8)], np.uint32)
    return 1, 1, rows, np.array([EDGE_L], np.uint32), regions
