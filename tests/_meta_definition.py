"""The quantity behind `gffx meta`, twice and independently of the engine, in Python integers.

A feature is [s, e) with L = e - s on the plus or the minus strand.  An offset t in the feature's orientation lies in the genome
at g(t) = s + t (plus) or e - t (minus).  A layout cuts B columns by B + 1 offsets:

    point    B = (UP + DOWN) / BIN;  t_k = a0 - UP + k BIN;  a0 = 0 (tss), L (tes), L // 2 (center)
    scaled   B = UP / BIN + M + DOWN / BIN;  t_k = -UP + k BIN up to k = UP / BIN, then (j L) // M for j = 0 .. M, then L + j BIN

Column j is the offsets [t_j, t_{j+1}): [s + t_j, s + t_{j+1}) on plus, [e - t_{j+1}, e - t_j) on minus, each boundary clamped to
[0, len] (len: the seqid's length, 2^32 - 1 without one).  bases[i][j] = the pileup's bases of the clamped column over the rows of
the feature's seqid, len[i][j] = its width; per column the sums over the features and the number of features with len > 0.

``dense`` walks an array of per-base depth with explicit loops over features, columns and bases (small coordinates);
``sparse`` asks _pileup_definition.closed_form for every clamped column and reaches 2^32 - 1.  ``HAND`` is worked by hand."""
import numpy as np

import _pileup_definition as pd

U32_MAX = 2 ** 32 - 1
POINT, SCALED = 0, 1
TSS, TES, CENTER = 0, 1, 2


def point(up, down, bin, anchor=TSS):
    return (POINT, anchor, up, down, bin, 0)


def scaled(up, down, bin, m):
    return (SCALED, 0, up, down, bin, m)


def columns(lay):
    """B, 0 for a layout that is none."""
    mode, anchor, up, down, bin, m = lay
    if bin == 0 or up % bin or down % bin:
        return 0
    if mode == POINT:
        return (up + down) // bin if anchor in (TSS, TES, CENTER) else 0
    if mode == SCALED:
        return up // bin + m + down // bin if m else 0
    return 0


def offsets(lay, L):
    """t_0 .. t_B for a feature of length L."""
    mode, anchor, up, down, bin, m = lay
    if mode == POINT:
        a0 = {TSS: 0, TES: L, CENTER: L // 2}[anchor]
        return [a0 - up + k * bin for k in range((up + down) // bin + 1)]
    t = [-up + k * bin for k in range(up // bin)]
    t += [(j * L) // m for j in range(m + 1)]
    t += [L + j * bin for j in range(1, down // bin + 1)]
    return t


def bounds(lay, s, e, minus, length=U32_MAX):
    """The clamped columns [(a, b)] of one feature, in column order."""
    clamp = lambda g: min(max(g, 0), length)  # noqa: E731
    t = offsets(lay, e - s)
    if minus:
        return [(clamp(e - t[j + 1]), clamp(e - t[j])) for j in range(len(t) - 1)]
    return [(clamp(s + t[j]), clamp(s + t[j + 1])) for j in range(len(t) - 1)]


def _feats(feats):
    return [tuple(int(x) for x in f) for f in np.asarray(feats, dtype=np.int64).reshape(-1, 4).tolist()]


def _len_of(seq_len, c):
    return U32_MAX if seq_len is None else int(seq_len[c])


def lens(feats, lay, seq_len=None):
    """len[i][j] as a G x B array of uint64."""
    B = columns(lay)
    out = np.zeros((len(_feats(feats)), B), dtype=np.uint64)
    for i, (c, s, e, minus) in enumerate(_feats(feats)):
        out[i] = [b - a for a, b in bounds(lay, s, e, minus, _len_of(seq_len, c))]
    return out


def dense(n_seq, rows, feats, lay, seq_len=None):
    """bases[i][j] from an array of per-base depth: loops over features, columns and bases.  Small coordinates only."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    feats = _feats(feats)
    top = max([int(rows[:, 2].max())] if len(rows) else [0]) + 1
    depth = [[0] * top for _ in range(n_seq)]
    for c, s, e in rows.tolist():
        for x in range(s, e):
            depth[c][x] += 1
    out = np.zeros((len(feats), columns(lay)), dtype=np.uint64)
    for i, (c, s, e, minus) in enumerate(feats):
        for j, (a, b) in enumerate(bounds(lay, s, e, minus, _len_of(seq_len, c))):
            total = 0
            for x in range(a, min(b, top)):  # (beyond the last row's end the depth is 0)
                total += depth[c][x]
            out[i, j] = total
    return out


def sparse(n_seq, rows, feats, lay, seq_len=None):
    """bases[i][j] from the closed form of the pileup, one segment per clamped column."""
    feats = _feats(feats)
    B = columns(lay)
    q, a, b = [], [], []
    for c, s, e, minus in feats:
        for lo, hi in bounds(lay, s, e, minus, _len_of(seq_len, c)):
            q.append(c), a.append(lo), b.append(hi)
    if not q:
        return np.zeros((len(feats), B), dtype=np.uint64)
    return pd.closed_form(np.asarray(rows, dtype=np.uint32).reshape(-1, 3), q, a, b).reshape(len(feats), B)


def segments(feats, lay, seq_len=None):
    """The G x B explicit clamped columns as (seq, start, end) uint32 arrays: what a Pileup takes as segments."""
    q, a, b = [], [], []
    for c, s, e, minus in _feats(feats):
        for lo, hi in bounds(lay, s, e, minus, _len_of(seq_len, c)):
            q.append(c), a.append(lo), b.append(hi)
    return tuple(np.array(x, dtype=np.uint32) for x in (q, a, b))


def totals(matrix, width):
    """(col_bases, col_len, col_features) of a bases matrix and its lens."""
    return (matrix.sum(0, dtype=np.uint64), width.sum(0, dtype=np.uint64), (width > 0).sum(0).astype(np.uint64))


def mirror(rows, feats, C):
    """Every coordinate x -> C - x, every strand flipped."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    f = np.asarray(feats, dtype=np.int64).reshape(-1, 4)
    return (np.stack([r[:, 0], C - r[:, 2], C - r[:, 1]], axis=1).astype(np.uint32),
            np.stack([f[:, 0], C - f[:, 2], C - f[:, 1], 1 - f[:, 3]], axis=1).astype(np.uint32))


def labels(lay):
    """(part, from, to) per column, as the summary prints them."""
    mode, anchor, up, down, bin, m = lay
    if mode == POINT:
        return [("point", -up + k * bin, -up + (k + 1) * bin) for k in range(columns(lay))]
    return ([("up", -up + k * bin, -up + (k + 1) * bin) for k in range(up // bin)] + [("body", j, j + 1) for j in range(m)] +
            [("down", k * bin, (k + 1) * bin) for k in range(down // bin)])


def summary_text(lay, col_bases, col_len, col_features):
    out = [b"#column\tpart\tfrom\tto\tfeatures\tbases\tlength\tmean_depth\n"]
    for j, (part, lo, hi) in enumerate(labels(lay)):
        bases, length = int(col_bases[j]), int(col_len[j])
        mean = "%.6f" % (bases / length) if length else "0.000000"
        out.append(("%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (j, part, lo, hi, int(col_features[j]), bases, length, mean)).encode())
    return b"".join(out)


def matrix_text(names, feats, ids, matrix):
    B = matrix.shape[1]
    out = [("#chr\tstart\tend\tid\tstrand" + "".join("\tc%d" % j for j in range(B)) + "\n").encode()]
    for (c, s, e, minus), name, row in zip(_feats(feats), ids, matrix.tolist()):
        out.append(("%s\t%d\t%d\t%s\t%s" % (names[c], s, e, name, "-" if minus else "+") + "".join("\t%d" % v for v in row) + "\n").encode())
    return b"".join(out)


def random_case(seed, n_seq=2, n_rows=60, n_feat=8, span=400, lo=100):
    """Small coordinates; with lo == 0 windows cross 0 and are clamped there."""
    rng = np.random.default_rng(seed)
    rows = np.empty((n_rows, 3), np.uint32)
    rows[:, 0] = rng.integers(0, n_seq, n_rows)
    rows[:, 1] = rng.integers(0, lo + span, n_rows)
    rows[:, 2] = rows[:, 1] + rng.choice([1, 2, 7, 40], n_rows)
    feats = np.empty((n_feat, 4), np.uint32)
    feats[:, 0] = rng.integers(0, n_seq, n_feat)
    feats[:, 1] = rng.integers(lo, lo + span, n_feat)
    feats[:, 2] = feats[:, 1] + rng.choice([1, 2, 3, 5, 17, 60], n_feat)
    feats[:, 3] = rng.integers(0, 2, n_feat)
    if lo == 0:  # two features whose windows do cross 0
        feats[0, 1:3] = (1, 4)
        feats[1, 1:3] = (0, 9)
    return n_seq, rows, feats


# ---- by hand ------------------------------------------------------------------------------------------------------------
# One seqid.  P = [10, 16) on plus (L = 6), Q = [20, 27) on minus (L = 7).  Six rows and the depth they give per base:
#   rows  [8,12) [10,11) [14,22) [25,30) [26,27) [0,3)
#   depth 0-2: 1 | 3-7: 0 | 8,9: 1 | 10: 2 | 11: 1 | 12,13: 0 | 14-21: 1 | 22-24: 0 | 25: 1 | 26: 2 | 27-29: 1 | 30-: 0
# Point mode, tss, UP = DOWN = 4, BIN = 2: t = -4 -2 0 2 4.
#   P  g = 6 8 10 12 14             columns [6,8) [8,10) [10,12) [12,14)          bases 0, 1+1, 2+1, 0
#   Q  g = 27 - t = 31 29 27 25 23  columns [29,31) [27,29) [25,27) [23,25)       bases 1+0, 1+1, 1+2, 0
# Scaled, M = 3, UP = DOWN = 4, BIN = 2 (B = 7):
#   P  t = -4 -2 | 0 2 4 6 | 8 10        g = 6 8 10 12 14 16 18 20     bases 0 2 3 | 0 2 2 | 2
#   Q  body t = 0, 7 // 3 = 2, 14 // 3 = 4, 7:  t = -4 -2 | 0 2 4 7 | 9 11   g = 31 29 27 25 23 20 18 16
#      columns [29,31) [27,29) | [25,27) [23,25) [20,23) | [18,20) [16,18)   bases 1 2 | 3 0 2 | 2 2; the last body column is 3 wide
# With the seqid 30 long, Q's first column is [29,30): the same base, 1 wide.
HAND_N_SEQ = 1
HAND_ROWS = np.array([(0, 8, 12), (0, 10, 11), (0, 14, 22), (0, 25, 30), (0, 26, 27), (0, 0, 3)], np.uint32)
HAND_FEATS = np.array([(0, 10, 16, 0), (0, 20, 27, 1)], np.uint32)
HAND_POINT = point(4, 4, 2)
HAND_SCALED = scaled(4, 4, 2, 3)
HAND = {
    "point": (HAND_POINT, None, [[0, 2, 3, 0], [1, 2, 3, 0]], [[2, 2, 2, 2], [2, 2, 2, 2]], [1, 4, 6, 0], [4, 4, 4, 4], [2, 2, 2, 2]),
    "point_len_30": (HAND_POINT, [30], [[0, 2, 3, 0], [1, 2, 3, 0]], [[2, 2, 2, 2], [1, 2, 2, 2]], [1, 4, 6, 0], [3, 4, 4, 4], [2, 2, 2, 2]),
    "scaled": (HAND_SCALED, None, [[0, 2, 3, 0, 2, 2, 2], [1, 2, 3, 0, 2, 2, 2]], [[2] * 7, [2, 2, 2, 2, 3, 2, 2]], [1, 4, 6, 0, 4, 4, 4],
               [4, 4, 4, 4, 5, 4, 4], [2] * 7),
}
HAND_POINT_SUMMARY = (b"#column\tpart\tfrom\tto\tfeatures\tbases\tlength\tmean_depth\n"
                      b"0\tpoint\t-4\t-2\t2\t1\t4\t0.250000\n"
                      b"1\tpoint\t-2\t0\t2\t4\t4\t1.000000\n"
                      b"2\tpoint\t0\t2\t2\t6\t4\t1.500000\n"
                      b"3\tpoint\t2\t4\t2\t0\t4\t0.000000\n")
HAND_SCALED_SUMMARY = (b"#column\tpart\tfrom\tto\tfeatures\tbases\tlength\tmean_depth\n"
                       b"0\tup\t-4\t-2\t2\t1\t4\t0.250000\n"
                       b"1\tup\t-2\t0\t2\t4\t4\t1.000000\n"
                       b"2\tbody\t0\t1\t2\t6\t4\t1.500000\n"
                       b"3\tbody\t1\t2\t2\t0\t4\t0.000000\n"
                       b"4\tbody\t2\t3\t2\t4\t5\t0.800000\n"
                       b"5\tdown\t0\t2\t2\t4\t4\t1.000000\n"
                       b"6\tdown\t2\t4\t2\t4\t4\t1.000000\n")
