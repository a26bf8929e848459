"""The quantity behind `gffx coverage --mean-depth`, twice and independently of the engine.  Coordinates are 0-based
half-open.  For a segment [a, b) on seqid c and the multiset of rows [s, e) of that seqid

    bases(a, b) = sum over the rows of max(0, min(e, b) - max(s, a)),       0 for a segment with a >= b

``brute`` is that sum, in numpy uint64 over (segments x rows of the seqid).  ``closed_form`` restates the device's way without
its code: with B(x) = sum_{s < x} (x - s) - sum_{e < x} (x - e), bases(a, b) = B(b) - B(a) -- np.searchsorted(side="left")
counts the keys < x, cumulative sums give the sums of the counted keys.  ``HAND`` are the shapes both test files walk."""
import numpy as np

U32_MAX = 2 ** 32 - 1


def _cols(rows):
    r = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    return r[:, 0], r[:, 1], r[:, 2]


def brute(rows, seg_seq, seg_start, seg_end, chunk=1 << 22):
    rq, rs, re_ = _cols(rows)
    q, a, b = (np.asarray(x, dtype=np.uint64) for x in (seg_seq, seg_start, seg_end))
    out = np.zeros(len(q), dtype=np.uint64)
    for c in np.unique(q):
        s, e = rs[rq == c], re_[rq == c]
        if not len(s):
            continue
        for i in np.nonzero(q == c)[0]:
            if a[i] >= b[i]:
                continue
            total = np.uint64(0)
            for at in range(0, len(s), chunk):  # (rows in pieces: one segment against 4 Mi rows stays a few arrays of 32 MB)
                lo, hi = np.maximum(s[at:at + chunk], a[i]), np.minimum(e[at:at + chunk], b[i])
                total += np.where(hi > lo, hi - lo, np.uint64(0)).sum(dtype=np.uint64)
            out[i] = total
    return out


def _below(keys_sorted, prefix, x):
    """sum over {k < x} of (x - k): count * x - sum of the counted keys (never negative: every counted key is < x)."""
    n = np.searchsorted(keys_sorted, x, side="left").astype(np.uint64)
    return n * x - prefix[n.astype(np.int64)]


def closed_form(rows, seg_seq, seg_start, seg_end):
    rq, rs, re_ = _cols(rows)
    q, a, b = (np.asarray(x, dtype=np.uint64) for x in (seg_seq, seg_start, seg_end))
    out = np.zeros(len(q), dtype=np.uint64)
    for c in np.unique(q):
        s, e = np.sort(rs[rq == c]), np.sort(re_[rq == c])  # (each on its own: starts and ends need not stay paired)
        ps = np.concatenate([[np.uint64(0)], np.cumsum(s, dtype=np.uint64)])
        pe = np.concatenate([[np.uint64(0)], np.cumsum(e, dtype=np.uint64)])
        m = (q == c) & (a < b)
        big_b = _below(s, ps, b[m]) - _below(e, pe, b[m])
        big_a = _below(s, ps, a[m]) - _below(e, pe, a[m])
        out[m] = big_b - big_a
    return out


def _rows(*triples):
    return np.array(triples, dtype=np.uint32).reshape(-1, 3)


def _segs(*triples):
    t = np.array(triples, dtype=np.uint32).reshape(-1, 3)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def _hand():
    h = {}
    # rows that only touch a segment (e == a or s == b) add nothing
    h["touching"] = (1, _rows((0, 10, 20), (0, 20, 30), (0, 0, 10)),
                     _segs((0, 20, 30), (0, 0, 10), (0, 10, 20), (0, 5, 15), (0, 19, 21), (0, 30, 40), (0, 9, 10), (0, 20, 21)))
    k = np.arange(300, dtype=np.uint32)
    # 300 equal starts / 300 equal ends: the searches must count exactly the keys < x among the ties
    h["equal_starts"] = (1, np.stack([0 * k, 100 + 0 * k, 101 + k], axis=1),
                         _segs((0, 100, 101), (0, 99, 100), (0, 100, 400), (0, 50, 500), (0, 101, 102), (0, 0, 100), (0, 399, 401)))
    h["equal_ends"] = (1, np.stack([0 * k, 700 + k, 1000 + 0 * k], axis=1),
                       _segs((0, 999, 1000), (0, 1000, 1001), (0, 700, 1000), (0, 0, 701), (0, 998, 1002), (0, 650, 2000)))
    h["extremes"] = (1, _rows((0, 0, U32_MAX), (0, 0, 1), (0, U32_MAX - 1, U32_MAX)),
                     _segs((0, 0, U32_MAX), (0, 0, 1), (0, U32_MAX - 1, U32_MAX), (0, U32_MAX, U32_MAX), (0, 1, U32_MAX - 1)))
    # three rows [0, 2^32 - 1) on the segment [0, 2^32 - 1): a total above 2^32
    h["three_full"] = (1, _rows((0, 0, U32_MAX), (0, 0, U32_MAX), (0, 0, U32_MAX)), _segs((0, 0, U32_MAX), (0, 5, 6)))
    # starts near 3 * 10^9: the prefix sums pass 2^32 at the second row
    h["big_starts"] = (1, _rows((0, 3_000_000_000, 3_000_000_100), (0, 3_000_000_050, 3_100_000_000), (0, 2_999_999_990, 3_000_000_060),
                                (0, 3_000_000_099, 3_000_000_100)),
                       _segs((0, 3_000_000_000, 3_000_000_100), (0, 2_999_999_000, 3_200_000_000), (0, 3_000_000_060, 3_000_000_099),
                             (0, 3_050_000_000, 3_050_000_001), (0, 0, 3_000_000_000)))
    h["seqid_without_rows"] = (4, _rows((0, 1, 9), (3, 5, 50), (3, 7, 8), (0, 2, 3)),
                               _segs((1, 0, 100), (2, 0, 100), (0, 0, 100), (3, 0, 100), (1, 5, 6)))
    h["empty_and_inverted_segments"] = (2, _rows((0, 10, 100), (1, 10, 100), (0, 40, 60)),
                                        _segs((0, 50, 50), (0, 60, 40), (1, 100, 10), (0, 40, 60), (1, 0, U32_MAX)))
    return h


HAND = _hand()
