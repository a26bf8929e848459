"""The quantity behind `gffx coverage --thresholds / --bedgraph`, twice and independently of the engine.
Coordinates are 0-based half-open.  For seqid c and the multiset of rows [s, e), s < e, depth_c(x) = #{rows with s <= x < e}.
The canonical profile of a seqid is the list of points (pos_i, d_i): pos strictly ascending, d_i the depth on
[pos_i, pos_{i+1}), d_i != d_{i-1} (d_{-1} = 0), the last depth 0; a seqid without rows has no points.

``brute`` counts the rows over a numpy array of bases (coordinates below a few thousand) and reads the points off where
neighbouring bases differ.  ``sweep`` is a sparse sweep: a Python dict of deltas per position, walked in ascending order -- no
array over the bases, so coordinates up to 2^32 - 1 work.  Both return (p_off u64 [n_seq + 1], pos u32, depth u32).
``spans_at_least`` and ``covered_at_least`` derive the spans "depth >= T" and a segment's bases at depth >= T from the points;
``weighted_bases`` the sum of depth x overlap (the pileup's figure).  ``HAND`` are the shapes the test files walk."""
import numpy as np

U32_MAX = 2 ** 32 - 1


def _rows(rows):
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def _pack(n_seq, per_seq):
    p_off = np.zeros(n_seq + 1, np.uint64)
    pos, dep = [], []
    for c in range(n_seq):
        for x, d in per_seq.get(c, []):
            pos.append(x)
            dep.append(d)
        p_off[c + 1] = len(pos)
    return p_off, np.array(pos, np.uint32), np.array(dep, np.uint32)


def brute(rows, n_seq, size=None):
    """Definition (a): an array over the bases [0, size]."""
    r = _rows(rows)
    size = (int(r[:, 2].max()) if len(r) else 0) + 2 if size is None else size
    assert size < 1 << 22, "brute force is for small coordinates"
    per_seq = {}
    for c in range(n_seq):
        depth = np.zeros(size, np.int64)
        for _, s, e in r[r[:, 0] == c]:
            depth[s:e] += 1
        change = np.nonzero(np.diff(np.concatenate([[0], depth])))[0]  # x with depth[x] != depth[x - 1]
        per_seq[c] = [(int(x), int(depth[x])) for x in change]
    return _pack(n_seq, per_seq)


def sweep(rows, n_seq):
    """Definition (b): deltas per position in a dict, walked in ascending order."""
    r = _rows(rows)
    deltas = {}
    for c, s, e in r.tolist():
        assert 0 <= c < n_seq and 0 <= s < e <= U32_MAX
        d = deltas.setdefault(c, {})
        d[s] = d.get(s, 0) + 1
        d[e] = d.get(e, 0) - 1
    per_seq = {}
    for c, d in deltas.items():
        depth, out = 0, []
        for x in sorted(d):
            if d[x] == 0:
                continue  # an event, but the depth is the same on both sides: no point
            depth += d[x]
            out.append((x, depth))
        assert depth == 0
        per_seq[c] = out
    return _pack(n_seq, per_seq)


def sweep_np(rows, n_seq):
    """Definition (b) again in numpy, for row counts a Python loop is too slow for: the deltas summed per distinct
    (seqid, position), positions whose deltas cancel dropped, one cumulative sum (a seqid's deltas add up to zero)."""
    r = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    assert not len(r) or (int(r[:, 0].max()) < n_seq and bool((r[:, 1] < r[:, 2]).all()))
    keys = np.concatenate([(r[:, 0] << np.uint64(32)) | r[:, 1], (r[:, 0] << np.uint64(32)) | r[:, 2]])
    uniq, inv = np.unique(keys, return_inverse=True)
    delta = np.bincount(inv, weights=np.concatenate([np.ones(len(r)), -np.ones(len(r))]), minlength=len(uniq)).astype(np.int64)
    keep = delta != 0
    uniq, depth = uniq[keep], np.cumsum(delta[keep])
    assert not len(depth) or (depth.min() >= 0 and depth[-1] == 0)
    p_off = np.searchsorted(uniq >> np.uint64(32), np.arange(n_seq + 1, dtype=np.uint64), side="left").astype(np.uint64)
    return p_off, (uniq & np.uint64(U32_MAX)).astype(np.uint32), depth.astype(np.uint32)


def runs(points):
    """[(seqid, start, end, depth)] for every stretch between two points of a seqid, depth 0 included."""
    p_off, pos, dep = points
    out = []
    for c in range(len(p_off) - 1):
        for i in range(int(p_off[c]), int(p_off[c + 1]) - 1):
            out.append((c, int(pos[i]), int(pos[i + 1]), int(dep[i])))
    return out


def spans_at_least(points, T):
    """(u_off u64, us u32, ue u32, pb u64): the maximal stretches with depth >= T, neighbours merged, in the union's layout."""
    n_seq = len(points[0]) - 1
    u_off, us, ue, pb = np.zeros(n_seq + 1, np.uint64), [], [], []
    by_seq = {}
    for c, a, b, d in runs(points):
        if d >= T:
            by_seq.setdefault(c, []).append((a, b))
    for c in range(n_seq):
        first = len(us)
        for a, b in by_seq.get(c, []):
            if len(us) > first and ue[-1] == a:
                ue[-1] = b
            else:
                us.append(a)
                ue.append(b)
        run = 0  # pb[k] = the bases of the seqid's spans before span k
        for k in range(first, len(us)):
            pb.append(run)
            run += ue[k] - us[k]
        u_off[c + 1] = len(us)
    return u_off, np.array(us, np.uint32), np.array(ue, np.uint32), np.array(pb, np.uint64)


def covered_at_least(points, T, seg_seq, seg_start, seg_end):
    """Per segment the bases at depth >= T (0 for a segment with start >= end or a seqid without points)."""
    rs = runs(points)
    out = np.zeros(len(seg_seq), np.uint64)
    for i, (q, a, b) in enumerate(zip(map(int, seg_seq), map(int, seg_start), map(int, seg_end))):
        out[i] = sum(max(0, min(e, b) - max(s, a)) for c, s, e, d in rs if c == q and d >= T)
    return out


def weighted_bases(points, seg_seq, seg_start, seg_end):
    """Per segment the sum of depth x overlap over the runs: the pileup's bases(a, b)."""
    rs = runs(points)
    return [sum(d * max(0, min(e, b) - max(s, a)) for c, s, e, d in rs if c == q)
            for q, a, b in zip(map(int, seg_seq), map(int, seg_start), map(int, seg_end))]


def depth_at(points, c, x):
    p_off, pos, dep = points
    lo, hi = int(p_off[c]), int(p_off[c + 1])
    k = int(np.searchsorted(pos[lo:hi], x, side="right"))
    return 0 if k == 0 else int(dep[lo + k - 1])


def max_depth(points):
    return int(points[2].max()) if len(points[2]) else 0


def _r(*triples):
    return np.array(triples, dtype=np.uint32).reshape(-1, 3)


def _hand():
    h = {}
    h["one_row"] = (1, _r((0, 5, 9)))
    h["touching"] = (1, _r((0, 10, 20), (0, 20, 30)))  # no point at the joint
    h["overlapping"] = (1, _r((0, 10, 20), (0, 15, 30)))
    h["nested"] = (1, _r((0, 10, 100), (0, 40, 60), (0, 45, 50)))
    k = np.arange(300, dtype=np.uint32)
    h["equal_starts"] = (1, np.stack([0 * k, 100 + 0 * k, 101 + k], axis=1))
    h["equal_ends"] = (1, np.stack([0 * k, 700 + k, 1000 + 0 * k], axis=1))
    h["same_row_300_times"] = (1, np.stack([0 * k, 100 + 0 * k, 200 + 0 * k], axis=1))  # one point up, one down
    h["full_range"] = (1, _r((0, 0, U32_MAX)))
    h["extremes"] = (1, _r((0, 0, 1), (0, U32_MAX - 1, U32_MAX), (0, 0, U32_MAX)))
    h["seqid_without_rows"] = (3, _r((0, 1, 9), (2, 5, 50), (2, 7, 8), (0, 2, 3)))
    z = np.zeros(70000, np.uint32)
    h["depth_70000"] = (1, np.stack([z, z + 1000, z + 1010], axis=1))  # above 2^16
    h["cancelling"] = (1, _r((0, 0, 10), (0, 10, 20), (0, 5, 10), (0, 10, 15)))  # 10 is an event but no point
    return h


HAND = _hand()

# the answers worked by hand: name -> [(pos, depth)] per seqid
BY_HAND = {
    "one_row": [[(5, 1), (9, 0)]],
    "touching": [[(10, 1), (30, 0)]],
    "overlapping": [[(10, 1), (15, 2), (20, 1), (30, 0)]],
    "nested": [[(10, 1), (40, 2), (45, 3), (50, 2), (60, 1), (100, 0)]],
    "same_row_300_times": [[(100, 300), (200, 0)]],
    "full_range": [[(0, 1), (U32_MAX, 0)]],
    "extremes": [[(0, 2), (1, 1), (U32_MAX - 1, 2), (U32_MAX, 0)]],
    "seqid_without_rows": [[(1, 1), (2, 2), (3, 1), (9, 0)], [], [(5, 1), (7, 2), (8, 1), (50, 0)]],
    "depth_70000": [[(1000, 70000), (1010, 0)]],
    "cancelling": [[(0, 1), (5, 2), (15, 1), (20, 0)]],
}


def hand_points(name):
    per = BY_HAND[name]
    return _pack(len(per), dict(enumerate(per)))


def same(p, q):
    return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(p, q))
