"""The definition of `gffx closest`, restated by brute force in numpy, and the hand cases of the closest tests.

Coordinates are 0-based and half-open.  The roots of seqid c are taken as [fs, fe) in INDEX POSITION order: start ascending,
stable (roots with one start keep the order the builder gave them).  fe >= fs.  A region is (c, qs, qe) with qs < qe.  Every
root of the seqid is in exactly one class with respect to the region:

    OVER    fs < qe and fe > qs     gap 0
    LEFT    fe <= qs                gap qs - fe + 1
    RIGHT   fs >= qe                gap fs - qe + 1         (adjacent intervals: gap 1, as in bedtools)

`ignore_overlaps` removes the OVER class from the candidates; side "left" removes RIGHT, side "right" removes LEFT, OVER
counts for every side.  The answer of a region is every candidate of minimal gap in ascending index position; a region without
candidates, and a row with qs >= qe, has an empty answer.  The signed distance of an answered root is -gap (LEFT), +gap
(RIGHT) or 0 (OVER).

brute() is O(regions x roots): it classifies every root against every region and searches nothing.
"""
import numpy as np

U32_MAX = 2 ** 32 - 1
IGNORE_OVERLAPS, LEFT_ONLY, RIGHT_ONLY = 1, 2, 4
# the six flag combinations: (ignore_overlaps, side)
COMBOS = [(ig, side) for ig in (False, True) for side in ("both", "left", "right")]


def flags_of(ignore_overlaps, side):
    return (IGNORE_OVERLAPS if ignore_overlaps else 0) | {"both": 0, "left": LEFT_ONLY, "right": RIGHT_ONLY}[side]


def index_arrays(n_seq, roots):
    """roots: (n, 3) rows (seqid, start, end) in builder order -> chr_offsets[n_seq + 1], start, end, root_fid, grouped by seqid
    in builder order (what gffx_hip_index_create takes); root_fid = the row's number in `roots`."""
    roots = np.asarray(roots, np.uint32).reshape(-1, 3)
    order = np.argsort(roots[:, 0], kind="stable")
    co = np.zeros(n_seq + 1, np.uint32)
    np.add.at(co, roots[:, 0].astype(np.int64) + 1, 1)
    return np.cumsum(co).astype(np.uint32), roots[order, 1].copy(), roots[order, 2].copy(), order.astype(np.uint32)


def position_order(roots):
    """The rows of `roots` in index position order over all seqids: by seqid, then start, stable."""
    roots = np.asarray(roots, np.uint32).reshape(-1, 3)
    return np.lexsort((roots[:, 1], roots[:, 0]))  # (lexsort is stable)


def end_table(n_seq, roots):
    """(e_end, e_pos): the ends sorted stably by (seqid, end) and the index position each came from."""
    roots = np.asarray(roots, np.uint32).reshape(-1, 3)
    by_pos = roots[position_order(roots)]
    o = np.lexsort((by_pos[:, 2], by_pos[:, 0]))
    return by_pos[o, 2].copy(), o.astype(np.uint32)


def brute(n_seq, roots, regions, ignore_overlaps=False, side="both"):
    """counts[nq] u32, offsets[nq + 1] u64, triples[pairs, 3] u32 (root_fid, fs, fe), gaps[nq] u32 (0 where the count is 0),
    positions[pairs] (index position over all seqids) and distances[pairs] int64.  A region with seqid >= n_seq: ValueError."""
    roots = np.asarray(roots, np.uint32).reshape(-1, 3)
    regions = np.asarray(regions, np.uint32).reshape(-1, 3)
    if len(regions) and int(regions[:, 0].max()) >= n_seq:
        raise ValueError("chr out of range")
    order = position_order(roots)
    R = roots[order].astype(np.int64)
    Q = regions.astype(np.int64)
    nq = len(Q)
    counts = np.zeros(nq, np.int64)
    gaps = np.zeros(nq, np.int64)
    per_seq = []
    for c in np.unique(Q[:, 0]) if nq else []:
        pos = np.nonzero(R[:, 0] == c)[0]
        rows = np.nonzero(Q[:, 0] == c)[0]
        if not len(pos):
            continue
        S, E = R[pos, 1][None, :], R[pos, 2][None, :]
        qs, qe = Q[rows, 1][:, None], Q[rows, 2][:, None]
        over = (S < qe) & (E > qs)
        left = ~over & (E <= qs)
        right = ~over & ~left
        gap = np.where(over, 0, np.where(left, qs - E + 1, S - qe + 1))
        cand = (over & (not ignore_overlaps)) | (left & (side != "right")) | (right & (side != "left"))
        cand &= qs < qe
        big = np.int64(2) ** 40
        g = np.where(cand, gap, big)
        mn = g.min(axis=1)
        ans = cand & (g == mn[:, None])
        counts[rows] = ans.sum(axis=1)
        gaps[rows] = np.where(mn < big, mn, 0)
        ri, pj = np.nonzero(ans)  # (row-major: by region, then ascending position)
        dist = np.where(over[ri, pj], 0, np.where(left[ri, pj], -gap[ri, pj], gap[ri, pj]))
        per_seq.append((rows[ri], pos[pj], dist))
    offsets = np.zeros(nq + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    positions = np.zeros(total, np.int64)
    distances = np.zeros(total, np.int64)
    for qrow, p, d in per_seq:
        first = np.r_[True, qrow[1:] != qrow[:-1]]
        start_of_run = np.maximum.accumulate(np.where(first, np.arange(len(qrow)), 0))
        dest = offsets[qrow] + (np.arange(len(qrow)) - start_of_run)
        positions[dest] = p
        distances[dest] = d
    assert int(gaps.max(initial=0)) <= U32_MAX
    triples = np.stack([order[positions].astype(np.uint32), R[positions, 1].astype(np.uint32), R[positions, 2].astype(np.uint32)], axis=1) \
        if total else np.zeros((0, 3), np.uint32)
    return counts.astype(np.uint32), offsets.astype(np.uint64), triples, gaps.astype(np.uint32), positions, distances


# ---- the worked example (the issue's table): roots A [100,200), B [150,160) inside A, C [300,400), D [300,350) on seqid 0 ----
TABLE_ROOTS = np.array([[0, 100, 200], [0, 150, 160], [0, 300, 400], [0, 300, 350]], np.uint32)
TABLE_NAMES = "ABCD"  # root_fid -> name
TABLE_REGIONS = np.array([[0, 220, 240], [0, 165, 170], [0, 250, 251], [0, 249, 251], [0, 200, 300]], np.uint32)
# per flag combination and region: the answered roots in index position order, each with its signed distance -- BY HAND
TABLE_BY_HAND = {
    (False, "both"): [[("A", -21)], [("A", 0)], [("C", 50), ("D", 50)], [("A", -50), ("C", 50), ("D", 50)], [("A", -1), ("C", 1), ("D", 1)]],
    (True, "both"): [[("A", -21)], [("B", -6)], [("C", 50), ("D", 50)], [("A", -50), ("C", 50), ("D", 50)], [("A", -1), ("C", 1), ("D", 1)]],
    (False, "left"): [[("A", -21)], [("A", 0)], [("A", -51)], [("A", -50)], [("A", -1)]],
    (True, "left"): [[("A", -21)], [("B", -6)], [("A", -51)], [("A", -50)], [("A", -1)]],
    (False, "right"): [[("C", 61), ("D", 61)], [("A", 0)], [("C", 50), ("D", 50)], [("C", 50), ("D", 50)], [("C", 1), ("D", 1)]],
    (True, "right"): [[("C", 61), ("D", 61)], [("C", 131), ("D", 131)], [("C", 50), ("D", 50)], [("C", 50), ("D", 50)], [("C", 1), ("D", 1)]],
}


def _ties(n, what):
    # 40 roots with one start (ends differ) / with one end (starts differ), a far root on either side, and a second seqid
    if what == "start":
        rows = [[0, 5000, 5001 + 7 * ((i * 13) % n)] for i in range(n)]
    else:
        rows = [[0, 5000 + 3 * ((i * 13) % n), 9000] for i in range(n)]
    return np.array([[0, 10, 20]] + rows + [[0, 20000, 20010], [1, 1, 2]], np.uint32)


# name -> (n_seq, roots in builder order, regions)
HAND = {
    "table": (1, TABLE_ROOTS, TABLE_REGIONS),
    "seqid_without_roots": (3, np.array([[0, 10, 20], [2, 30, 40]], np.uint32), np.array([[1, 0, 100], [1, 5, 6], [0, 50, 60], [2, 0, 5]], np.uint32)),
    "seqid_with_one_root": (2, np.array([[1, 100, 200]], np.uint32),
                            np.array([[1, 0, 50], [1, 0, 100], [1, 99, 101], [1, 150, 160], [1, 199, 300], [1, 200, 201], [1, 500, 501], [0, 1, 2]], np.uint32)),
    "before_and_after_every_root": (1, np.array([[0, 1000, 1100], [0, 1050, 1300], [0, 1200, 1250]], np.uint32),
                                    np.array([[0, 0, 10], [0, 0, 1000], [0, 999, 1000], [0, 1300, 1301], [0, 5000, 6000], [0, 1301, U32_MAX]], np.uint32)),
    "forty_roots_with_one_start": (2, _ties(40, "start"),
                                   np.array([[0, 100, 200], [0, 4999, 5000], [0, 4000, 5001], [0, 5300, 5310], [0, 6000, 6001], [0, 0, 5], [0, 30000, 30001],
                                             [0, 21, 4999]], np.uint32)),
    "forty_roots_with_one_end": (2, _ties(40, "end"),
                                 np.array([[0, 9000, 9001], [0, 9500, 9600], [0, 14000, 15000], [0, 5050, 5051], [0, 100, 200], [0, 8999, 9000],
                                           [0, 14504, 14506]], np.uint32)),
    "coordinate_edges": (1, np.array([[0, 0, 1], [0, 5, U32_MAX], [0, U32_MAX - 1, U32_MAX], [0, 7, 8]], np.uint32),
                         np.array([[0, 0, 1], [0, 1, 2], [0, 1, 5], [0, 0, U32_MAX], [0, U32_MAX - 1, U32_MAX], [0, U32_MAX - 2, U32_MAX - 1], [0, 2, 3],
                                   [0, 8, 9]], np.uint32)),
    "far_apart": (1, np.array([[0, 0, 0], [0, U32_MAX - 1, U32_MAX - 1]], np.uint32),
                  np.array([[0, U32_MAX - 1, U32_MAX], [0, 0, 1], [0, 1, 2], [0, 5, U32_MAX - 5]], np.uint32)),
    "empty_and_inverted_regions": (1, TABLE_ROOTS, np.array([[0, 150, 150], [0, 240, 220], [0, 0, 0], [0, U32_MAX, 0], [0, 220, 240]], np.uint32)),
}

# answers of some of the other cases, worked by hand: (case, (ignore_overlaps, side)) -> per region [(root_fid, distance), ...]
BY_HAND = {
    ("seqid_without_roots", (False, "both")): [[], [], [(0, -31)], [(1, 26)]],
    ("seqid_with_one_root", (False, "both")): [[(0, 51)], [(0, 1)], [(0, 0)], [(0, 0)], [(0, 0)], [(0, -1)], [(0, -301)], []],
    ("seqid_with_one_root", (True, "left")): [[], [], [], [], [], [(0, -1)], [(0, -301)], []],
    ("before_and_after_every_root", (False, "both")): [[(0, 991)], [(0, 1)], [(0, 1)], [(1, -1)], [(1, -3701)], [(1, -2)]],
    ("before_and_after_every_root", (False, "left")): [[], [], [], [(1, -1)], [(1, -3701)], [(1, -2)]],
    ("coordinate_edges", (True, "both")): [[(1, 5)], [(0, -1)], [(0, -1), (1, 1)], [], [(3, -(U32_MAX - 8))], [(2, 1)], [(0, -2)], [(3, -1)]],
    ("far_apart", (False, "both")): [[(1, -1)], [(0, -1)], [(0, -2)], [(1, 5)]],
    ("far_apart", (False, "right")): [[], [(1, U32_MAX - 1)], [(1, U32_MAX - 2)], [(1, 5)]],
    ("far_apart", (False, "left")): [[(1, -1)], [(0, -1)], [(0, -2)], [(0, -6)]],
    ("empty_and_inverted_regions", (False, "both")): [[], [], [], [], [(0, -21)]],
}


def answers(n_seq, roots, regions, ignore_overlaps, side):
    """brute() as per-region lists [(root_fid, distance), ...]."""
    counts, offsets, triples, _, _, dist = brute(n_seq, roots, regions, ignore_overlaps, side)
    return [[(int(triples[k, 0]), int(dist[k])) for k in range(int(offsets[i]), int(offsets[i + 1]))] for i in range(len(counts))]


def random_world(seed=7, n_roots=400, n_regions=3000, n_seq=3):
    """A few hundred roots on three seqids (dense, with nested and tied coordinates) and a few thousand regions around them."""
    rng = np.random.default_rng(seed)
    roots = np.empty((n_roots, 3), np.uint32)
    roots[:, 0] = rng.integers(0, n_seq, n_roots)
    roots[:, 1] = rng.integers(0, 60, n_roots) * 100 + rng.integers(0, 3, n_roots) * 7  # (many ties in start)
    roots[:, 2] = roots[:, 1] + rng.choice([0, 1, 30, 93, 100, 400, 2500], n_roots)     # (... and in end; empty and long roots)
    regions = np.empty((n_regions, 3), np.uint32)
    regions[:, 0] = rng.integers(0, n_seq, n_regions)
    regions[:, 1] = rng.integers(0, 9000, n_regions)
    regions[:, 2] = regions[:, 1] + rng.choice([1, 2, 7, 100, 1000], n_regions)
    return n_seq, roots, regions
