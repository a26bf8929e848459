"""The definition of `gffx annotate` restated twice, and a hand-written example.

T layers of rows (layer, seqid, start, end) in priority order; a row covers [start, end).  class(x) on a seqid = the smallest
layer with a row that covers x, or T.  The class map of a seqid = the points (pos_i, class_i): pos ascending, class_i the
class on [pos_i, pos_{i+1}), class_i != class_{i-1}, the first class not T, the last class T.  cb[k][i] = the bases of class k
on all points before point i, over all seqids.  A region (c, qs, qe): bases_k for k = 0 .. T, and its class = the smallest
k < T with bases_k > 0, or T; qs >= qe gives zeros and T; c >= n_seq is refused.

``dense``   an array over the bases of every seqid (small coordinates only): classes are written base by base, lowest
            priority first; points are read off where neighbours differ; a region's answer is a count over its slice.
``sparse``  per (seqid, layer) a dict position -> +1 / -1; one sweep over the sorted positions with a depth per layer; a
            region's answer walks the pieces of its seqid.  Reaches 2^32 - 1; shares no search and no array with ``dense``.
"""
import numpy as np

U32_MAX = 0xFFFFFFFF
E_INVALID, E_CHR_RANGE, E_STATE = -1, -5, -6


def _rows(rows):
    return np.asarray(rows, np.int64).reshape(-1, 4)


def _check(n_seq, T, rows):
    r = _rows(rows)
    if len(r) and (np.any(r[:, 0] >= T) or np.any(r[:, 1] >= n_seq)):
        raise ValueError("range")
    if len(r) and np.any(r[:, 2] >= r[:, 3]):
        raise ValueError("inverted")
    return r


def _pack(n_seq, T, per_seq):
    """per_seq: {seqid: [(pos, cls), ...]} -> (p_off u64, pos u32, cls u8, cb u64 [T, n])."""
    p_off = np.zeros(n_seq + 1, np.uint64)
    pos, cls = [], []
    for c in sorted(per_seq):
        p_off[c + 1] = len(per_seq[c])
        pos += [p for p, _ in per_seq[c]]
        cls += [k for _, k in per_seq[c]]
    p_off = np.cumsum(p_off).astype(np.uint64)
    n = len(pos)
    cb = np.zeros((T, n), np.uint64)
    acc = [0] * T
    seq_of = np.repeat(np.arange(n_seq), np.diff(p_off.astype(np.int64))) if n else np.zeros(0, np.int64)
    for i in range(n):
        for k in range(T):
            cb[k, i] = acc[k]
        if cls[i] < T and i + 1 < n and seq_of[i + 1] == seq_of[i]:
            acc[cls[i]] += pos[i + 1] - pos[i]
    return p_off, np.array(pos, np.uint32), np.array(cls, np.uint8), cb


def dense(n_seq, T, rows, regions, size=4096):
    """-> (p_off, pos, cls, cb, counts [nq, T + 1] u32, region class u8).  Coordinates must stay below `size`."""
    r = _check(n_seq, T, rows)
    grid = np.full((n_seq, size + 1), T, np.int64)  # (base `size` stays T: every seqid ends outside all rows)
    for k in range(T - 1, -1, -1):
        for _, c, s, e in r[r[:, 0] == k]:
            assert e <= size
            grid[c, s:e] = k
    per_seq = {}
    for c in range(n_seq):
        prev, pts = T, []
        for x in range(size + 1):
            if grid[c, x] != prev:
                pts.append((x, int(grid[c, x])))
                prev = grid[c, x]
        if pts:
            per_seq[c] = pts
    q = np.asarray(regions, np.int64).reshape(-1, 3)
    counts, best = np.zeros((len(q), T + 1), np.uint32), np.full(len(q), T, np.uint8)
    for i, (c, qs, qe) in enumerate(q):
        if c >= n_seq:
            raise ValueError("range")
        if qs >= qe:
            continue
        inside = grid[c, qs:min(qe, size)]
        counts[i] = np.bincount(inside, minlength=T + 1)
        counts[i, T] += qe - qs - len(inside)
        hit = np.flatnonzero(counts[i, :T])
        if len(hit):
            best[i] = hit[0]
    return _pack(n_seq, T, per_seq) + (counts, best)


def sparse_map(n_seq, T, rows):
    """{seqid: [(pos, cls), ...]} by a sweep over per-layer deltas."""
    r = _check(n_seq, T, rows)
    delta = {}
    for k, c, s, e in r.tolist():
        d = delta.setdefault(c, {})
        d[(s, k)] = d.get((s, k), 0) + 1
        d[(e, k)] = d.get((e, k), 0) - 1
    per_seq = {}
    for c, d in delta.items():
        depth, prev, pts = [0] * T, T, []
        keys = sorted(d)
        for j, (x, k) in enumerate(keys):
            depth[k] += d[(x, k)]
            if j + 1 < len(keys) and keys[j + 1][0] == x:
                continue
            now = next((m for m in range(T) if depth[m] > 0), T)
            if now != prev:
                pts.append((x, now))
                prev = now
        assert prev == T and not any(depth)
        per_seq[c] = pts
    return per_seq


def sparse(n_seq, T, rows, regions):
    """-> the same tuple as ``dense``, for any u32 coordinates."""
    per_seq = sparse_map(n_seq, T, rows)
    q = np.asarray(regions, np.int64).reshape(-1, 3)
    counts, best = np.zeros((len(q), T + 1), np.uint32), np.full(len(q), T, np.uint8)
    for i, (c, qs, qe) in enumerate(q.tolist()):
        if c >= n_seq:
            raise ValueError("range")
        if qs >= qe:
            continue
        got = [0] * (T + 1)
        pts = per_seq.get(c, [])
        for j, (x, k) in enumerate(pts):  # the piece [x, next x) has class k; before the first and behind the last: T
            nxt = pts[j + 1][0] if j + 1 < len(pts) else None
            lo, hi = max(x, qs), qe if nxt is None else min(nxt, qe)
            if hi > lo:
                got[k] += hi - lo
        got[T] = qe - qs - sum(got[:T])
        counts[i] = got
        best[i] = next((m for m in range(T) if got[m]), T)
    return _pack(n_seq, T, per_seq) + (counts, best)


def sparse_np(n_seq, T, rows, regions):
    """``sparse`` restated over whole arrays, for maps of 10^5 .. 10^6 events (``sparse`` walks every point for every region):
    the 2 n events sorted by (seqid, position); per layer its depth behind every event by a cumsum of its +1 / -1; the class
    behind the last event of every (seqid, position); a point where that class differs from the one before (T before the first:
    a seqid ends at depth 0 everywhere).  A region's bases of class k are B_k(qe) - B_k(qs), B_k(x) = the bases of class k below
    x on the region's seqid: cb at the last point at or before x, plus the piece from that point to x if its class is k.
    tests/test_annotate_cpu.py pins it to ``sparse``."""
    r = _check(n_seq, T, rows)
    q = np.asarray(regions, np.int64).reshape(-1, 3)
    if len(q) and np.any(q[:, 0] >= n_seq):
        raise ValueError("range")
    m = len(r)
    seq, pos = np.concatenate([r[:, 1], r[:, 1]]), np.concatenate([r[:, 2], r[:, 3]])
    lay, d = np.concatenate([r[:, 0], r[:, 0]]), np.concatenate([np.ones(m, np.int64), -np.ones(m, np.int64)])
    order = np.lexsort((pos, seq))
    seq, pos, lay, d = seq[order], pos[order], lay[order], d[order]
    now = np.full(2 * m, T, np.int64)
    for k in range(T - 1, -1, -1):  # (the smallest covering layer wins: written last)
        now[np.cumsum(np.where(lay == k, d, 0)) > 0] = k
    tail = np.ones(2 * m, bool)
    tail[:-1] = (seq[1:] != seq[:-1]) | (pos[1:] != pos[:-1])
    t_seq, t_pos, t_cls = seq[tail], pos[tail], now[tail]
    point = t_cls != np.concatenate([[T], t_cls])[:-1]
    p_seq, p_pos, p_cls = t_seq[point], t_pos[point], t_cls[point]
    n = len(p_pos)
    p_off = np.searchsorted(p_seq, np.arange(n_seq + 1)).astype(np.uint64)
    length = np.zeros(n, np.int64)
    if n:
        inside = p_seq[1:] == p_seq[:-1]
        assert np.all(p_cls[:-1][~inside] == T) and p_cls[-1] == T  # a seqid's last point has class T
        length[:-1] = np.where(inside, p_pos[1:] - p_pos[:-1], 0)
    cb = np.zeros((T, n), np.int64)
    for k in range(T):
        mine = np.where(p_cls == k, length, 0)
        cb[k] = np.cumsum(mine) - mine

    def below(c, x):  # B_k(x) for every k: [T, nq]
        first = p_off.astype(np.int64)[c]
        i = np.searchsorted((p_seq << 32) | p_pos, (c << 32) | x, side="right") - 1
        have = i >= first
        i, first = np.where(have, i, 0), np.minimum(first, max(n - 1, 0))
        out = np.zeros((T, len(c)), np.int64)
        if n:
            for k in range(T):
                out[k] = np.where(have, cb[k, i] - cb[k, first] + np.where(p_cls[i] == k, x - p_pos[i], 0), 0)
        return out

    real = q[:, 1] < q[:, 2]
    per = np.where(real, below(q[:, 0], q[:, 2]) - below(q[:, 0], q[:, 1]), 0)
    counts = np.zeros((len(q), T + 1), np.int64)
    counts[:, :T] = per.T
    counts[:, T] = np.where(real, q[:, 2] - q[:, 1], 0) - counts[:, :T].sum(1)
    best = np.where((counts[:, :T] > 0).any(1), np.argmax(counts[:, :T] > 0, 1), T) if T else np.full(len(q), T)
    return p_off, p_pos.astype(np.uint32), p_cls.astype(np.uint8), cb.astype(np.uint64), counts.astype(np.uint32), best.astype(np.uint8)


# ---- the example by hand: layers 0 = CDS, 1 = exon, 2 = gene; two seqids -----------------------------------------------------
HAND_T, HAND_N_SEQ = 3, 2
HAND_ROWS = np.array([
    [2, 0, 100, 500],   # a gene ...
    [1, 0, 150, 300],   # ... an exon inside it, sticking out of the CDS on both sides
    [1, 0, 300, 400],   # ... a second exon that touches the first
    [1, 0, 150, 300],   # ... the first exon once more (another transcript)
    [0, 0, 200, 250],   # ... the CDS, nested in the exon
    [2, 0, 600, 700],   # a second gene
    [1, 1, 0, 10],      # seqid 1: an exon from base 0 ...
    [0, 1, 10, 20],     # ... touched by a CDS of another layer
], np.uint32)
HAND_P_OFF = [0, 8, 11]
HAND_POS = [100, 150, 200, 250, 400, 500, 600, 700, 0, 10, 20]
HAND_CLS = [2, 1, 0, 1, 2, 3, 2, 3, 1, 0, 3]
HAND_CB = [[0, 0, 0, 50, 50, 50, 50, 50, 50, 50, 60],
           [0, 0, 50, 50, 200, 200, 200, 200, 200, 210, 210],
           [0, 50, 50, 50, 50, 150, 150, 250, 250, 250, 250]]
HAND_REGIONS = np.array([
    [0, 0, 100], [0, 100, 500], [0, 120, 220], [0, 260, 650], [0, 450, 620], [0, 700, 1000], [0, 200, 250], [0, 300, 300],
    [0, 400, 300], [1, 0, 30], [1, 5, 15],
], np.uint32)
HAND_COUNTS = [[0, 0, 0, 100], [50, 200, 150, 0], [20, 50, 30, 0], [0, 140, 150, 100], [0, 0, 70, 100], [0, 0, 0, 300], [50, 0, 0, 0],
               [0, 0, 0, 0], [0, 0, 0, 0], [10, 10, 0, 10], [5, 5, 0, 0]]
HAND_CLASS = [3, 0, 0, 1, 2, 3, 0, 3, 3, 0, 0]


def hand():
    return (np.array(HAND_P_OFF, np.uint64), np.array(HAND_POS, np.uint32), np.array(HAND_CLS, np.uint8), np.array(HAND_CB, np.uint64),
            np.array(HAND_COUNTS, np.uint32), np.array(HAND_CLASS, np.uint8))


def same(a, b):
    """Two result tuples are equal bit for bit (dtypes included)."""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---- cases for the shared rules and the device ---------------------------------------------------------------------------
def probe_regions(n_seq, T, rows, extra=()):
    """Regions of every kind: beginning or ending exactly on a point, one base around every point, before the first point and
    behind the last, over everything, empty and inverted, and on a seqid without points."""
    per_seq = sparse_map(n_seq, T, rows)
    out = []
    for c in sorted(per_seq)[:4] + sorted(per_seq)[-1:]:
        xs = sorted({p for p, _ in per_seq[c]})
        if len(xs) > 24:
            xs = xs[:12] + xs[-12:]
        edge = sorted({min(max(x + d, 0), U32_MAX) for x in xs for d in (-1, 0, 1)} | {0, U32_MAX})
        out += [[c, a, b] for a in edge for b in edge if a < b][:400]
        out += [[c, xs[0], xs[0]], [c, xs[-1], xs[0]], [c, 0, U32_MAX]]
        if xs[0] > 0:
            out.append([c, 0, xs[0]])
        if xs[-1] < U32_MAX:
            out.append([c, xs[-1], U32_MAX])
    empty = [c for c in (0, n_seq - 1, n_seq // 2) if c not in per_seq]
    out += [[c, 5, 500] for c in empty] + [list(e) for e in extra]
    return np.array(out, np.uint32).reshape(-1, 3)


def random_case(seed, n_seq=3, T=4, n=40, size=300):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, T + 1))
    s = rng.integers(0, size - 1, n)
    e = np.minimum(s + 1 + rng.integers(0, 40, n), size)
    rows = np.stack([rng.integers(0, T, n), rng.integers(0, n_seq, n), s, e], 1).astype(np.uint32)
    a = rng.integers(0, size + 20, 30)
    b = rng.integers(0, size + 20, 30)
    regions = np.stack([rng.integers(0, n_seq, 30), a, b], 1).astype(np.uint32)
    return n_seq, T, rows, regions


def events_case(n_events, T=2, seq=0):
    """Disjoint, non-touching rows, so every row is a span and gives two events: n_events / 2 rows (a span always gives two
    events, so the count is even)."""
    assert n_events % 2 == 0
    m = n_events // 2
    i = np.arange(m, dtype=np.int64)
    return np.stack([i % T, np.full(m, seq), 10 + 7 * i, 10 + 7 * i + 1 + (i % 5)], 1).astype(np.uint32)


# ---- the command's hand-written input: HAND_ROWS as GFF lines (1-based, closed), with lines that belong to no layer -------
GFF_NAMES = ["chrA", "chrB"]
GFF = """##gff-version 3
chrA\thand\tgene\t101\t500\t.\t+\t.\tID=g1;gene_name=G1
chrA\thand\tmRNA\t101\t500\t.\t+\t.\tID=m1;Parent=g1
chrA\thand\texon\t151\t300\t.\t+\t.\tID=e1;Parent=m1
chrA\thand\texon\t301\t400\t.\t+\t.\tID=e2;Parent=m1
chrA\thand\tCDS\t201\t250\t.\t+\t0\tID=c1;Parent=m1
chrA\thand\tmRNA\t101\t500\t.\t+\t.\tID=m2;Parent=g1
chrA\thand\texon\t151\t300\t.\t+\t.\tID=e3;Parent=m2
# a comment between the lines
chrA\thand\tgene\t601\t700\t.\t-\t.\tID=g2;gene_name=G2
chrA\thand\tmRNA\t601\t700\t.\t-\t.\tID=m3;Parent=g2
chrB\thand\tgene\t1\t20\t.\t+\t.\tID=g3;gene_name=G3
chrB\thand\tmRNA\t1\t20\t.\t+\t.\tID=m4;Parent=g3
chrB\thand\texon\t1\t10\t.\t+\t.\tID=e4;Parent=m4
chrB\thand\tCDS\t11\t20\t.\t+\t0\tID=c2;Parent=m4
"""
# (with -T CDS,exon,gene chrB's gene [0, 20) lies under its exon and CDS everywhere: the hand answers of seqid 1 stand)
BED = (b"chrA\t0\t100\nchrA\t100\t500\tpeak\nchrA\t120\t220\n# a comment\nchrA\t260\t650\nchrUn\t5\t10\nchrA\t450\t620\nchrA\t700\t1000\n"
       b"chrA\t200\t250\nchrA\t300\t300\nchrA\t400\t300\nchrB\t0\t30\nchrB\t5\t15\n")
LAYER_NAMES = ["CDS", "exon", "gene"]


def expected_text(names=LAYER_NAMES, counts=HAND_COUNTS, classes=HAND_CLASS, regions=HAND_REGIONS):
    T = len(names)
    out = ["#chr\tstart\tend\tclass\t" + "\t".join(names) + "\tnone\n"]
    for (c, s, e), row, k in zip(np.asarray(regions).tolist(), counts, classes):
        out.append("%s\t%d\t%d\t%s\t%s\n" % (GFF_NAMES[c], s, e, names[k] if k < T else ".", "\t".join(str(v) for v in row)))
    return "".join(out).encode()


def expected_summary(names=LAYER_NAMES, counts=HAND_COUNTS, classes=HAND_CLASS):
    T = len(names)
    return "".join("%s\t%d\t%d\n" % (names[k] if k < T else "none", sum(1 for c in classes if c == k), sum(r[k] for r in counts))
                   for k in range(T + 1)).encode()


BY_HAND_TEXT = (
    "#chr\tstart\tend\tclass\tCDS\texon\tgene\tnone\n"
    "chrA\t0\t100\t.\t0\t0\t0\t100\n"
    "chrA\t100\t500\tCDS\t50\t200\t150\t0\n"
    "chrA\t120\t220\tCDS\t20\t50\t30\t0\n"
    "chrA\t260\t650\texon\t0\t140\t150\t100\n"
    "chrA\t450\t620\tgene\t0\t0\t70\t100\n"
    "chrA\t700\t1000\t.\t0\t0\t0\t300\n"
    "chrA\t200\t250\tCDS\t50\t0\t0\t0\n"
    "chrA\t300\t300\t.\t0\t0\t0\t0\n"
    "chrA\t400\t300\t.\t0\t0\t0\t0\n"
    "chrB\t0\t30\tCDS\t10\t10\t0\t10\n"
    "chrB\t5\t15\tCDS\t5\t5\t0\t0\n").encode()
BY_HAND_SUMMARY = b"CDS\t5\t135\nexon\t1\t405\ngene\t1\t400\nnone\t4\t610\n"
