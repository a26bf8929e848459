"""The definition of `gffx coverage`'s region union and of a segment's covered bases, exact at any u32 coordinate, and the
builders of the hand-shaped inputs of tests/test_coverage_edges_gpu.py (held to account in tests/test_coverage_edges_cpu.py).

merge_rows   per seqid: stable sort by start, running maximum of the ends, a record heads a span when it is the seqid's first or
             starts beyond the running maximum before it (merge_intervals, commands/coverage.rs:92-109: `s <= current end` merges)
covered      F(b) - F(a) with F(x) = pb[k-1] + min(x, ue[k-1]) - us[k-1], k = #{us < x}: no array over bases
Neither uses the device's tricks: the seqids are handled one by one (no packed (seqid, end) value), the searches are plain
np.searchsorted (no directory), all arithmetic is int64.

A builder returns the rows IN SORTED ORDER (by seqid, then start, ties in the order given) and says at which sorted position its
border, break or pair sits; `place` hands them to the device under a fixed permutation that keeps ties in order, so the device's
stable sort puts every row back on the position the builder names (`sorted_rows` is that sort, restated).

The device code these shapes are tied to (gffx_amd/csrc/device/coverage.hip): a thread owns 4 consecutive
sorted records, a wave 256, a tile 1024; k_union_carry walks 256 tiles (262 144 records) per step; one fold takes 8 Mi new rows;
the sort runs one pass per byte of the start and 1 / 2 / 3 passes for <= 256 / <= 65 536 / more seqids.
"""
import numpy as np

U32_MAX = 0xFFFFFFFF
THREAD, WAVE, TILE, CARRY_STEP = 4, 256, 1024, 262144
UNION_FOLD = 8 << 20
EDGE_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 262143, 262144, 262145, 263169)
EDGE_POSITIONS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 262144)


# ------------------------------------------------------------------------------------------------------------ the reference
def rows_of(seq, start, end):
    r = np.empty((len(start), 3), np.uint32)
    r[:, 0], r[:, 1], r[:, 2] = seq, start, end
    return r


def sorted_rows(rows):
    """The rows as a stable sort by (seqid, start) leaves them."""
    rows = np.asarray(rows, np.uint32).reshape(-1, 3)
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def merge_rows(rows, n_seq):
    """(u_off u64 [n_seq + 1], us u32, ue u32, pb u64) of (n, 3) rows {seqid, start, end}."""
    r = sorted_rows(rows)
    seq, start, end = r[:, 0].astype(np.int64), r[:, 1].astype(np.int64), r[:, 2].astype(np.int64)
    assert not len(seq) or int(seq.max()) < n_seq
    first = np.concatenate([[0], np.nonzero(seq[1:] != seq[:-1])[0] + 1]) if len(seq) else np.zeros(0, np.int64)
    present, count = seq[first], np.diff(np.concatenate([first, [len(seq)]]))
    n_spans = np.zeros(n_seq + 1, np.int64)
    us, ue, pb = [], [], []
    for c, lo, m in zip(present.tolist(), first.tolist(), count.tolist()):
        s, e = start[lo:lo + m], end[lo:lo + m]
        cm = np.maximum.accumulate(e)
        head = np.ones(m, bool)
        head[1:] = s[1:] > cm[:-1]
        at = np.nonzero(head)[0]
        last = np.concatenate([at[1:] - 1, [m - 1]])  # the span's last record
        a, b = s[at], cm[last]
        us.append(a), ue.append(b), pb.append(np.cumsum(b - a) - (b - a))
        n_spans[c + 1] = len(at)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return np.cumsum(n_spans).astype(np.uint64), cat(us).astype(np.uint32), cat(ue).astype(np.uint32), cat(pb).astype(np.uint64)


def covered(spans, seg_seq, seg_start, seg_end):
    """u32 covered bases of the segments [seg_start, seg_end) under `spans` = (u_off, us, ue, pb)."""
    u_off, us, ue, pb = (np.asarray(x).astype(np.int64) for x in spans)
    q = np.asarray(seg_seq).astype(np.int64)
    a, b = np.asarray(seg_start).astype(np.int64), np.asarray(seg_end).astype(np.int64)
    out = np.zeros(len(q), np.int64)

    def below(s, e, p, x):
        k = np.searchsorted(s, x, "left")
        j = np.maximum(k - 1, 0)
        return np.where(k == 0, 0, p[j] + np.minimum(x, e[j]) - s[j])

    for c in np.unique(q).tolist():
        lo, hi = int(u_off[c]), int(u_off[c + 1])
        if hi == lo:
            continue
        i = np.nonzero(q == c)[0]
        s, e, p = us[lo:hi], ue[lo:hi], pb[lo:hi]
        out[i] = np.where(a[i] < b[i], below(s, e, p, b[i]) - below(s, e, p, a[i]), 0)
    assert not len(out) or (0 <= int(out.min()) and int(out.max()) <= U32_MAX)
    return out.astype(np.uint32)


def directory_rule(starts):
    """(shift, nb) of the directory over one seqid's span starts (coverage.hip: the smallest shift with
    (vmax >> shift) + 1 <= max(2 n_u, 16); nb = (vmax >> shift) + 1)."""
    vmax, budget = int(max(starts)), max(2 * len(starts), 16)
    shift = 0
    while (vmax >> shift) + 1 > budget:
        shift += 1
    return shift, (vmax >> shift) + 1


def seqid_sort_passes(n_seq):
    """Passes the union's sort spends on the seqid: one per byte that n_seq values need."""
    k = 1
    while k < 4 and n_seq > (1 << (8 * k)):
        k += 1
    return k


# ---------------------------------------------------------------------------------------------------- from sorted to shuffled
def place(rows_sorted, seed):
    """The sorted rows under a fixed permutation; rows with equal (seqid, start) keep their relative order, so a stable sort
    by (seqid, start) gives `rows_sorted` back, row for row."""
    r = np.asarray(rows_sorted, np.uint32).reshape(-1, 3)
    n = len(r)
    if n == 0:
        return r.copy()
    pos = np.random.default_rng(seed).permutation(n)  # input position of sorted row i
    new_key = np.ones(n, bool)
    new_key[1:] = (r[1:, 0] != r[:-1, 0]) | (r[1:, 1] != r[:-1, 1])
    pos = pos[np.lexsort((pos, np.cumsum(new_key)))]  # ascending inside every run of equal keys
    out = np.empty_like(r)
    out[pos] = r
    return out


# ----------------------------------------------------------------------------------------------------------------- A: shapes
SHAPES = ("disjoint", "chain", "broken_chain", "first_covers_all", "pairs", "pairs_odd")


def shape_rows(shape, n, seq=1):
    """(sorted rows on one seqid, number of spans)."""
    i = np.arange(n, dtype=np.int64)
    w = 1 + (i % 5)
    if shape == "disjoint":
        s = 10 * i + 5
        e, spans = s + w, n
    elif shape == "chain":  # s[i + 1] == e[i]
        e = np.cumsum(w) + 3
        s, spans = e - w, 1
    elif shape == "broken_chain":  # s[i + 1] == e[i] + 1
        e = np.cumsum(w + 1) + 3
        s, spans = e - w, n
    elif shape == "first_covers_all":  # only record 0 knows the span's end
        s, e = 10 + 3 * i, 12 + 3 * i
        s[0], e[0], spans = 0, 0xFFFFFFF0, 1
    else:  # pairs: records 2k, 2k + 1 touch (pairs_odd: 2k + 1, 2k + 2), one base free behind every pair
        j = i + (1 if shape == "pairs_odd" else 0)
        s = 12 * (j // 2) + 7 * (j % 2)
        e = s + np.where(j % 2 == 0, 7, 4)
        spans = int(np.count_nonzero(j % 2 == 0)) + (1 if shape == "pairs_odd" and n else 0)
    return rows_of(seq, s, e), spans


# ------------------------------------------------------------------------------------------- A: one event at sorted position p
EVENTS = ("seqid_border", "span_break", "touching_pair", "carried_end")


def event_rows(event, p, n=None):
    """(sorted rows, n_seq, number of spans): the event sits between sorted records p - 1 and p; nothing like it anywhere else."""
    n = p + 1030 if n is None else n
    assert 1 <= p < n
    i = np.arange(n, dtype=np.int64)
    seq = np.full(n, 1, np.int64)
    if event == "seqid_border":
        # every record overlaps the next inside its seqid; seqid 2 restarts at small coordinates, far below seqid 1's running
        # maximum: only the seqid tells records p - 1 and p apart
        seq[p:] = 2
        s = np.where(i < p, 1000 + 10 * i, 10 * (i - p))
        e, spans = s + 15, 2
    elif event == "span_break":  # one chain, broken by ONE free base in front of record p
        w = 1 + (i % 5)
        e = np.cumsum(w) + 3 + (i >= p)
        s, spans = e - w, 2
    elif event == "touching_pair":  # all disjoint (one base free), except that record p starts where record p - 1 ends
        w = 1 + (i % 5)
        e = np.cumsum(w + 1) + 3 - (i >= p)
        s, spans = e - w, n - 1
    else:  # carried_end: record 0 holds the largest end of the span that record p - 1 closes; record p starts one base behind it
        big = 40 * n
        s, e = 10 + 3 * i, 12 + 3 * i
        s[0], e[0] = 0, big
        s[p:] = big + 1 + 10 * (i[p:] - p)
        e[p:] = s[p:] + 4
        spans = 1 + (n - p)
    return rows_of(seq, s, e), 4, spans


def restart_rows(pos):
    """Seqid 1 = sorted records [0, pos): small disjoint rows, then [0xFFFFFF00, 0xFFFFFFFF) and [0xFFFFFFFE, 0xFFFFFFFF); seqid 2
    from sorted position pos on: small rows of its own.  -> (sorted rows, n_seq)."""
    assert pos >= 2
    n = pos + 40
    i = np.arange(n, dtype=np.int64)
    seq = np.where(i < pos, 1, 2)
    s = np.where(i < pos, 20 * i + 3, 9 * (i - pos) + 1)
    e = s + np.where(i % 3 == 0, 9, 4)  # (seqid 2: every third row touches the next)
    s[pos - 2], e[pos - 2] = 0xFFFFFF00, U32_MAX
    s[pos - 1], e[pos - 1] = 0xFFFFFFFE, U32_MAX
    return rows_of(seq, s, e), 4


def equal_start_rows(border, long_first):
    """Disjoint rows; sorted records border - 1 and border share a start, one ends at +5 and one at +50 (long_first: which comes
    first); record border + 1 starts inside the long one only, record border + 2 beyond both.  -> (sorted rows, n_seq, spans)"""
    n = border + 1030
    i = np.arange(n, dtype=np.int64)
    s = 100 * i
    e = s + 7
    s[border] = s[border - 1]
    e[border - 1], e[border] = (s[border] + 50, s[border] + 5) if long_first else (s[border] + 5, s[border] + 50)
    s[border + 1] = s[border] + 20
    e[border + 1] = s[border + 1] + 3
    return rows_of(1, s, e), 3, n - 2


# ------------------------------------------------------------------------------------------------------- B: the sort's plan
SORT_N_SEQ = (1, 255, 256, 257, 65535, 65536, 65537)
START_KINDS = ("low_byte", "top_byte", "all_bytes")


def sort_plan_seqids(n_seq):
    return sorted({c for c in (0, n_seq - 1, 255, 256, 65535, 65536) if c < n_seq})


def sort_plan_rows(n_seq, kind, n=6000, seed=0):
    """n shuffled rows (more than one sort tile of 4096) on sort_plan_seqids(n_seq)."""
    rng = np.random.default_rng([seed, n_seq, START_KINDS.index(kind)])
    seq = rng.choice(sort_plan_seqids(n_seq), n)
    if kind == "low_byte":  # bytes 1, 2 and 3 of every start are 0: three copy passes
        s = rng.integers(0, 256, n)
        e = s + rng.integers(1, 4, n)
    elif kind == "top_byte":  # k << 24: bytes 0, 1 and 2 are 0, byte 3 takes all 256 values
        s = np.arange(n, dtype=np.int64) % 256 << 24
        rng.shuffle(s)
        e = s + rng.choice([1, 1000, 1 << 24, (1 << 24) + 1], n)
    else:
        s = rng.integers(0, U32_MAX, n)  # <= 0xFFFFFFFE
        s[:4] = (0, U32_MAX - 1, 1 << 31, (1 << 24) - 1)
        e = s + rng.choice([1, 300, 1 << 16, 1 << 22], n)
    return rows_of(seq, s, np.minimum(e, U32_MAX))


# ----------------------------------------------------------------------------------------------- E: unions for the directory
DIRECTORY_CASES = ("one_span_per_seqid", "eight_spans", "nine_spans", "starts_on_bin_edges", "empty_bins_in_the_middle",
                   "empty_first_bins", "spread_to_the_top", "more_than_2_31_bases")
ONE_SPAN_STARTS = (0, 15, 16, 17, (1 << 28) - 1, 1 << 28, 0xFFFFFFFE)


def directory_case(name):
    """(n_seq, rows): disjoint, non-touching rows, so the rows ARE the spans."""
    if name == "one_span_per_seqid":
        st = np.array(ONE_SPAN_STARTS, np.int64)
        return len(st) + 1, rows_of(np.arange(len(st)), st, np.minimum(st + 40, U32_MAX))
    if name in ("eight_spans", "nine_spans"):  # the same largest start, 17: 18 bins fit a budget of 18 and not one of 16
        st = np.arange(3 if name == "eight_spans" else 1, 18, 2, dtype=np.int64)
        return 2, rows_of(1, st, st + 1)
    if name == "starts_on_bin_edges":
        st = np.array([0, 1, 2, 3, 4, 7, 8, 12, 13], np.int64) << 24
        en = st + np.array([1, 1 << 23, 5, 77, (2 << 24) + 5, 1 << 20, (3 << 24), 9, 1 << 25], np.int64)
        return 2, rows_of(0, st, en)
    if name == "empty_bins_in_the_middle":
        st = np.array([10, 20, 30, 3_000_000_000, 3_000_000_100, 4_000_000_000], np.int64)
        return 3, rows_of(2, st, st + 5)
    if name == "empty_first_bins":
        st = np.array([(1 << 30) + 5, 1 << 31, 3 << 30], np.int64)
        return 2, rows_of(1, st, st + np.array([1 << 29, 1000, 1 << 29], np.int64))
    if name == "spread_to_the_top":
        st = np.arange(40, dtype=np.int64) * 110_000_000 + 12345
        rows = rows_of(0, st, st + 1 + (np.arange(40) % 4) * 25_000_000)
        rows[-1] = (0, 0xFFFFFFF0, U32_MAX)
        return 1, rows
    assert name == "more_than_2_31_bases"
    return 2, np.array([[1, 0, (1 << 31) + 10], [1, (1 << 31) + 20, U32_MAX]], np.uint32)


def probe_points(us, ue):
    """Every x the issue lists for one seqid's spans: around every span's start and end, around every bin edge, 0 and 2^32 - 1."""
    shift, nb = directory_rule(us)
    xs = {0, U32_MAX}
    for v in list(map(int, us)) + list(map(int, ue)) + [b << shift for b in range(nb + 1)]:
        xs.update((v - 1, v, v + 1))
    return np.array(sorted(x for x in xs if 0 <= x <= U32_MAX), np.int64)


def probe_segments(spans, n_seq):
    """Every pair (a, b) of probe points as a segment, a >= b included, on every seqid with spans; a few on the others."""
    u_off, us, ue, _ = spans
    q, a, b = [], [], []
    for c in range(n_seq):
        lo, hi = int(u_off[c]), int(u_off[c + 1])
        if hi == lo:
            q.append(np.full(3, c, np.int64)), a.append(np.array([0, 5, 0])), b.append(np.array([U32_MAX, 9, 0]))
            continue
        xs = probe_points(us[lo:hi], ue[lo:hi])
        aa, bb = np.meshgrid(xs, xs, indexing="ij")
        q.append(np.full(aa.size, c, np.int64)), a.append(aa.ravel()), b.append(bb.ravel())
    return np.concatenate(q).astype(np.uint32), np.concatenate(a).astype(np.uint32), np.concatenate(b).astype(np.uint32)


# -------------------------------------------------------------------------------------------------------- D: the fold's split
def fold_split_rows(n=UNION_FOLD + 1025):
    """One add that needs two folds.  40 clusters of heavily overlapping rows (one span each) on two seqids and an isolated
    one-base row every 50 000 rows; the last 1025 rows -- the second fold -- bring a cluster of their own beyond everything
    before, isolated rows, and rows that lengthen the first fold's last span on seqid 0."""
    i = np.arange(n, dtype=np.int64)
    h = (i * 2654435761) % (1 << 32)
    cluster = h % 40
    seq = cluster % 2
    s = cluster * 20_000_000 + (h >> 8) % 50_000
    e = s + 20_000
    lone = i % 50_000 == 49_999
    s[lone] = 2_000_000_000 + 3 * i[lone]
    e[lone] = s[lone] + 1
    seq[lone] = 2
    t = i >= UNION_FOLD  # the second fold
    k = i[t] - UNION_FOLD
    seq[t] = np.where(k % 4 == 0, 2, np.where(k % 4 == 1, 0, 1))
    s[t] = np.where(k % 4 == 0, 3_000_000_000 + 3 * k,                # isolated
                    np.where(k % 4 == 1, 38 * 20_000_000 + 60_000 + 10 * k,  # touches / overlaps seqid 0's last span (cluster 38)
                             3_500_000_000 + 7 * k))                     # a cluster only the second fold has
    e[t] = np.where(k % 4 == 0, s[t] + 1, np.where(k % 4 == 1, s[t] + 5000, s[t] + 100))
    return rows_of(seq, s, e)
