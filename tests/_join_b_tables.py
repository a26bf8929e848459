"""Join B's references, shared by the GPU suites (tests/test_join_b_gpu.py, tests/test_join_b_sort_gpu.py): the keep flags by the
oracle's literal linear scan (commands/intersect.rs:500-521) and the region tables as the definition builds them, in numpy."""
import numpy as np

from oracle import binding as ob


def _oracle_keep(seq, s, e, regions, n_seq, mode):
    order = np.argsort(regions[:, 0], kind="stable")
    r = regions[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(r[:, 0], minlength=n_seq))])
    out = np.zeros(len(seq), dtype=bool)
    for i in range(len(seq)):
        c = int(seq[i])
        if c >= n_seq or off[c + 1] == off[c]:
            continue
        out[i] = ob.line_predicate(int(s[i]), int(e[i]), r[off[c]:off[c + 1], 1], r[off[c]:off[c + 1], 2], int(mode))
    return out


def _host_tables(regions, n_seq):
    """The region tables as the definition builds them (numpy): stable (seqid, start) order, running max / min of the
    ends inside a seqid, the count of regions with start > end before every position, the bin directory over the starts
    (~2 bins per region, >= 16), and the ends of the start > end regions sorted per seqid."""
    r = regions[np.lexsort((regions[:, 1], regions[:, 0]))]  # (lexsort is stable: ties keep the BED order)
    n = len(r)
    q_off = np.concatenate([[0], np.cumsum(np.bincount(r[:, 0], minlength=n_seq))]).astype(np.uint64)
    qs, e = r[:, 1].copy(), r[:, 2].copy()
    pm, sm = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    deg = qs > e
    cd = (np.cumsum(deg) - deg).astype(np.uint32)
    d_off = np.zeros(n_seq + 1, np.uint64)
    dq_off = np.zeros(n_seq + 1, np.uint64)
    shift_nb = np.zeros((n_seq, 2), np.uint32)
    dq, de = [], []
    for c in range(n_seq):
        lo, hi = int(q_off[c]), int(q_off[c + 1])
        d_off[c + 1] = d_off[c]
        dq_off[c + 1] = dq_off[c]
        if hi == lo:
            continue
        pm[lo:hi] = np.maximum.accumulate(e[lo:hi])
        sm[lo:hi] = np.minimum.accumulate(e[lo:hi][::-1])[::-1]
        de.append(np.sort(e[lo:hi][deg[lo:hi]]))
        dq_off[c + 1] = dq_off[c] + len(de[-1])
        vmax = int(qs[hi - 1])
        budget = max(2 * (hi - lo), 16)
        shift = 0
        while (vmax >> shift) + 1 > budget:
            shift += 1
        nb = (vmax >> shift) + 1
        shift_nb[c] = (shift, nb)
        edges = np.arange(nb + 1, dtype=np.uint64) << np.uint64(shift)
        dq.append(lo + np.searchsorted(qs[lo:hi].astype(np.uint64), edges, "left"))
        dq[-1][-1] = hi  # the last entry is the seqid's end
        d_off[c + 1] = d_off[c] + nb + 1
    cat = lambda x: np.concatenate(x).astype(np.uint32) if x else np.zeros(0, np.uint32)  # noqa: E731
    return dict(q_off=q_off, qs=qs, pm=pm, sm=sm, cd=cd, d_off=d_off, shift_nb=shift_nb, dir_qs=cat(dq), dq_off=dq_off, de=cat(de))
