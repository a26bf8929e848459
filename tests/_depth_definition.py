"""What `gffx depth` computes per (block, ID) group, restated in numpy (`_numpy_depth`: the reference of tests/test_depth_gpu.py,
tests/test_depth_edges_gpu.py and tools/fuzz_lines.py), and a builder of hand-shaped line tables (`hand_table`) whose regions
overlap chosen lines of chosen blocks, wherever those lines sit in line order."""
import numpy as np


def _numpy_depth(roots, block_of_fid, block_off, ls, le, lg, n_groups, regions):
    depth = np.zeros(n_groups, np.uint64)
    mn = np.full(n_groups, 0xFFFFFFFF, np.uint32)
    mx = np.zeros(n_groups, np.uint32)
    co, S, E, F = roots["chr_offsets"], roots["start"].astype(np.int64), roots["end"].astype(np.int64), roots["fid"]
    for c, qs, qe in regions.astype(np.int64).tolist():
        lo, hi = int(co[c]), int(co[c + 1])
        hit = np.nonzero((S[lo:hi] < qe) & (E[lo:hi] > qs))[0] + lo
        for fid in np.unique(F[hit]).tolist():  # a region counts a root once (depth.rs:241)
            b = int(block_of_fid[fid])
            if b == 0xFFFFFFFF:
                continue
            a, z = int(block_off[b]), int(block_off[b + 1])
            ov = np.maximum(ls[a:z].astype(np.int64), qs) < np.minimum(le[a:z].astype(np.int64), qe)
            if not ov.any():
                continue
            g = lg[a:z][ov]
            depth[np.unique(g)] += 1
            np.minimum.at(mn, g, ls[a:z][ov])
            np.maximum.at(mx, g, le[a:z][ov])
    return depth, mn, mx


# ---------------------------------------------------------------------------------------------- hand-shaped tables
NO_BLOCK = 0xFFFFFFFF
BELOW, ABOVE = -2, -1  # window tags of lines that lie in no window: before the first window / behind the last one
ROOT_STRIDE = 100_000  # block b's root is [b * ROOT_STRIDE, b * ROOT_STRIDE + ROOT_WIDTH) on seqid 0
ROOT_WIDTH = 60_000
QUIET = (10, 20)       # inside every root, far from every line: a region here hits the root and no line
BELOW0 = 500           # BELOW lines: [root + 500, root + 1010)
WIN0, WIN_WIDTH, N_WIN = 2_000, 100, 256  # window w of a root: [root + WIN0 + w * WIN_WIDTH, + WIN_WIDTH); they touch
ABOVE0 = 40_000        # ABOVE lines: [root + 40 000, root + 40 510)
GAP = (70_000, 70_010)  # behind the root, before the next one: a region here has no pair at all


class HandTable:
    """The arrays DepthTable and TreeIndexData take (roots, block_of_fid, block_off, ls, le, lg, n_groups), plus where things are:
    `line0[b]` / `n_lines[b]` the block's lines, `group0[b]` its first group, `sizes[b]` its group sizes."""

    def window(self, b, w_lo, w_hi=None):
        """The region over windows w_lo .. w_hi of block b's root: it overlaps exactly the block's lines tagged w_lo .. w_hi."""
        w_hi = w_lo if w_hi is None else w_hi
        assert 0 <= w_lo <= w_hi < N_WIN
        r = b * ROOT_STRIDE + WIN0
        return (0, r + w_lo * WIN_WIDTH, r + (w_hi + 1) * WIN_WIDTH)

    def whole(self, b, b_last=None):
        """The region over the whole roots of blocks b .. b_last: every line of them."""
        return (0, b * ROOT_STRIDE, (b if b_last is None else b_last) * ROOT_STRIDE + ROOT_WIDTH)

    def quiet(self, b):
        return (0, b * ROOT_STRIDE + QUIET[0], b * ROOT_STRIDE + QUIET[1])

    def gap(self, b):
        return (0, b * ROOT_STRIDE + GAP[0], b * ROOT_STRIDE + GAP[1])

    def lines_hit(self, b, region):
        """Block-local numbers of the lines of block b that `region` overlaps (half-open, depth.rs:78-82): from the table alone."""
        a, z = self.line0[b], self.line0[b] + self.n_lines[b]
        s, e = self.ls[a:z].astype(np.int64), self.le[a:z].astype(np.int64)
        return np.nonzero(np.maximum(s, int(region[1])) < np.minimum(e, int(region[2])))[0].tolist()

    def roots_hit(self, region):
        """Indices (in index order) of the roots `region` overlaps."""
        S, E = self.roots["start"].astype(np.int64), self.roots["end"].astype(np.int64)
        return np.nonzero((S < int(region[2])) & (E > int(region[1])))[0].tolist()

    def items(self, region):
        """Line counts of the (region, block) items the kernel walks for `region`: one per distinct root_fid with a block of at
        least one line, the fids `known` to the device table only (n_fid)."""
        out = []
        for fid in np.unique(self.roots["fid"][self.roots_hit(region)]).tolist():
            b = int(self.block_of_fid[fid])
            if b != NO_BLOCK and self.n_lines[b] > 0:
                out.append(self.n_lines[b])
        return out

    def group_of_line(self, b, line):
        return self.group0[b] + int(np.searchsorted(np.cumsum(self.sizes[b]), line, "right"))

    def expect(self, hits):
        """(depth, min start, max end) of a batch given as [(block, [block-local lines its region overlaps]), ...] -- one entry
        per (region, block) -- by the rule itself: a group gains 1 per region with at least one overlapped line in it, and its
        extent is taken over the overlapped lines."""
        depth = np.zeros(self.n_groups, np.uint64)
        mn = np.full(self.n_groups, 0xFFFFFFFF, np.uint32)
        mx = np.zeros(self.n_groups, np.uint32)
        for b, lines in hits:
            for g in sorted({self.group_of_line(b, l) for l in lines}):
                depth[g] += 1
            for l in lines:
                g, at = self.group_of_line(b, l), self.line0[b] + l
                mn[g], mx[g] = min(mn[g], self.ls[at]), max(mx[g], self.le[at])
        return depth, mn, mx

    def definition(self, regions, block_of_fid=None):
        r = np.asarray(regions, np.uint32).reshape(-1, 3)
        return _numpy_depth(self.roots, self.block_of_fid if block_of_fid is None else block_of_fid, self.block_off, self.ls,
                            self.le, self.lg, self.n_groups, r)


def hand_table(blocks, tags=None, fids=None, extra_roots=(), n_fid=None):
    """blocks[b]: the group sizes of block b in line order; tags[b]: one window tag per line of the block (default: every line ABOVE).
    Block b lies in a root of its own, fid `fids[b]` (default 2 * b), so every odd fid has no block.  A line tagged w >= 0 lies
    inside window w of its root, a line tagged BELOW / ABOVE before / behind all windows; the k-th line of a block starts
    7 k mod 31 behind its window's start and ends 5 k mod 29 before its end, so lines differ in both and the block's first line
    (k = 0) touches both neighbouring windows.  extra_roots: further (start, end, fid) intervals of the index -- a second root of
    a fid, a root whose fid has no block."""
    T = HandTable()
    n_blocks = len(blocks)
    fids = [2 * b for b in range(n_blocks)] if fids is None else list(fids)
    assert len(set(fids)) == n_blocks
    ls, le, lg, block_off, g = [], [], [], [0], 0
    T.sizes, T.line0, T.n_lines, T.group0 = [], [], [], []
    for b, sizes in enumerate(blocks):
        n = sum(sizes)
        tg = [ABOVE] * n if tags is None or tags[b] is None else list(tags[b])
        assert len(tg) == n and all(s > 0 for s in sizes)
        T.sizes.append(list(sizes)), T.line0.append(len(ls)), T.n_lines.append(n), T.group0.append(g)
        root, k = b * ROOT_STRIDE, 0
        for size in sizes:
            for _ in range(size):
                if tg[k] >= 0:
                    assert tg[k] < N_WIN
                    ws = root + WIN0 + tg[k] * WIN_WIDTH
                    s, e = ws + 7 * k % 31, ws + WIN_WIDTH - 5 * k % 29
                else:
                    s = root + (BELOW0 if tg[k] == BELOW else ABOVE0) + (k % 50) * 10
                    e = s + 3 + k % 7
                ls.append(s), le.append(e), lg.append(g)
                k += 1
            g += 1
        block_off.append(len(ls))
    iv = [(b * ROOT_STRIDE, b * ROOT_STRIDE + ROOT_WIDTH, fids[b]) for b in range(n_blocks)] + [tuple(r) for r in extra_roots]
    iv.sort(key=lambda r: r[0])
    T.roots = {"chr_offsets": np.array([0, len(iv)], np.uint32), "start": np.array([r[0] for r in iv], np.uint32),
               "end": np.array([r[1] for r in iv], np.uint32), "fid": np.array([r[2] for r in iv], np.uint32)}
    n_fid = (max(r[2] for r in iv) + 2 if iv else 1) if n_fid is None else n_fid
    T.block_of_fid = np.full(n_fid, NO_BLOCK, np.uint32)
    for b in range(n_blocks):
        T.block_of_fid[fids[b]] = b
    T.fids = fids
    T.block_off = np.array(block_off, np.uint64)
    T.ls, T.le, T.lg = np.array(ls, np.uint32), np.array(le, np.uint32), np.array(lg, np.uint32)
    T.n_groups = g
    return T
