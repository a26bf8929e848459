"""Python mirror of the reference's interface for the `intersect` hot path, over the C-ABI.

Names and argument meaning follow the reference (Baohua-Chen/GFFx v0.4.0, src/):

* ``OverlapMode``                     commands/intersect.rs:73-78
* ``TreeIndexData``                   utils/tree_index.rs:12-16 (``chr_entries`` live in HBM)
* ``query_features(index_data, regions, mode, invert, verbose)``
                                      commands/intersect.rs:105-111
* ``QueryBatch``                      the streaming form of the same call (device-resident
                                      regions, reusable buffers, HIP-event kernel timing)

Everything here is plumbing around ``libgffx_hip.so``; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import enum
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import check, lib, u32p, u64p


class OverlapMode(enum.IntEnum):
    Contained = 0
    ContainsRegion = 1
    Overlap = 2


OUT_COUNTS, OUT_FIDS, OUT_TRIPLES, OUT_ROOT_BITMAP, OUT_OFFSETS, OUT_EMIT_ORDER = 1, 2, 4, 8, 16, 32
OUT_OFFSETS32, OUT_BITMAP_KEEP, OUT_SEGBASE, OUT_NO_COUNTS = 64, 128, 256, 512
SEG_GROUP = 256  # regions per OUT_SEGBASE entry
STRATEGY_AUTO, STRATEGY_DIRECT, STRATEGY_SORTED, STRATEGY_FUSED, STRATEGY_WINDOWS = 0, 1, 2, 3, 5  # (4: the retired slots strategy)
K_JOIN_COUNT, K_JOIN_EMIT, K_SORT, K_LINES, K_FUSED, K_UNPERMUTE, K_FUSED_DIRECT, K_DEPTH, K_SLOTS = 0, 1, 2, 3, 4, 5, 6, 7, 8
K_WINDOWS, K_BITMAP_OR, K_WAVE = 9, 10, 11
KERNEL_NAMES = {K_JOIN_COUNT: "k_join_count", K_JOIN_EMIT: "k_join_emit", K_SORT: "k_partition",
                K_LINES: "k_lines_exists", K_FUSED: "k_tile_join", K_UNPERMUTE: "k_unpermute",
                K_FUSED_DIRECT: "k_join_fused", K_DEPTH: "k_depth_regions",
                K_WINDOWS: "k_join_roots", K_BITMAP_OR: "k_bitmap_fold", K_WAVE: "k_join_pairs"}


def _options(fn, handle) -> dict:
    import json
    buf = C.create_string_buffer(1024)
    n = fn(handle, buf, len(buf))
    if n >= len(buf):
        buf = C.create_string_buffer(n + 1)
        fn(handle, buf, len(buf))
    return json.loads(buf.value.decode())


def device_count() -> int:
    return lib().gffx_hip_device_count()


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a: np.ndarray):
    return a.ctypes.data_as(u32p)


class TreeIndexData:
    """Per-seqid root intervals resident in HBM + the seqid name maps (tree_index.rs:12-16)."""

    def __init__(self, handle, num_to_seqid: Sequence[str]):
        self._h = handle
        self._batches = 0      # open QueryBatches: each holds the native index (its device, its count of busy batches)
        self._closing = False  # close() was asked for while batches were open: the last of them destroys the index
        self.num_to_seqid: List[str] = list(num_to_seqid)
        # FxHashMap built by collect(): a later duplicate name wins (index_loader/core.rs:28-32)
        self.seqid_to_num: Dict[str, int] = {n: i for i, n in enumerate(self.num_to_seqid)}

    @classmethod
    def from_roots(cls, chr_offsets, start, end, root_fid, names: Optional[Sequence[str]] = None,
                   device: int = 0) -> "TreeIndexData":
        co, s, e, f = _u32(chr_offsets), _u32(start), _u32(end), _u32(root_fid)
        if co.ndim != 1 or len(co) < 1:
            raise ValueError("chr_offsets must have n_chr+1 entries")
        h = C.c_void_p()
        check(lib().gffx_hip_index_create(len(co) - 1, _p(co), _p(s), _p(e), _p(f), device, C.byref(h)))
        if names is None:
            names = ["seq%d" % i for i in range(len(co) - 1)]
        return cls(h, names)

    def clone(self, device: int) -> "TreeIndexData":
        """The same index on another device of the node (gffx_hip_index_clone: device arrays copied GPU to GPU)."""
        h = C.c_void_p()
        check(lib().gffx_hip_index_clone(self._h, int(device), C.byref(h)))
        return TreeIndexData(h, self.num_to_seqid)

    def close(self) -> None:
        """Destroys the native index -- once no QueryBatch of it is open any more: gffx_hip_batch_destroy reads the index, and
        the collector finalises an index and its batches in no particular order when they die together in a reference cycle."""
        if getattr(self, "_h", None):
            if getattr(self, "_batches", 0) > 0:
                self._closing = True
                return
            lib().gffx_hip_index_destroy(self._h)
            self._h = None

    def _batch_closed(self) -> None:
        self._batches -= 1
        if self._closing and self._batches == 0:
            self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_chr(self) -> int:
        return lib().gffx_hip_index_n_chr(self._h)

    @property
    def n_roots(self) -> int:
        return lib().gffx_hip_index_n_roots(self._h)

    @property
    def device(self) -> int:
        return lib().gffx_hip_index_device(self._h)

    def options(self) -> dict:
        """The index builders' GFFX_HIP_* knobs that were not at their defaults when the index was created."""
        return _options(lib().gffx_hip_index_options, self._h)

    def sorted_fids(self) -> np.ndarray:
        n = self.n_roots
        if n == 0:  # (an index without roots has no array behind the pointer)
            return np.zeros(0, dtype=np.uint32)
        ptr = lib().gffx_hip_index_sorted_fids(self._h)
        return np.ctypeslib.as_array(ptr, shape=(n,)).copy()


class RegionStore:
    """gffx_hip_regions_*: BED rows resident in HBM, filled chunk by chunk through two pinned staging buffers.  keep_all=False:
    a ring of two slots of chunk_rows rows (an append from buffer k overwrites slot k); keep_all=True: every append goes
    behind the rows before it, up to max(capacity_rows, chunk_rows) rows.  The caller's protocol is the commands': fill
    ``staging(k)``, ``append(k, n)``, hand the rows to a batch / union / line table, and call ``wait_staging(k)`` (and
    ``QueryBatch.sync`` for a batch that ran on slot k) before writing buffer k again."""

    def __init__(self, capacity_rows: int, chunk_rows: int, keep_all: bool, device: int = 0):
        self.chunk_rows = int(chunk_rows)
        self.keep_all = bool(keep_all)
        self._h = C.c_void_p()
        check(lib().gffx_hip_regions_create(int(device), int(capacity_rows), self.chunk_rows, int(self.keep_all), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_regions_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def staging(self, k: int) -> np.ndarray:
        """Writable (chunk_rows, 3) u32 view of pinned staging buffer k; valid until close()."""
        ptr = lib().gffx_hip_regions_staging(self._h, int(k))
        if not ptr:
            raise ValueError("staging buffer %r: k must be 0 or 1" % (k,))
        return np.ctypeslib.as_array(C.cast(ptr, u32p), shape=(self.chunk_rows, 3))

    def wait_staging(self, k: int) -> None:
        check(lib().gffx_hip_regions_wait_staging(self._h, int(k)))

    def append(self, k: int, n_rows: int) -> None:
        """The first n_rows rows of staging buffer k go to the device (asynchronously)."""
        check(lib().gffx_hip_regions_append(self._h, int(k), int(n_rows)))

    def append_parts(self, k: int, stage_first, n_rows) -> None:
        """One chunk gathered from pieces of staging buffer k: rows [stage_first[p], stage_first[p] + n_rows[p]) in the
        order given, back to back on the device."""
        f = np.ascontiguousarray(stage_first, dtype=np.uint64)
        n = np.ascontiguousarray(n_rows, dtype=np.uint64)
        if f.ndim != 1 or f.shape != n.shape:
            raise ValueError("stage_first and n_rows must be 1-D and of the same length")
        check(lib().gffx_hip_regions_append_parts(self._h, int(k), len(f), f.ctypes.data_as(u64p), n.ctypes.data_as(u64p)))

    def rows(self) -> int:
        """Rows held (keep_all stores; a ring reports 0)."""
        return int(lib().gffx_hip_regions_rows(self._h))


class QueryBatch:
    """Reusable query batch on one HIP stream (create once, run many)."""

    def __init__(self, index: TreeIndexData, max_queries: int):
        self.index = index
        self._h = C.c_void_p()
        check(lib().gffx_hip_batch_create(index._h, int(max_queries), C.byref(self._h)))
        index._batches += 1
        self._keep = None  # keeps host/device inputs alive until wait()

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_batch_destroy(self._h)
            self._h = None
            self.index._batch_closed()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs
    def set_regions(self, regions) -> None:
        """regions: (nq,3) u32 rows (chr, start, end) == the reference's &[(u32,u32,u32)]."""
        r = _u32(regions).reshape(-1, 3)
        self._keep = r
        check(lib().gffx_hip_batch_set_regions_host(self._h, _p(r), r.shape[0]))

    def set_regions_soa(self, chr_, start, end) -> None:
        c, s, e = _u32(chr_), _u32(start), _u32(end)
        self._keep = (c, s, e)
        check(lib().gffx_hip_batch_set_regions_soa_host(self._h, _p(c), _p(s), _p(e), len(c)))

    def set_regions_device(self, d_chr: int, d_start: int, d_end: int, nq: int, keep=None) -> None:
        """Borrow three device arrays (raw pointers, e.g. torch.Tensor.data_ptr())."""
        self._keep = keep
        check(lib().gffx_hip_batch_set_regions_device(self._h, d_chr, d_start, d_end, int(nq)))

    def set_regions_store(self, store: "RegionStore", k: int, first: int, n_rows: int) -> None:
        """Rows [first, first + n_rows) of the store's last append from staging buffer k (no copy: the batch reads the store)."""
        self._keep = store
        check(lib().gffx_hip_batch_set_regions_store(self._h, store.handle, int(k), int(first), int(n_rows)))

    def set_option(self, name: str, value: int) -> None:
        """A tuning knob of this batch's passes (include/gffx_hip.h "Tuning knobs"), e.g. ("WIN_THREADS", 512)."""
        check(lib().gffx_hip_batch_set_option(self._h, name.encode(), int(value)))

    def options(self) -> dict:
        """The knobs of this batch that are not at their defaults (environment at creation + set_option)."""
        return _options(lib().gffx_hip_batch_options, self._h)

    @property
    def kept_pairs_accumulated(self) -> int:
        """Kept pairs of all root passes since the last one without OUT_BITMAP_KEEP (after wait)."""
        out = C.c_uint64(0)
        check(lib().gffx_hip_batch_kept_pairs_accumulated(self._h, C.byref(out)))
        return int(out.value)

    def reserve_hits(self, n_pairs: int) -> None:
        check(lib().gffx_hip_batch_reserve_hits(self._h, int(n_pairs)))

    # ---- run
    def run(self, mode: int = OverlapMode.Overlap, invert: bool = False, out_flags: int = OUT_FIDS,
            strategy: int = STRATEGY_AUTO) -> None:
        check(lib().gffx_hip_batch_run(self._h, int(mode), int(bool(invert)), int(out_flags), int(strategy)))

    def timed_runs(self, mode: int, invert: bool, out_flags: int, strategy: int, n: int) -> float:
        """n passes back to back between one pair of HIP events on the batch's stream; returns microseconds per pass."""
        ms = C.c_double(0.0)
        check(lib().gffx_hip_batch_timed_runs(self._h, int(mode), int(bool(invert)), int(out_flags), int(strategy), int(n), C.byref(ms)))
        return 1e3 * ms.value / n

    @property
    def block_threads(self) -> int:
        """threads per block of the last windows-strategy pair pass (512 or 1024; 0: none ran)"""
        return int(lib().gffx_hip_batch_block_threads(self._h))

    @property
    def block_count(self) -> int:
        """blocks of that launch (one 512-thread block per CU when two or more other batches of the index were in flight)"""
        return int(lib().gffx_hip_batch_block_count(self._h))

    @property
    def block_share(self) -> int:
        """the batch's own blocks of that launch (block_count is the whole grid of a launch that serves a group of batches)"""
        return int(lib().gffx_hip_batch_block_share(self._h))

    @property
    def filter_level(self) -> int:
        """coverage filter of the last windows-strategy launch: 0 none, 1 the coarse level, 2 the fine one"""
        return int(lib().gffx_hip_batch_filter_level(self._h))

    @property
    def wide_form(self) -> bool:
        """the last run's pair passes took the wide form of the window kernel (regions of any width, every mode)"""
        return bool(lib().gffx_hip_batch_wide_form(self._h))

    def wait(self) -> None:
        check(lib().gffx_hip_batch_wait(self._h))

    def sync(self) -> None:
        check(lib().gffx_hip_batch_sync(self._h))

    # ---- results
    @property
    def n_queries(self) -> int:
        return lib().gffx_hip_batch_n_queries(self._h)

    @property
    def total_hits(self) -> int:
        return lib().gffx_hip_batch_total_hits(self._h)

    @property
    def device_regions(self) -> int:
        """Device address of the batch's own AoS copy of the regions (0 unless set_regions uploaded them)."""
        return lib().gffx_hip_batch_device_regions(self._h) or 0

    def device_pointers(self):
        """(counts, fids, triples) device addresses of the last pass (0 where not produced): for consumers on the GPU."""
        L = lib()
        return (L.gffx_hip_batch_device_counts(self._h) or 0, L.gffx_hip_batch_device_fids(self._h) or 0,
                L.gffx_hip_batch_device_triples(self._h) or 0)

    def counts(self) -> np.ndarray:
        out = np.empty(max(self.n_queries, 1), dtype=np.uint32)
        check(lib().gffx_hip_batch_copy_counts(self._h, _p(out)))
        return out[: self.n_queries]

    def offsets(self) -> np.ndarray:
        out = np.empty(self.n_queries + 1, dtype=np.uint64)
        check(lib().gffx_hip_batch_copy_offsets(self._h, out.ctypes.data_as(u64p)))
        return out

    def offsets32(self) -> np.ndarray:
        """Segment starts as u32 (OUT_OFFSETS32), nq entries."""
        out = np.empty(max(self.n_queries, 1), dtype=np.uint32)
        check(lib().gffx_hip_batch_copy_offsets32(self._h, _p(out)))
        return out[: self.n_queries]

    def segbase(self) -> np.ndarray:
        """OUT_SEGBASE: start of the run of pairs of every group of SEG_GROUP consecutive regions (u64)."""
        n = (self.n_queries + SEG_GROUP - 1) // SEG_GROUP
        out = np.empty(max(n, 1), dtype=np.uint64)
        check(lib().gffx_hip_batch_copy_segbase(self._h, out.ctypes.data_as(u64p)))
        return out[:n]

    def offsets_from_segbase(self, counts: np.ndarray | None = None) -> np.ndarray:
        """Per-region segment starts derived the way a consumer of OUT_SEGBASE does: group base + counts before the region."""
        c = (self.counts() if counts is None else counts).astype(np.uint64)
        n = len(c)
        if n == 0:
            return np.zeros(0, dtype=np.uint64)
        ex = np.cumsum(c) - c
        g0 = np.arange(0, n, SEG_GROUP)
        within = ex - np.repeat(ex[g0], np.minimum(SEG_GROUP, n - g0))
        return np.repeat(self.segbase(), np.minimum(SEG_GROUP, n - g0)) + within

    def query_records(self, with_offsets: bool = True):
        """(rows, counts, offsets) in emission order: rows[i] = input row of the i-th served query."""
        n = self.n_queries
        rows = np.empty(max(n, 1), dtype=np.uint32)
        cnt = np.empty(max(n, 1), dtype=np.uint32)
        off = np.empty(max(n, 1), dtype=np.uint64) if with_offsets else None
        check(lib().gffx_hip_batch_copy_query_records(self._h, _p(rows), _p(cnt),
                                                      off.ctypes.data_as(u64p) if with_offsets else None))
        return rows[:n], cnt[:n], (off[:n] if with_offsets else None)

    def fids(self) -> np.ndarray:
        n = self.total_hits
        out = np.empty(max(n, 1), dtype=np.uint32)
        check(lib().gffx_hip_batch_copy_fids(self._h, _p(out)))
        return out[:n]

    def triples(self) -> np.ndarray:
        n = self.total_hits
        out = np.empty((max(n, 1), 3), dtype=np.uint32)
        check(lib().gffx_hip_batch_copy_triples(self._h, _p(out)))
        return out[:n]

    def root_bitmap(self) -> np.ndarray:
        """bool array over the index's roots in sorted order (see TreeIndexData.sorted_fids)."""
        n = self.index.n_roots
        words = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        check(lib().gffx_hip_batch_copy_root_bitmap(self._h, words.ctypes.data_as(u64p), len(words)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
        return bits.astype(bool)

    def unique_roots(self) -> np.ndarray:
        """Sorted unique root_fids with >=1 kept pair (commands/intersect.rs:598-615)."""
        return np.unique(self.index.sorted_fids()[self.root_bitmap()])

    # ---- profiling (HIP events on the batch's stream)
    def set_profiling(self, on: bool) -> None:
        check(lib().gffx_hip_batch_set_profiling(self._h, int(bool(on))))

    def reset_profile(self) -> None:
        check(lib().gffx_hip_batch_reset_profile(self._h))

    def kernel_ms(self, kernel_id: int) -> Tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        check(lib().gffx_hip_batch_kernel_ms(self._h, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class LineTable:
    """(seqid number, raw column-4 start, raw column-5 end) of GFF lines, resident in HBM.

    ``test(regions, n_seq, mode)`` is the numeric core of gff_line_overlaps_queries
    (commands/intersect.rs:500-521) for every line at once: one bool per line."""

    NO_SEQ = 0xFFFFFFFF

    def __init__(self, seq, start, end, device: int = 0):
        q, s, e = _u32(seq), _u32(start), _u32(end)
        if not (len(q) == len(s) == len(e)):
            raise ValueError("seq/start/end must have the same length")
        self.n = len(q)
        self._h = C.c_void_p()
        check(lib().gffx_hip_lines_create(device, self.n, _p(q), _p(s), _p(e), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_lines_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def test(self, regions, n_seq: int, mode: int = OverlapMode.Overlap) -> np.ndarray:
        r = _u32(regions).reshape(-1, 3)
        keep = np.zeros(max(self.n, 1), dtype=np.uint8)
        check(lib().gffx_hip_lines_test(self._h, _p(r), r.shape[0], int(n_seq), int(mode),
                                        keep.ctypes.data_as(_ffi.u8p)))
        return keep[: self.n].astype(bool)

    def test_device(self, d_regions: int, nq: int, n_seq: int, mode: int = OverlapMode.Overlap) -> np.ndarray:
        """The same with the regions already in HBM as AoS triples (``QueryBatch.device_regions``)."""
        keep = np.zeros(max(self.n, 1), dtype=np.uint8)
        check(lib().gffx_hip_lines_test_device(self._h, d_regions, int(nq), int(n_seq), int(mode),
                                               keep.ctypes.data_as(_ffi.u8p)))
        return keep[: self.n].astype(bool)

    def test_store(self, store: "RegionStore", n_seq: int, mode: int = OverlapMode.Overlap) -> np.ndarray:
        """The same with all rows of a keep_all ``RegionStore`` as the regions (what `gffx intersect` runs after Join A)."""
        keep = np.zeros(max(self.n, 1), dtype=np.uint8)
        check(lib().gffx_hip_lines_test_store(self._h, store.handle, int(n_seq), int(mode), keep.ctypes.data_as(_ffi.u8p)))
        return keep[: self.n].astype(bool)

    @property
    def last_kernel_ms(self) -> float:
        """HIP-event duration of k_lines_exists in the last ``test`` call."""
        return lib().gffx_hip_lines_last_kernel_ms(self._h)

    @property
    def last_sort_passes(self) -> int:
        """Radix passes of the last call's region sort (4 with the mixed-radix top digit, else 4 + seqid bytes; 0: no regions)."""
        return lib().gffx_hip_lines_last_sort_passes(self._h)

    @property
    def last_prep_ms(self) -> float:
        """HIP-event duration of the device preparation of the region tables (radix sorts, scans, directories)."""
        return lib().gffx_hip_lines_last_prep_ms(self._h)

    def tables(self, nq: int, n_seq: int):
        """Region tables of the last ``test``: dict(q_off, qs, pm, sm, cd, d_off, shift_nb, dir_qs) and, after an
        Overlap-mode test, dq_off / de (the regions with start > end: their ends sorted per seqid)."""
        u64p = _ffi.u64p
        q_off = np.zeros(n_seq + 1, dtype=np.uint64)
        tabs = [np.zeros(max(nq, 1), dtype=np.uint32) for _ in range(4)]
        check(lib().gffx_hip_lines_copy_tables(self._h, q_off.ctypes.data_as(u64p), *[_p(t) for t in tabs]))
        d_off = np.zeros(n_seq + 1, dtype=np.uint64)
        shift_nb = np.zeros((max(n_seq, 1), 2), dtype=np.uint32)
        check(lib().gffx_hip_lines_copy_dirs(self._h, d_off.ctypes.data_as(u64p), _p(shift_nb), None))
        total = int(d_off[-1])
        dq = np.zeros(max(total, 1), dtype=np.uint32)
        check(lib().gffx_hip_lines_copy_dirs(self._h, None, None, _p(dq)))
        out = dict(q_off=q_off, qs=tabs[0][:nq], pm=tabs[1][:nq], sm=tabs[2][:nq], cd=tabs[3][:nq], d_off=d_off,
                   shift_nb=shift_nb[:n_seq], dir_qs=dq[:total])
        n_deg = C.c_uint64(0)
        if lib().gffx_hip_lines_copy_degenerate(self._h, C.byref(n_deg), None, None) == 0:
            dq_off = np.zeros(n_seq + 1, dtype=np.uint64)
            de = np.zeros(max(n_deg.value, 1), dtype=np.uint32)
            check(lib().gffx_hip_lines_copy_degenerate(self._h, None, dq_off.ctypes.data_as(u64p), _p(de)))
            out.update(dq_off=dq_off, de=de[: n_deg.value])
        return out


class DepthTable:
    """Feature lines of the root blocks, resident in HBM, plus the per-group accumulators of `gffx depth`
    (commands/depth.rs:121-293).  ``accumulate(batch)`` adds the regions of a finished Overlap pass."""

    def __init__(self, n_groups: int, block_line_off, line_start, line_end, line_group, block_of_fid, device: int = 0):
        bo = np.ascontiguousarray(block_line_off, dtype=np.uint64)
        ls, le, lg, bf = _u32(line_start), _u32(line_end), _u32(line_group), _u32(block_of_fid)
        self.n_groups = int(n_groups)
        self._h = C.c_void_p()
        check(lib().gffx_hip_depth_create(device, self.n_groups, len(bo) - 1, bo.ctypes.data_as(u64p), _p(ls), _p(le),
                                          _p(lg), len(bf), _p(bf), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_depth_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate(self, batch: "QueryBatch") -> None:
        check(lib().gffx_hip_depth_accumulate(self._h, batch._h))

    def reset(self) -> None:
        check(lib().gffx_hip_depth_reset(self._h))

    def results(self):
        n = max(self.n_groups, 1)
        d = np.zeros(n, dtype=np.uint64)
        s = np.zeros(n, dtype=np.uint32)
        e = np.zeros(n, dtype=np.uint32)
        check(lib().gffx_hip_depth_copy(self._h, d.ctypes.data_as(u64p), _p(s), _p(e)))
        return d[: self.n_groups], s[: self.n_groups], e[: self.n_groups]


def segments_covered(seg_seq, seg_start, seg_end, regions, n_seq: int, device: int = 0) -> np.ndarray:
    """Covered bases of every segment under the union of the regions of its seqid (commands/coverage.rs:92-124,
    :339-364); regions = (n,3) u32 rows (chr, start, end) with start < end."""
    q, s, e = _u32(seg_seq), _u32(seg_start), _u32(seg_end)
    r = _u32(regions).reshape(-1, 3)
    out = np.zeros(max(len(q), 1), dtype=np.uint32)
    check(lib().gffx_hip_segments_covered(device, len(q), _p(q), _p(s), _p(e), _p(r), r.shape[0], int(n_seq), _p(out)))
    return out[: len(q)]


class RegionUnion:
    """merge_intervals (commands/coverage.rs:92-109) over all rows added, per seqid, built on the device: sorted, disjoint,
    non-touching spans.  Any grouping of the rows into ``add`` calls gives the same spans."""

    def __init__(self, n_seq: int, device: int = 0):
        self.n_seq = int(n_seq)
        self._h = C.c_void_p()
        check(lib().gffx_hip_union_create(device, self.n_seq, C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_union_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, rows) -> None:
        r = _u32(rows).reshape(-1, 3)
        check(lib().gffx_hip_union_add_host(self._h, _p(r), r.shape[0]))

    def add_store(self, store, k: int, first: int, n_rows: int) -> None:
        """Rows [first, first + n_rows) of the last append from staging buffer k of ``store`` (a RegionStore or a raw handle)."""
        handle = store.handle if isinstance(store, RegionStore) else store
        check(lib().gffx_hip_union_add_store(self._h, handle, int(k), int(first), int(n_rows)))

    def add_spans(self, u_off, us, ue) -> None:
        o = np.ascontiguousarray(u_off, dtype=np.uint64)
        a, b = _u32(us), _u32(ue)
        check(lib().gffx_hip_union_add_spans(self._h, o.ctypes.data_as(u64p), _p(a), _p(b)))

    def finish(self) -> None:
        check(lib().gffx_hip_union_finish(self._h))

    @property
    def n_spans(self) -> int:
        return int(lib().gffx_hip_union_n_spans(self._h))

    def spans(self):
        """(u_off, us, ue, pb) after ``finish``."""
        n = self.n_spans
        o = np.zeros(self.n_seq + 1, dtype=np.uint64)
        a, b = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        p = np.zeros(max(n, 1), dtype=np.uint64)
        check(lib().gffx_hip_union_copy_spans(self._h, o.ctypes.data_as(u64p), _p(a), _p(b), p.ctypes.data_as(u64p)))
        return o, a[:n], b[:n], p[:n]

    def segments_covered(self, seg_seq, seg_start, seg_end) -> np.ndarray:
        q, s, e = _u32(seg_seq), _u32(seg_start), _u32(seg_end)
        out = np.zeros(max(len(q), 1), dtype=np.uint32)
        check(lib().gffx_hip_union_segments_covered(self._h, len(q), _p(q), _p(s), _p(e), _p(out)))
        return out[: len(q)]

    def stats(self) -> Dict[str, float]:
        ms, rows, folds = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().gffx_hip_union_stats(self._h, C.byref(ms), C.byref(rows), C.byref(folds)))
        return {"kernel_ms": ms.value, "rows": rows.value, "folds": folds.value}


def _pileup_constants() -> Tuple[int, int]:
    """(rows per fold, records per block of the prefix-sum kernels) of the library as it was built."""
    return int(lib().gffx_hip_pileup_fold_rows()), int(lib().gffx_hip_pileup_scan_tile())


def _profile_constants() -> Tuple[int, int]:
    """(new rows per fold, records per block of the scan kernels) of the depth profile as the library was built."""
    return int(lib().gffx_hip_profile_fold_rows()), int(lib().gffx_hip_profile_scan_tile())


def __getattr__(name: str):
    # PILEUP_FOLD / PILEUP_SCAN_TILE, PROFILE_FOLD / PROFILE_SCAN_TILE: asked of the library on first use, so that importing
    # this module loads nothing
    if name in ("PILEUP_FOLD", "PILEUP_SCAN_TILE"):
        fold, tile = _pileup_constants()
        globals().update(PILEUP_FOLD=fold, PILEUP_SCAN_TILE=tile)
        return fold if name == "PILEUP_FOLD" else tile
    if name in ("PROFILE_FOLD", "PROFILE_SCAN_TILE"):
        fold, tile = _profile_constants()
        globals().update(PROFILE_FOLD=fold, PROFILE_SCAN_TILE=tile)
        return fold if name == "PROFILE_FOLD" else tile
    if name == "SEQ_TILE":
        globals().update(SEQ_TILE=seq_tile())
        return globals()["SEQ_TILE"]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


class Pileup:
    """gffx_hip_pileup_*: the bases the rows added so far lay on every segment (`gffx coverage --mean-depth`),
    bases[i] = sum over the rows (seqid, s, e) of seqid seg_seq[i] of max(0, min(e, seg_end[i]) - max(s, seg_start[i])).
    A sum over rows: any grouping of the rows into ``add`` calls, or over several objects whose totals are added, gives the
    same numbers."""

    def __init__(self, n_seq: int, seg_seq, seg_start, seg_end, device: int = 0):
        self.n_seq = int(n_seq)
        q, s, e = _u32(seg_seq).ravel(), _u32(seg_start).ravel(), _u32(seg_end).ravel()
        if not (len(q) == len(s) == len(e)):
            raise ValueError("seg_seq, seg_start and seg_end must have the same length")
        self.n_seg = len(q)
        self.n_feat, self.meta_columns, self.meta_matrix = 0, 0, False  # (set by meta_set)
        self._h = C.c_void_p()
        check(lib().gffx_hip_pileup_create(int(device), self.n_seq, self.n_seg, _p(q), _p(s), _p(e), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_pileup_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, rows) -> None:
        r = _u32(rows).reshape(-1, 3)
        check(lib().gffx_hip_pileup_add_host(self._h, _p(r), r.shape[0]))

    def add_store(self, store, k: int, first: int, n_rows: int) -> None:
        """Rows [first, first + n_rows) of the last append from staging buffer k of ``store`` (a RegionStore or a raw handle)."""
        handle = store.handle if isinstance(store, RegionStore) else store
        check(lib().gffx_hip_pileup_add_store(self._h, handle, int(k), int(first), int(n_rows)))

    def bases(self) -> np.ndarray:
        """The running totals, one u64 per segment (waits for the folds in flight)."""
        out = np.zeros(max(self.n_seg, 1), dtype=np.uint64)
        check(lib().gffx_hip_pileup_copy(self._h, out.ctypes.data_as(u64p)))
        return out[: self.n_seg]

    def reset(self) -> None:
        check(lib().gffx_hip_pileup_reset(self._h))

    def stats(self) -> Dict[str, float]:
        ms, rows, folds = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().gffx_hip_pileup_stats(self._h, C.byref(ms), C.byref(rows), C.byref(folds)))
        st = [C.c_double(0) for _ in range(4)]
        check(lib().gffx_hip_pileup_stage_ms(self._h, *[C.byref(x) for x in st]))
        return {"kernel_ms": ms.value, "rows": rows.value, "folds": folds.value, "keys_ms": st[0].value, "sorts_ms": st[1].value,
                "scan_ms": st[2].value, "segments_ms": st[3].value}

    # ---- the second consumer: the stranded depth profile around features (`gffx meta`, gffx_hip_pileup_meta_*) ----

    def meta_set(self, feat_seq, feat_start, feat_end, feat_minus, layout: "MetaLayout", seq_len=None, keep_matrix: bool = False) -> int:
        """The features and the layout (they replace earlier ones and zero the meta totals); returns the number of columns."""
        q, s, e = _u32(feat_seq).ravel(), _u32(feat_start).ravel(), _u32(feat_end).ravel()
        m = np.ascontiguousarray(feat_minus, dtype=np.uint8).ravel()
        if not (len(q) == len(s) == len(e) == len(m)):
            raise ValueError("feat_seq, feat_start, feat_end and feat_minus must have the same length")
        ln = None
        if seq_len is not None:
            ln = _u32(seq_len).ravel()
            if len(ln) != self.n_seq:
                raise ValueError("seq_len must have one length per seqid")
        check(lib().gffx_hip_pileup_meta_set(self._h, len(q), _p(q), _p(s), _p(e), m.ctypes.data_as(_ffi.u8p), _p(ln) if ln is not None else None,
                                             C.byref(layout), int(bool(keep_matrix))))
        self.n_feat, self.meta_columns, self.meta_matrix = len(q), layout.columns, bool(keep_matrix)
        return self.meta_columns

    def meta(self, matrix: bool = False):
        """(col_bases, col_len, col_features), each u64[B]; with ``matrix`` also the n_feat x B matrix (waits for the folds)."""
        B = self.meta_columns
        cols = [np.zeros(max(B, 1), dtype=np.uint64) for _ in range(3)]
        mat = np.zeros(max(self.n_feat * B, 1), dtype=np.uint64) if matrix else None
        check(lib().gffx_hip_pileup_meta_copy(self._h, *[c.ctypes.data_as(u64p) for c in cols], mat.ctypes.data_as(u64p) if matrix else None))
        out = tuple(c[:B] for c in cols)
        return out + (mat[: self.n_feat * B].reshape(self.n_feat, B),) if matrix else out

    def meta_ms(self) -> float:
        ms = C.c_double(0)
        check(lib().gffx_hip_pileup_meta_ms(self._h, C.byref(ms)))
        return ms.value


META_POINT, META_SCALED = 0, 1
META_TSS, META_TES, META_CENTER = 0, 1, 2


class MetaLayout(C.Structure):
    """gffx_hip_meta_layout: point mode around an anchor, or scaled mode with ``body_bins`` columns over the feature."""
    _fields_ = [("mode", C.c_uint32), ("anchor", C.c_uint32), ("up", C.c_uint32), ("down", C.c_uint32), ("bin", C.c_uint32), ("body_bins", C.c_uint32)]

    @classmethod
    def point(cls, up: int, down: int, bin: int, anchor: int = META_TSS) -> "MetaLayout":
        return cls(META_POINT, anchor, up, down, bin, 0)

    @classmethod
    def scaled(cls, up: int, down: int, bin: int, body_bins: int) -> "MetaLayout":
        return cls(META_SCALED, 0, up, down, bin, body_bins)

    @property
    def columns(self) -> int:
        """B, 0 for a layout that is none (it may exceed meta_max_columns())."""
        return int(lib().gffx_hip_pileup_meta_columns(C.byref(self)))


def meta_constants() -> Tuple[int, int]:
    """(the column limit, the features per block of k_pileup_meta) of the library as it was built."""
    return int(lib().gffx_hip_pileup_meta_max_columns()), int(lib().gffx_hip_pileup_meta_tile())


CLOSEST_IGNORE_OVERLAPS, CLOSEST_LEFT_ONLY, CLOSEST_RIGHT_ONLY = 1, 2, 4  # enum gffx_closest_flags
_CLOSEST_SIDES = {"both": 0, "left": CLOSEST_LEFT_ONLY, "right": CLOSEST_RIGHT_ONLY}


def closest_flags(ignore_overlaps: bool = False, side: str = "both") -> int:
    if side not in _CLOSEST_SIDES:
        raise ValueError("side must be 'both', 'left' or 'right', not %r" % (side,))
    return (CLOSEST_IGNORE_OVERLAPS if ignore_overlaps else 0) | _CLOSEST_SIDES[side]


def closest_distances(regions, counts, triples, gaps) -> np.ndarray:
    """Signed distance of every answered root as int64, in pair order: -gap for a root left of its region (end <= region
    start), +gap for one to the right (start >= region end), 0 for an overlap.  It follows from the triple and the region."""
    r = _u32(regions).reshape(-1, 3).astype(np.int64)
    t = np.asarray(triples).reshape(-1, 3).astype(np.int64)
    c = np.asarray(counts).astype(np.int64)
    qs, qe, g = np.repeat(r[:, 1], c), np.repeat(r[:, 2], c), np.repeat(np.asarray(gaps).astype(np.int64), c)
    over = (t[:, 1] < qe) & (t[:, 2] > qs)
    return np.where(over, 0, np.where(t[:, 2] <= qs, -g, g)).astype(np.int64)


class Closest:
    """gffx_hip_closest_*: the roots nearest to every region, and how far away (`gffx closest`).  One handle per index, on the
    index's device; it builds the end table (the roots' ends sorted by (seqid, end)) on the device when it is created."""

    def __init__(self, index: TreeIndexData, max_queries: int = 1 << 20):
        self.index = index
        self._h = C.c_void_p()
        check(lib().gffx_hip_closest_create(index._h, int(max_queries), C.byref(self._h)))
        index._batches += 1  # (the handle reads the native index, like a batch)
        self.max_queries = int(max_queries)
        self._nq = 0
        self._keep = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_closest_destroy(self._h)
            self._h = None
            self.index._batch_closed()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _results(self, nq: int):
        check(lib().gffx_hip_closest_wait(self._h))
        self._keep = None
        total = C.c_uint64()
        check(lib().gffx_hip_closest_total_pairs(self._h, C.byref(total)))
        counts, gaps = np.empty(nq, dtype=np.uint32), np.empty(nq, dtype=np.uint32)
        offsets = np.empty(nq + 1, dtype=np.uint64)
        triples = np.empty((total.value, 3), dtype=np.uint32)
        check(lib().gffx_hip_closest_copy_counts(self._h, _p(counts)))
        check(lib().gffx_hip_closest_copy_offsets(self._h, offsets.ctypes.data_as(u64p)))
        check(lib().gffx_hip_closest_copy_triples(self._h, _p(triples)))
        check(lib().gffx_hip_closest_copy_gaps(self._h, _p(gaps)))
        return counts, offsets, triples, gaps

    def run(self, regions, ignore_overlaps: bool = False, side: str = "both", flags: Optional[int] = None):
        """regions: (nq, 3) u32 rows (chr, start, end).  Returns counts[nq], offsets[nq + 1] (u64, the exclusive prefix in input
        order), triples[pairs, 3] (root_fid, start, end; ascending index position inside a region) and gaps[nq] (undefined
        where the count is 0).  `flags`, when given, is passed as it is (enum gffx_closest_flags)."""
        r = _u32(regions).reshape(-1, 3)
        f = closest_flags(ignore_overlaps, side) if flags is None else int(flags)
        check(lib().gffx_hip_closest_run_host(self._h, _p(r), r.shape[0], f))
        return self._results(r.shape[0])

    def run_store(self, store: "RegionStore", k: int, first: int, n_rows: int, ignore_overlaps: bool = False, side: str = "both"):
        """The same over rows [first, first + n_rows) of the store's last append from staging buffer k, read in place."""
        self._keep = store
        check(lib().gffx_hip_closest_run_store(self._h, store.handle, int(k), int(first), int(n_rows), closest_flags(ignore_overlaps, side)))
        return self._results(int(n_rows))

    def end_table(self):
        """(e_end, e_pos): the ends of the roots sorted stably by (seqid, end), and the index position each came from."""
        n = self.index.n_roots
        e_end, e_pos = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        check(lib().gffx_hip_closest_copy_end_table(self._h, _p(e_end), _p(e_pos)))
        return e_end, e_pos

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        check(lib().gffx_hip_closest_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_grid(self) -> Tuple[int, int]:
        """(blocks, regions per block) of the last run's launches."""
        blocks, chunk = C.c_uint32(), C.c_uint64()
        check(lib().gffx_hip_closest_last_grid(self._h, C.byref(blocks), C.byref(chunk)))
        return blocks.value, chunk.value

    def stats(self) -> Dict[str, float]:
        ms, grows = C.c_double(), C.c_uint64()
        check(lib().gffx_hip_closest_stats(self._h, C.byref(ms), C.byref(grows)))
        return {"build_ms": ms.value, "grows": grows.value}


class DepthProfile:
    """gffx_hip_profile_*: the per-base depth of the rows added so far as canonical points per seqid (`gffx coverage
    --thresholds / --bedgraph`): (pos_i, d_i) with d_i the depth on [pos_i, pos_{i+1}), d_i != d_{i-1}, the last depth 0.
    A function of the multiset of rows: any grouping into ``add`` calls, any order and profiles merged with ``add_points``
    give the same points bit for bit."""

    def __init__(self, n_seq: int, device: int = 0):
        self.n_seq = int(n_seq)
        self._h = C.c_void_p()
        check(lib().gffx_hip_profile_create(int(device), self.n_seq, C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_profile_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, rows) -> None:
        r = _u32(rows).reshape(-1, 3)
        check(lib().gffx_hip_profile_add_host(self._h, _p(r), r.shape[0]))

    def add_store(self, store, k: int, first: int, n_rows: int) -> None:
        """Rows [first, first + n_rows) of the last append from staging buffer k of ``store`` (a RegionStore or a raw handle)."""
        handle = store.handle if isinstance(store, RegionStore) else store
        check(lib().gffx_hip_profile_add_store(self._h, handle, int(k), int(first), int(n_rows)))

    def add_points(self, p_off, pos, depth) -> None:
        """Another profile's ``points()``: the merge over devices.  Points that are not canonical are refused."""
        o = np.ascontiguousarray(p_off, dtype=np.uint64)
        a, b = _u32(pos), _u32(depth)
        if len(o) != self.n_seq + 1 or len(a) != len(b) or (len(o) and int(o[-1]) != len(a)):
            raise ValueError("p_off must have n_seq + 1 entries and end at the number of points")
        check(lib().gffx_hip_profile_add_points(self._h, o.ctypes.data_as(u64p), _p(a), _p(b)))

    def finish(self) -> None:
        check(lib().gffx_hip_profile_finish(self._h))

    @property
    def n_points(self) -> int:
        return int(lib().gffx_hip_profile_n_points(self._h))

    def points(self):
        """(p_off, pos, depth) after ``finish``."""
        o = np.zeros(self.n_seq + 1, dtype=np.uint64)
        check(lib().gffx_hip_profile_copy_points(self._h, o.ctypes.data_as(u64p), None, None))  # (GFFX_E_STATE before finish)
        n = int(o[-1])
        a, b = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().gffx_hip_profile_copy_points(self._h, None, _p(a), _p(b)))
        return o, a[:n], b[:n]

    def union_at_least(self, T: int) -> "RegionUnion":
        """The spans "depth >= T" as a finished RegionUnion on the profile's device (written there, never copied out)."""
        h = C.c_void_p()
        check(lib().gffx_hip_profile_union_at_least(self._h, int(T), C.byref(h)))
        u = RegionUnion.__new__(RegionUnion)
        u.n_seq, u._h = self.n_seq, h
        return u

    def reset(self) -> None:
        check(lib().gffx_hip_profile_reset(self._h))

    def stats(self) -> Dict[str, float]:
        ms, rows, folds = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().gffx_hip_profile_stats(self._h, C.byref(ms), C.byref(rows), C.byref(folds)))
        st = [C.c_double(0) for _ in range(4)]
        check(lib().gffx_hip_profile_stage_ms(self._h, *[C.byref(x) for x in st]))
        return {"kernel_ms": ms.value, "rows": rows.value, "folds": folds.value, "events_ms": st[0].value, "sort_ms": st[1].value,
                "scan_ms": st[2].value, "points_ms": st[3].value}


def _classmap_constants() -> Tuple[int, int, int]:
    """(events per scan tile, regions per block of the regions kernel, tiles per step of the single-block carry walks) of the
    class map."""
    return int(lib().gffx_hip_classmap_scan_tile()), int(lib().gffx_hip_classmap_block_size()), int(lib().gffx_hip_classmap_carry_tiles())


class ClassMap:
    """gffx_hip_classmap_*: per region the bases of every feature class (`gffx annotate`).  ``n_layers`` layers of intervals in
    priority order; the class of a base is the first layer that covers it, or ``n_layers`` for none.  The class map is a
    function of the multiset of rows: any grouping into ``add_rows`` calls, any order and duplicates give the same points."""

    def __init__(self, n_seq: int, n_layers: int, device: int = 0):
        self.n_seq, self.n_layers = int(n_seq), int(n_layers)
        self._h = C.c_void_p()
        self._keep = None
        check(lib().gffx_hip_classmap_create(int(device), self.n_seq, self.n_layers, C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_classmap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_rows(self, rows) -> None:
        """rows: (n, 4) u32 (layer, seqid, start, end)."""
        r = _u32(rows).reshape(-1, 4)
        check(lib().gffx_hip_classmap_add_rows_host(self._h, _p(r), r.shape[0]))

    def finish(self) -> None:
        check(lib().gffx_hip_classmap_finish(self._h))

    @property
    def n_points(self) -> int:
        return int(lib().gffx_hip_classmap_n_points(self._h))

    def points(self):
        """(p_off, pos, cls) after ``finish``."""
        o = np.zeros(self.n_seq + 1, dtype=np.uint64)
        check(lib().gffx_hip_classmap_copy_points(self._h, o.ctypes.data_as(u64p), None, None))  # (GFFX_E_STATE before finish)
        n = int(o[-1])
        a, b = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint8)
        check(lib().gffx_hip_classmap_copy_points(self._h, None, _p(a), b.ctypes.data_as(C.POINTER(C.c_uint8))))
        return o, a[:n], b[:n]

    def bases(self) -> np.ndarray:
        """cb[k, i]: the bases of class k on all points before point i, (n_layers, n_points) u64."""
        n = self.n_points
        cb = np.zeros((self.n_layers, max(n, 1)), dtype=np.uint64)
        check(lib().gffx_hip_classmap_copy_bases(self._h, cb.ctypes.data_as(u64p)) if n else lib().gffx_hip_classmap_copy_bases(self._h, None))
        return cb[:, :n]

    def _results(self, nq: int):
        check(lib().gffx_hip_classmap_wait(self._h))
        self._keep = None
        counts = np.zeros((max(nq, 1), self.n_layers + 1), dtype=np.uint32)
        cls = np.zeros(max(nq, 1), dtype=np.uint8)
        check(lib().gffx_hip_classmap_copy_counts(self._h, _p(counts)))
        check(lib().gffx_hip_classmap_copy_class(self._h, cls.ctypes.data_as(C.POINTER(C.c_uint8))))
        return counts[:nq], cls[:nq]

    def run(self, regions):
        """regions: (nq, 3) u32 rows (chr, start, end).  Returns counts[nq, n_layers + 1] and the class byte per region
        (n_layers for none)."""
        r = _u32(regions).reshape(-1, 3)
        check(lib().gffx_hip_classmap_run_host(self._h, _p(r), r.shape[0]))
        return self._results(r.shape[0])

    def run_store(self, store: "RegionStore", k: int, first: int, n_rows: int):
        """The same over rows [first, first + n_rows) of the store's last append from staging buffer k, read in place."""
        self._keep = store
        check(lib().gffx_hip_classmap_run_store(self._h, store.handle, int(k), int(first), int(n_rows)))
        return self._results(int(n_rows))

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        check(lib().gffx_hip_classmap_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def stage_ms(self) -> Dict[str, float]:
        ms = (C.c_double * 6)()
        check(lib().gffx_hip_classmap_stage_ms(self._h, ms))
        return dict(zip(("union_ms", "toggles_ms", "sort_ms", "scan_ms", "points_ms", "bases_ms"), [float(x) for x in ms]))

    # ---- permutation totals (`gffx enrich`) ----
    def perm_begin(self, seq_len, n_perm: int, seed: int = 0) -> None:
        """Start (or start over) the totals of ``n_perm`` permutations: ``seq_len[c]`` is the length of seqid c."""
        L = _u32(seq_len).reshape(-1)
        if len(L) != self.n_seq:
            raise ValueError("seq_len must have n_seq entries")
        check(lib().gffx_hip_classmap_perm_begin(self._h, _p(L), int(n_perm), int(seed) & 0xFFFFFFFFFFFFFFFF))
        self._n_perm = int(n_perm)  # (a refused call leaves the earlier totals and their shape)

    def perm_run(self, regions, first_row: int = 0) -> None:
        """Add regions ((nq, 3) u32 rows; region j is global row ``first_row + j``) to the totals.  Asynchronous."""
        r = _u32(regions).reshape(-1, 3)
        check(lib().gffx_hip_classmap_perm_run_host(self._h, _p(r), r.shape[0], int(first_row)))

    def perm_run_store(self, store: "RegionStore", k: int, first: int, n_rows: int, first_row: int = 0) -> None:
        """The same over rows [first, first + n_rows) of the store's last append from staging buffer k, read in place."""
        self._keep = store
        check(lib().gffx_hip_classmap_perm_run_store(self._h, store.handle, int(k), int(first), int(n_rows), int(first_row)))

    def perm_totals(self):
        """Waits for the runs.  -> (bases, regions) as (n_perm + 1, n_layers + 1) u64 -- row 0 the observed data -- and
        the number of unplaceable regions."""
        check(lib().gffx_hip_classmap_perm_wait(self._h))
        self._keep = None
        shape = (getattr(self, "_n_perm", 0) + 1, self.n_layers + 1)
        b, r, u = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), np.zeros(1, np.uint64)
        check(lib().gffx_hip_classmap_perm_copy_totals(self._h, b.ctypes.data_as(u64p), r.ctypes.data_as(u64p), u.ctypes.data_as(u64p)))
        return b, r, int(u[0])

    def perm_last_kernel_ms(self) -> float:
        ms = C.c_double()
        check(lib().gffx_hip_classmap_perm_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


def _enrich_constants() -> Tuple[int, int]:
    """(rows of the totals per block, regions per block) of k_classmap_permute."""
    return int(lib().gffx_hip_classmap_perm_group()), int(lib().gffx_hip_classmap_block_size())


def run_batches(batches: Sequence["QueryBatch"], mode: int = OverlapMode.Overlap, invert: bool = False, out_flags: int = OUT_FIDS,
                strategy: int = STRATEGY_AUTO, n_passes: Optional[int] = None) -> None:
    """gffx_hip_batches_run_n: pass i over batches[i % len(batches)], enqueued by ONE call.  Distinct batches of one index that
    resolve to the same pass of the windows strategy are served by ONE launch per group of up to 8 (knob GFFX_HIP_GROUP of
    batches[0]); results are those of single `run` calls."""
    arr = (C.c_void_p * len(batches))(*[b._h for b in batches])
    check(lib().gffx_hip_batches_run_n(arr, len(batches), int(mode), int(bool(invert)), int(out_flags), int(strategy),
                                       int(len(batches) if n_passes is None else n_passes)))


def batches_plan(batches: Sequence["QueryBatch"]):
    """(groups per walk over the batches -- 0: pass by pass --, largest group, streams) of run_batches for these batches"""
    arr = (C.c_void_p * len(batches))(*[b._h for b in batches])
    g, m, st = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(lib().gffx_hip_batches_plan(arr, len(batches), C.byref(g), C.byref(m), C.byref(st)))
    return int(g.value), int(m.value), int(st.value)


def timed_group_runs(batches: Sequence["QueryBatch"], mode: int, invert: bool, out_flags: int, strategy: int, n: int):
    """n launches, each one pass over every batch (a group of <= 8), back to back between one pair of HIP events.
    Returns (microseconds per launch, grouped: the passes ran as one launch)."""
    arr = (C.c_void_p * len(batches))(*[b._h for b in batches])
    ms, grouped = C.c_double(0.0), C.c_uint32(0)
    check(lib().gffx_hip_batches_timed_runs(arr, len(batches), int(mode), int(bool(invert)), int(out_flags), int(strategy), int(n),
                                            C.byref(ms), C.byref(grouped)))
    return 1e3 * ms.value / n, bool(grouped.value)


def warmup(device: int = 0) -> None:
    """Pay the process's one-off HIP costs now (gffx_hip_warmup); optional."""
    check(lib().gffx_hip_warmup(int(device)))


def query_features(index_data: TreeIndexData, regions, mode: int = OverlapMode.Overlap,
                   invert: bool = False, verbose: bool = False) -> np.ndarray:
    """commands/intersect.rs:105-169: (root_fid, iv.start, iv.end) per kept (region, root) pair.

    Returns an (n,3) u32 array.  Pair order: regions in input order, unspecified inside a region
    (the reference's order is an FxHashMap walk plus a tree DFS, i.e. unspecified as well).  Raises GffxHipError
    (GFFX_E_CHR_RANGE) where the reference panics on an out-of-range chr.
    """
    r = _u32(regions).reshape(-1, 3)
    if verbose:
        import sys
        print("[DEBUG] Querying %d regions on device %d" % (r.shape[0], index_data.device), file=sys.stderr)
    tp = u32p()
    n = C.c_uint64()
    check(lib().gffx_hip_query_features(index_data._h, _p(r), r.shape[0], int(mode), int(bool(invert)),
                                        C.byref(tp), C.byref(n)))
    out = np.ctypeslib.as_array(tp, shape=(max(n.value, 1), 3))[: n.value].copy()
    lib().gffx_hip_free_host(tp)
    return out


# ---- BAM sources (include/gffx_hip.h "BAM sources"; device/bgzf.hip) ----------------------------------------------------
def _u8(data: bytes):
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    return buf, buf.ctypes.data_as(_ffi.u8p)


def bgzf_inflate(data: bytes, device: int = 0) -> bytes:
    """The BGZF members of `data`, inflated on the device (one wave per member; CRC32 and ISIZE checked)."""
    buf, ptr = _u8(data)
    n = C.c_uint64()
    check(lib().gffx_hip_bgzf_inflate(device, ptr, len(data), None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), np.uint8)
    check(lib().gffx_hip_bgzf_inflate(device, ptr, len(data), out.ctypes.data_as(_ffi.u8p), n.value, C.byref(n)))
    return out[: n.value].tobytes()


def bgzf_members(data: bytes) -> List[int]:
    """Offsets of the BGZF members of `data` (plus len(data)), by hopping their BSIZE fields (the BC subfield, wherever it
    stands among the extra subfields)."""
    off, at = [], 0
    while at < len(data):
        off.append(at)
        if len(data) - at < 18:
            raise ValueError("truncated BGZF member at offset %d" % at)
        sub, end, bsize = at + 12, at + 12 + int.from_bytes(data[at + 10:at + 12], "little"), None
        while sub + 4 <= min(end, len(data)):
            slen = int.from_bytes(data[sub + 2:sub + 4], "little")
            if data[sub:sub + 2] == b"BC" and slen == 2:
                bsize = int.from_bytes(data[sub + 4:sub + 6], "little")
            sub += 4 + slen
        if bsize is None:
            raise ValueError("no BC subfield in the BGZF member at offset %d" % at)
        at += bsize + 1
    off.append(len(data))
    return off


class _SourceReader:
    """What BamReader, SamReader and BedReader share: the gffx_hip_<stem>_* calls on one handle (device/source_stream.hpp is the
    pipeline behind both).  A subclass creates self._h and names the four tallies and the three stages of its format."""
    _stem = ""
    _count_keys: Tuple[str, ...] = ()
    _stage_keys: Tuple[str, ...] = ()

    def _fn(self, name: str):
        return getattr(lib(), "gffx_hip_%s_%s" % (self._stem, name))

    def feed(self, data: bytes) -> None:
        buf, ptr = _u8(data)
        check(self._fn("feed")(self._h, ptr, len(data)))

    def finish(self) -> None:
        check(self._fn("finish")(self._h))

    def rows(self) -> np.ndarray:
        n = self._fn("rows")(self._h)
        out = np.zeros((max(n, 1), 3), np.uint32)
        check(self._fn("copy_rows")(self._h, _p(out)))
        return out[:n]

    def counts(self) -> Dict[str, int]:
        v = [C.c_uint64() for _ in range(4)]
        check(self._fn("counts")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(self._count_keys, (x.value for x in v)))

    def stage_ms(self) -> Dict[str, float]:
        v = [C.c_double() for _ in range(3)]
        check(self._fn("stage_ms")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(self._stage_keys, (x.value for x in v)))

    def close(self) -> None:
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamReader(_SourceReader):
    """gffx_hip_bam_*: the kept (seqid, start, end) rows of a BAM stream.  ref_seq[tid] = seqid number or 0xFFFFFFFF;
    header_bytes = the BAM header's size in the decompressed stream."""
    _stem, _count_keys, _stage_keys = "bam", ("records", "unmapped", "no_seq", "kept"), ("inflate", "frame", "rows")

    def __init__(self, ref_seq, header_bytes: int, chunk_bytes: int = 0, device: int = 0):
        rs = _u32(ref_seq)
        self._h = C.c_void_p()
        check(lib().gffx_hip_bam_create(device, len(rs), _p(rs) if len(rs) else None, header_bytes, chunk_bytes, C.byref(self._h)))


def bam_rows(data: bytes, ref_seq, header_bytes: int, chunk_bytes: int = 0, feed_members: int = 0, device: int = 0) -> np.ndarray:
    """The rows of a whole BAM stream in file order.  feed_members > 0: fed that many members per call."""
    r = BamReader(ref_seq, header_bytes, chunk_bytes, device)
    try:
        if feed_members > 0:
            off = bgzf_members(data)
            for i in range(0, len(off) - 1, feed_members):
                r.feed(data[off[i]:off[min(i + feed_members, len(off) - 1)]])
        else:
            r.feed(data)
        r.finish()
        return r.rows()
    finally:
        r.close()


# ---- SAM sources (include/gffx_hip.h "SAM sources"; device/sam.hip) ----------------------------------------------------
class SamReader(_SourceReader):
    """gffx_hip_sam_*: the kept (seqid, start, end) rows of a SAM stream, plain text or BGZF-compressed (bgzf=True).
    names = the SN values of the header's @SQ lines in order, ref_seq[tid] = seqid number or 0xFFFFFFFF;
    header_bytes = the offset of the first line that does not begin with '@' in the (inflated) text."""
    _stem, _count_keys, _stage_keys = "sam", ("lines", "unmapped", "no_seq", "kept"), ("inflate", "lines", "rows")

    def __init__(self, names, ref_seq, header_bytes: int, chunk_bytes: int = 0, bgzf: bool = False, device: int = 0):
        nb = [n if isinstance(n, bytes) else str(n).encode() for n in names]
        rs = _u32(ref_seq)
        if len(nb) != len(rs):
            raise ValueError("names and ref_seq differ in length")
        off = np.zeros(len(nb) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in nb], dtype=np.uint64) if nb else 0
        self._h = C.c_void_p()
        check(lib().gffx_hip_sam_create(device, len(nb), b"".join(nb), off.ctypes.data_as(_ffi.u64p), _p(rs) if len(rs) else None,
                                        header_bytes, chunk_bytes, int(bool(bgzf)), C.byref(self._h)))


def sam_rows(data: bytes, names, ref_seq, header_bytes: int, chunk_bytes: int = 0, bgzf: bool = False, feed_bytes: int = 0,
             feed_members: int = 0, device: int = 0, counts: Optional[dict] = None) -> np.ndarray:
    """The rows of a whole SAM stream in file order.  feed_bytes > 0: plain text fed in pieces of that many bytes;
    feed_members > 0: BGZF fed that many members per call.  counts: filled with SamReader.counts()."""
    r = SamReader(names, ref_seq, header_bytes, chunk_bytes, bgzf, device)
    try:
        if bgzf and feed_members > 0:
            off = bgzf_members(data)
            for i in range(0, len(off) - 1, feed_members):
                r.feed(data[off[i]:off[min(i + feed_members, len(off) - 1)]])
        elif not bgzf and feed_bytes > 0:
            for i in range(0, len(data), feed_bytes):
                r.feed(data[i:i + feed_bytes])
        else:
            r.feed(data)
        r.finish()
        if counts is not None:
            counts.update(r.counts())
        return r.rows()
    finally:
        r.close()


# ---- BED sources (include/gffx_hip.h "BED sources"; device/bed.hip) ----------------------------------------------------
BED_INTERSECT, BED_DEPTH = 0, 1  # the dialects: host/bed_parse.cpp (`gffx intersect`), host/depth.cpp (`gffx depth` / `coverage`)


class BedReader(_SourceReader):
    """gffx_hip_bed_*: the kept (seqid, start, end) rows of a BED stream, plain text or BGZF-compressed (bgzf=True), by the
    rules of one of the two host parsers (dialect).  names[i] = the name of seqid number i."""
    _stem, _count_keys, _stage_keys = "bed", ("lines", "skipped", "no_seq", "kept"), ("inflate", "lines", "rows")

    def __init__(self, names, dialect: int, chunk_bytes: int = 0, bgzf: bool = False, device: int = 0):
        nb = [n if isinstance(n, (bytes, bytearray)) else str(n).encode() for n in names]
        off = np.zeros(len(nb) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in nb], dtype=np.uint64) if nb else 0
        self._h = C.c_void_p()
        check(lib().gffx_hip_bed_create(device, len(nb), b"".join(nb), off.ctypes.data_as(_ffi.u64p), int(dialect), chunk_bytes,
                                        int(bool(bgzf)), C.byref(self._h)))


def bed_rows(data: bytes, names, dialect: int, chunk_bytes: int = 0, bgzf: bool = False, feed_bytes: int = 0, device: int = 0,
             counts: Optional[dict] = None) -> np.ndarray:
    """The rows of a whole BED stream in file order.  feed_bytes > 0: plain text fed in pieces of that many bytes, BGZF one
    member per call.  counts: filled with BedReader.counts()."""
    r = BedReader(names, dialect, chunk_bytes, bgzf, device)
    try:
        if bgzf and feed_bytes > 0:
            off = bgzf_members(data)
            for i in range(len(off) - 1):
                r.feed(data[off[i]:off[i + 1]])
        elif feed_bytes > 0:
            for i in range(0, len(data), feed_bytes):
                r.feed(data[i:i + feed_bytes])
        else:
            r.feed(data)
        r.finish()
        if counts is not None:
            counts.update(r.counts())
        return r.rows()
    finally:
        r.close()


# ---- `gffx extract` (include/gffx_hip.h "gffx extract"; device/ids.hip) ------------------------------------------------
NONE = 0xFFFFFFFF  # a name that is not in the table / a fid without a valid root


def _cat(names) -> Tuple[bytes, np.ndarray]:
    nb = [n if isinstance(n, (bytes, bytearray)) else str(n).encode() for n in names]
    off = np.zeros(len(nb) + 1, np.uint64)
    if nb:
        off[1:] = np.cumsum([len(n) for n in nb], dtype=np.uint64)
    return b"".join(nb), off


def _bitmap_indices(fn, handle, words: int) -> np.ndarray:
    """the set bits of the `words` 64-bit words that fn (a gffx_hip_*_copy_*_bitmap) downloads, ascending"""
    w = np.zeros(max(words, 1), np.uint64)
    check(fn(handle, w.ctypes.data_as(u64p), words))
    return np.flatnonzero(np.unpackbits(w[:words].view(np.uint8), bitorder="little")).astype(np.uint32)


def _filter_lines(fn, handle, text: bytes, line_off, line_root, types) -> np.ndarray:
    """one call of fn (a gffx_hip_*_filter_lines): keep[i] of the lines text[line_off[i]:line_off[i + 1]]"""
    lo = np.ascontiguousarray(line_off, dtype=np.uint64)
    lr = _u32(line_root)
    n = len(lr)
    if len(lo) != n + 1:
        raise ValueError("line_off needs one entry more than line_root")
    keep = np.zeros(max(n, 1), np.uint8)
    tb, toff = _cat(types or [])
    toff32 = toff.astype(np.uint32)
    buf, ptr = _u8(text)
    tbuf, tptr = _u8(tb)
    check(fn(handle, ptr, len(text), n, lo.ctypes.data_as(u64p), _p(lr) if n else None, int(types is not None), len(toff) - 1, tptr,
             _p(toff32), keep.ctypes.data_as(_ffi.u8p)))
    return keep[:n]


class FeatureIds:
    """gffx_hip_ids_*: the feature-ID table of `.fts` with the parent pointers of `.prt` on the device (the reference's FtsMap +
    PrtMap, index_loader/fts.rs:9-93, prt.rs:18-102).  A name's fid is the LAST line that holds it; a fid's root is where the
    parent chase ends, NONE when a child or parent is out of range -- or, unlike the reference, which never returns then,
    when a parent cycle has no root.  hash_bits (0..31) is a test hook: only that many low bits of the name hash are used."""

    def __init__(self, handle, n_names: int, n_prt: int):
        self._h = handle
        self.n = n_names
        self._words = (max(n_names, n_prt) + 63) // 64

    @classmethod
    def from_arrays(cls, names, prt, hash_bits: Optional[int] = None, device: int = 0) -> "FeatureIds":
        blob, off = _cat(names)
        p = _u32(prt)
        buf, ptr = _u8(blob)
        h = C.c_void_p()
        check(lib().gffx_hip_ids_create(device, len(off) - 1, ptr, off.ctypes.data_as(u64p), len(p), _p(p) if len(p) else None,
                                        -1 if hash_bits is None else int(hash_bits), C.byref(h)))
        return cls(h, len(off) - 1, len(p))

    @classmethod
    def from_files(cls, gff: str, hash_bits: Optional[int] = None, device: int = 0) -> "FeatureIds":
        """`<gff>.fts` (fts.rs:97-138: empty lines dropped, a trailing "\\r" stripped) and `<gff>.prt` (prt.rs:108-125)"""
        with open(gff + ".fts", "rb") as f:
            names = [ln[:-1] if ln.endswith(b"\r") else ln for ln in f.read().split(b"\n") if ln]
        for n in names:
            n.decode("utf-8")  # "FTS contains invalid UTF-8"
        raw = open(gff + ".prt", "rb").read()
        if len(raw) % 4:
            raise ValueError("Corrupted PRT: not aligned to u32")
        return cls.from_arrays(names, np.frombuffer(raw, dtype="<u4"), hash_bits, device)

    def close(self) -> None:
        if self._h:
            lib().gffx_hip_ids_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def options(self) -> dict:
        return _options(lib().gffx_hip_ids_options, self._h)

    def resolve(self, names) -> Tuple[np.ndarray, np.ndarray]:
        """(fids, roots) per name, NONE for a name that is not found / a fid without a valid root; the found fids and the
        valid roots are added to the handle's bitmaps (requested_fids / unique_roots) until reset()."""
        blob, off = _cat(names)
        nq = len(off) - 1
        fids, roots = np.zeros(max(nq, 1), np.uint32), np.zeros(max(nq, 1), np.uint32)
        buf, ptr = _u8(blob)
        check(lib().gffx_hip_ids_resolve(self._h, nq, ptr, off.ctypes.data_as(u64p), _p(fids), _p(roots)))
        return fids[:nq], roots[:nq]

    def _bits(self, fn) -> np.ndarray:
        return _bitmap_indices(fn, self._h, self._words)

    def unique_roots(self) -> np.ndarray:
        return self._bits(lib().gffx_hip_ids_copy_root_bitmap)

    def requested_fids(self) -> np.ndarray:
        return self._bits(lib().gffx_hip_ids_copy_requested_bitmap)

    def reset(self) -> None:
        check(lib().gffx_hip_ids_reset(self._h))

    def filter_lines(self, text: bytes, line_off, line_root, types=None) -> np.ndarray:
        """keep[i] for line i = text[line_off[i]:line_off[i + 1]] (whole lines back to back, each with its line ending) in the
        block of root line_root[i]: write_gff_output_filtered's test with the key "ID" (utils/common.rs:418-431).  types: None,
        or the allowed column-3 names (-T already split at ',', trimmed, the empty ones dropped; an empty list keeps nothing)."""
        return _filter_lines(lib().gffx_hip_ids_filter_lines, self._h, text, line_off, line_root, types)

    def stage_ms(self) -> Dict[str, float]:
        v = [C.c_double() for _ in range(3)]
        check(lib().gffx_hip_ids_stage_ms(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("build", "resolve", "filter"), (x.value for x in v)))


# ---- `gffx search` (include/gffx_hip.h "gffx search"; device/search.hip; the regex compiler in libgffx_host.so) -----------
_host_lib = _ffi.host_lib  # (include/gffx_host.h: the regex compiler lives on the host and needs no device)


class RegexError(ValueError):
    """a pattern outside the subset of `gffx search -r`, or one that needs more DFA states than the cap"""


class CompiledRegex:
    """The DFAs of a pattern list (host/regex_dfa.hpp): groups[g] = dict(n_states, n_classes, init, first_pattern, n_patterns,
    cls (256 x u8: byte -> column), trans (n_states x n_classes u16; the last column is the end of the text; state 0 accepts
    and is absorbing)).  match(values) runs device/search_core.hpp's loop on the host."""

    def __init__(self, handle):
        self._h = handle
        L = _host_lib()
        self.groups: List[dict] = []
        for g in range(L.gffx_host_regex_groups(handle)):
            v = [C.c_uint32() for _ in range(5)]
            if L.gffx_host_regex_group_info(handle, g, *[C.byref(x) for x in v]) != 0:
                raise RuntimeError("gffx_host_regex_group_info failed for group %d" % g)
            ns, nc, init, first, npat = (x.value for x in v)
            cls = np.zeros(256, np.uint8)
            trans = np.zeros(ns * nc, np.uint16)
            if L.gffx_host_regex_group_tables(handle, g, cls.ctypes.data_as(_ffi.u8p), trans.ctypes.data_as(C.POINTER(C.c_uint16))) != 0:
                raise RuntimeError("gffx_host_regex_group_tables failed for group %d" % g)
            self.groups.append(dict(n_states=ns, n_classes=nc, init=init, first_pattern=first, n_patterns=npat, cls=cls,
                                    trans=trans.reshape(ns, nc)))

    def match(self, values) -> np.ndarray:
        blob, off = _cat(values)
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.uint8)
        buf, ptr = _u8(blob)
        if _host_lib().gffx_host_regex_match(self._h, n, ptr, off.ctypes.data_as(u64p), out.ctypes.data_as(_ffi.u8p)) != 0:
            raise RuntimeError("gffx_host_regex_match failed (a closed CompiledRegex?)")
        return out[:n].astype(bool)

    def close(self) -> None:
        if self._h:
            _host_lib().gffx_host_regex_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compile_regex(patterns, max_states: int = 0) -> CompiledRegex:
    """The patterns (str or bytes) of one `gffx search -r` run as DFAs; RegexError for syntax outside the subset and for a
    pattern over the state cap (max_states; 0: GFFX_SEARCH_DFA_STATES, else the 64 KiB default).  Needs no device."""
    blob, off = _cat(patterns)
    buf, ptr = _u8(blob)
    h = C.c_void_p()
    err = C.create_string_buffer(4096)
    if _host_lib().gffx_host_regex_compile(len(off) - 1, ptr, off.ctypes.data_as(u64p), int(max_states), C.byref(h), err, len(err)) != 0:
        raise RegexError(err.value.decode(errors="replace"))
    return CompiledRegex(h)


class AttrSearch:
    """gffx_hip_attrs_*: the attribute values of `.atn` with the fid -> aid words of `.a2f` and the parent words of `.prt` on
    the device (commands/search.rs:89-218).  match / match_regex OR into the matched-aid bitmap until reset(); resolve() turns
    it into the fid, root and invalid-fid bitmaps and the (value class, root) pair set that filter_lines tests against.
    hash_bits (0..31) and dfa_path ("lds" / "global") are test hooks; results never depend on them."""

    def __init__(self, handle, n_values: int, n_a2f: int, n_prt: int):
        self._h = handle
        self.n = n_values
        self._mwords = (n_values + 63) // 64
        self._words = (max(n_a2f, n_prt) + 63) // 64

    @classmethod
    def from_arrays(cls, values, a2f, prt, key="gene_name", hash_bits: Optional[int] = None, dfa_path: Optional[str] = None,
                    device: int = 0) -> "AttrSearch":
        blob, off = _cat(values)
        a, p = _u32(a2f), _u32(prt)
        kb = key if isinstance(key, (bytes, bytearray)) else str(key).encode()
        buf, ptr = _u8(blob)
        kbuf, kptr = _u8(kb)
        h = C.c_void_p()
        check(lib().gffx_hip_attrs_create(device, len(off) - 1, ptr, off.ctypes.data_as(u64p), len(a), _p(a) if len(a) else None, len(p),
                                          _p(p) if len(p) else None, kptr, len(kb), -1 if hash_bits is None else int(hash_bits),
                                          {None: 0, "lds": 1, "global": 2}[dfa_path], C.byref(h)))
        return cls(h, len(off) - 1, len(a), len(p))

    def close(self) -> None:
        if self._h:
            lib().gffx_hip_attrs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def options(self) -> dict:
        return _options(lib().gffx_hip_attrs_options, self._h)

    def match(self, wanted) -> None:
        """exact: every aid whose value is one of the wanted strings (search.rs:105-110)"""
        blob, off = _cat(wanted)
        buf, ptr = _u8(blob)
        check(lib().gffx_hip_attrs_match_exact(self._h, len(off) - 1, ptr, off.ctypes.data_as(u64p)))

    def match_regex(self, compiled: CompiledRegex) -> List[str]:
        """every aid whose value some group's DFA accepts (search.rs:99-103); returns the kernel form each group's launch took"""
        names = []
        for g in compiled.groups:
            trans = np.ascontiguousarray(g["trans"], dtype=np.uint16)
            check(lib().gffx_hip_attrs_match_dfa(self._h, g["n_states"], g["n_classes"], g["init"], g["cls"].ctypes.data_as(_ffi.u8p),
                                                 trans.ctypes.data_as(C.POINTER(C.c_uint16))))
            names.append(lib().gffx_hip_attrs_dfa_kernel(self._h).decode())
        return names

    def reset(self) -> None:
        check(lib().gffx_hip_attrs_reset(self._h))

    def resolve(self) -> None:
        check(lib().gffx_hip_attrs_resolve(self._h))

    def _bits(self, fn, words) -> np.ndarray:
        return _bitmap_indices(fn, self._h, words)

    def matched_aids(self) -> np.ndarray:
        return self._bits(lib().gffx_hip_attrs_copy_matched_bitmap, self._mwords)

    def matched_fids(self) -> np.ndarray:
        return self._bits(lib().gffx_hip_attrs_copy_fid_bitmap, self._words)

    def unique_roots(self) -> np.ndarray:
        return self._bits(lib().gffx_hip_attrs_copy_root_bitmap, self._words)

    def invalid_fids(self) -> np.ndarray:
        return self._bits(lib().gffx_hip_attrs_copy_invalid_bitmap, self._words)

    def filter_lines(self, text: bytes, line_off, line_root, types=None) -> np.ndarray:
        """keep[i] for line i = text[line_off[i]:line_off[i + 1]] in the block of root line_root[i]: write_gff_output_filtered's
        test with the key `<attribute name>` (utils/common.rs:418-431) against the pairs of the last resolve().  types as for
        FeatureIds.filter_lines."""
        return _filter_lines(lib().gffx_hip_attrs_filter_lines, self._h, text, line_off, line_root, types)

    def stage_ms(self) -> Dict[str, float]:
        v = [C.c_double() for _ in range(4)]
        check(lib().gffx_hip_attrs_stage_ms(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("build", "match", "resolve", "filter"), (x.value for x in v)))


# ---- `gffx index --gpu` (include/gffx_hip.h "gffx index --gpu"; device/gff.hip) -----------------------------------------
DEFAULT_SKIP_TYPES = "remark,note,comment,region,gap,assembly_gap,contig,scaffold,source"


class GffBuilt:
    """The arrays of an index, with the fields of oracle.gffx_oracle_py.Built: ids (the `.fts` lines), fid, prt, a2f, atn,
    seqids, gof [(fid, seq, start offset, end offset)], trees_input [per seqid: (start, end, fid) in file order]."""
    FIELDS = ("ids", "fid", "prt", "a2f", "atn", "seqids", "gof", "trees_input")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def astuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)


class GffIndexer:
    """gffx_hip_gff_*: GFF3 text in (file order, cut anywhere), the arrays of the side-cars out.  skip_types is the raw
    --skip-types string (split at ',', not trimmed).  chunk_bytes bounds a device pass (0: 64 MiB); hash_bits (0..31) is
    the test hook of FeatureIds.  A malformed line fails feed() / finish(); error() then names it."""
    ERROR_KINDS = {4: "BAD_UTF8", 5: "COLUMNS", 6: "DIGITS", 7: "NO_ID"}
    _count_keys = ("lines", "blank", "skipped_type", "zero_end", "rows", "roots", "seqids", "attr_values")
    _stage_keys = ("scan", "rows", "table", "resolve", "number")

    def __init__(self, attr_key: str = "gene_name", skip_types: str = DEFAULT_SKIP_TYPES, device: int = 0, chunk_bytes: int = 0,
                 hash_bits: int = -1):
        key = attr_key if isinstance(attr_key, bytes) else attr_key.encode()
        raw = skip_types if isinstance(skip_types, bytes) else skip_types.encode()
        parts = raw.split(b",")
        off = np.zeros(len(parts) + 1, np.uint32)
        off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint32)
        self._h = C.c_void_p()
        check(lib().gffx_hip_gff_create(device, key, len(parts), b"".join(parts), _p(off), chunk_bytes, hash_bits, C.byref(self._h)))

    def feed(self, data: bytes) -> None:
        buf, ptr = _u8(data)
        check(lib().gffx_hip_gff_feed(self._h, ptr, len(data)))

    def finish(self) -> None:
        check(lib().gffx_hip_gff_finish(self._h))

    def error(self) -> Optional[Tuple[int, str]]:
        """(file offset of the first bad line, its kind), or None"""
        off, kind = C.c_uint64(), C.c_int()
        check(lib().gffx_hip_gff_error(self._h, C.byref(off), C.byref(kind)))
        return (off.value, self.ERROR_KINDS.get(kind.value, str(kind.value))) if kind.value else None

    @property
    def counts(self) -> Dict[str, int]:
        v = [C.c_uint64() for _ in range(8)]
        check(lib().gffx_hip_gff_counts(self._h, *[C.byref(x) for x in v]))
        return dict(zip(self._count_keys, (x.value for x in v)))

    @property
    def stage_ms(self) -> Dict[str, float]:
        v = [C.c_double() for _ in range(5)]
        check(lib().gffx_hip_gff_stage_ms(self._h, *[C.byref(x) for x in v]))
        return dict(zip(self._stage_keys, (x.value for x in v)))

    def _bytes(self, size_fn, copy_fn) -> bytes:
        out = np.zeros(max(size_fn(self._h), 1), np.uint8)
        check(copy_fn(self._h, out.ctypes.data_as(_ffi.u8p)))
        return out[:size_fn(self._h)].tobytes()

    def _words(self, n: int, copy_fn, dtype=np.uint32) -> np.ndarray:
        out = np.zeros(max(n, 1), dtype)
        check(copy_fn(self._h, out.ctypes.data_as(u64p if dtype == np.uint64 else u32p)))
        return out[:n]

    def fts(self) -> bytes:
        return self._bytes(lib().gffx_hip_gff_fts_bytes, lib().gffx_hip_gff_copy_fts)

    def atn(self) -> bytes:
        return self._bytes(lib().gffx_hip_gff_atn_bytes, lib().gffx_hip_gff_copy_atn)

    def sqs(self) -> bytes:
        return self._bytes(lib().gffx_hip_gff_seqids_bytes, lib().gffx_hip_gff_copy_seqids)

    def gof(self) -> bytes:
        L = lib()
        return self._bytes(lambda h: 24 * L.gffx_hip_gff_n_roots(h), L.gffx_hip_gff_copy_gof)

    def fid(self) -> np.ndarray:
        return self._words(lib().gffx_hip_gff_n_rows(self._h), lib().gffx_hip_gff_copy_fid)

    def prt(self) -> np.ndarray:
        return self._words(lib().gffx_hip_gff_n_rows(self._h), lib().gffx_hip_gff_copy_prt)

    def a2f(self) -> np.ndarray:
        return self._words(lib().gffx_hip_gff_n_rows(self._h), lib().gffx_hip_gff_copy_a2f)

    def roots(self) -> np.ndarray:
        """(start, end, fid, seqid) per root, in file order"""
        n = lib().gffx_hip_gff_n_roots(self._h)
        return self._words(4 * n, lib().gffx_hip_gff_copy_roots).reshape(-1, 4)

    def skipped_lines(self) -> np.ndarray:
        return self._words(lib().gffx_hip_gff_n_skipped_lines(self._h), lib().gffx_hip_gff_copy_skipped_lines, np.uint64)

    def warn_rows(self) -> np.ndarray:
        return self._words(lib().gffx_hip_gff_n_warn_rows(self._h), lib().gffx_hip_gff_copy_warn_rows)

    def built(self) -> GffBuilt:
        names = lambda b: [x.decode("utf-8") for x in b.split(b"\n")[:-1]]  # noqa: E731
        seqids = names(self.sqs())
        gof = np.frombuffer(self.gof(), dtype=np.dtype([("fid", "<u4"), ("seq", "<u4"), ("a", "<u8"), ("z", "<u8")]))
        trees: List[List[Tuple[int, int, int]]] = [[] for _ in seqids]
        for s, e, f, q in self.roots().tolist():
            trees[q].append((s, e, f))
        return GffBuilt(ids=names(self.fts()), fid=self.fid().tolist(), prt=self.prt().tolist(), a2f=self.a2f().tolist(),
                        atn=names(self.atn()), seqids=seqids, gof=[tuple(int(x) for x in g) for g in gof.tolist()], trees_input=trees)

    def close(self) -> None:
        if self._h:
            lib().gffx_hip_gff_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gff_index(data: bytes, attr_key: str = "gene_name", skip_types: str = DEFAULT_SKIP_TYPES, chunk_bytes: int = 0, feed_bytes: int = 0,
              hash_bits: int = -1, device: int = 0) -> GffIndexer:
    """A finished GffIndexer over the whole text (feed_bytes > 0: fed in pieces of that many bytes).  The caller closes it."""
    g = GffIndexer(attr_key, skip_types, device, chunk_bytes, hash_bits)
    try:
        if feed_bytes > 0:
            for i in range(0, len(data), feed_bytes):
                g.feed(data[i:i + feed_bytes])
        else:
            g.feed(data)
        g.finish()
    except Exception:
        g.close()
        raise
    return g


# ---- `gffx seq`: the genome object and the sequence plan (device/genome.hip, device/seq.hip) ----------------------------------
SEQ_MINUS, SEQ_DROPPED = 1, 8  # rec_flags bits (GFFX_SEQ_*); the phase 0 .. 2 sits in bits 1 .. 2


def seq_tile() -> int:
    """SEQ_TILE: the output bytes per block of the emit kernel."""
    return int(lib().gffx_hip_seq_tile())


def scan64_constants() -> Tuple[int, int]:
    """(values per tile, tile sums per step of the single carry block) of the 64-bit prefix sum behind the genome's line and byte
    offsets, the seq plan's ``pre`` and ``body_off`` and the effect build's ``pre``: a scan of more than tile * carry_tiles values
    takes a second carry step."""
    return int(lib().gffx_hip_scan64_tile()), int(lib().gffx_hip_scan64_carry_tiles())


class Genome:
    """gffx_hip_genome_*: a plain FASTA text, fed in pieces cut anywhere, packed into one arena of bases on the device.
    After ``finish``: ``names`` (bytes), ``lengths`` (u32), ``offsets`` (u64, n_seq + 1: where every sequence begins in the
    arena, the last one the base total) and ``bases(at, n)``."""

    def __init__(self, device: int = 0, chunk_bytes: int = 0):
        self._h = C.c_void_p()
        check(lib().gffx_hip_genome_create(int(device), int(chunk_bytes), C.byref(self._h)))
        self.names: List[bytes] = []
        self.lengths = np.zeros(0, dtype=np.uint32)
        self.offsets = np.zeros(1, dtype=np.uint64)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_genome_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, n_bytes: int) -> None:
        check(lib().gffx_hip_genome_reserve(self._h, int(n_bytes)))

    def feed(self, data: bytes) -> None:
        buf, p = _u8(data)
        check(lib().gffx_hip_genome_feed(self._h, p, len(data)))

    def finish(self) -> None:
        check(lib().gffx_hip_genome_finish(self._h))
        n = int(lib().gffx_hip_genome_n_seq(self._h))
        names = np.zeros(max(int(lib().gffx_hip_genome_name_bytes(self._h)), 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        check(lib().gffx_hip_genome_copy_names(self._h, names.ctypes.data_as(_ffi.u8p), off.ctypes.data_as(u64p)))
        raw = names.tobytes()
        self.names = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
        self.offsets = np.zeros(n + 1, dtype=np.uint64)
        self.lengths = np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().gffx_hip_genome_copy_seqs(self._h, self.offsets.ctypes.data_as(u64p), _p(self.lengths)))
        self.lengths = self.lengths[:n]

    @property
    def n_bases(self) -> int:
        return int(lib().gffx_hip_genome_n_bases(self._h))

    def bases(self, at: int = 0, n: Optional[int] = None) -> bytes:
        n = self.n_bases - at if n is None else n
        out = np.zeros(max(n, 1), dtype=np.uint8)
        check(lib().gffx_hip_genome_copy_bases(self._h, int(at), int(n), out.ctypes.data_as(_ffi.u8p)))
        return out[:n].tobytes()

    def sequence(self, i: int) -> bytes:
        return self.bases(int(self.offsets[i]), int(self.lengths[i]))

    def stage_ms(self) -> Dict[str, float]:
        a, b = C.c_double(), C.c_double()
        check(lib().gffx_hip_genome_stage_ms(self._h, C.byref(a), C.byref(b)))
        return {"lines_ms": a.value, "pack_ms": b.value}


def genome_from_fasta(data: bytes, feed_bytes: int = 0, chunk_bytes: int = 0, device: int = 0) -> Genome:
    """A finished Genome over the whole text (feed_bytes > 0: fed in pieces of that many bytes).  The caller closes it."""
    g = Genome(device, chunk_bytes)
    try:
        if feed_bytes > 0:
            for i in range(0, len(data), feed_bytes):
                g.feed(data[i:i + feed_bytes])
        else:
            g.feed(data)
        g.finish()
    except Exception:
        g.close()
        raise
    return g


class SeqPlan:
    """gffx_hip_seq_*: the bodies of the records of ``rows`` -- (n, 4) u32 (record, sequence number, start - 1, end) -- over a
    finished Genome.  ``rec_flags[r]`` = SEQ_MINUS | phase << 1 | SEQ_DROPPED.  ``body_off`` (u64, n_records + 1) and ``dropped``
    (u8) come back from the plan; ``emit(at, n)`` gives bytes [at, at + n) of the concatenated bodies."""

    def __init__(self, genome: Genome, rows, rec_flags, translate: bool = False, width: int = 60):
        r = _u32(rows).reshape(-1, 4)
        f = np.ascontiguousarray(rec_flags, dtype=np.uint8)
        self._genome = genome  # (it must outlive the plan)
        self.n_records = int(f.shape[0])
        self._h = C.c_void_p()
        check(lib().gffx_hip_seq_create(genome._h, r.shape[0], _p(r), self.n_records, f.ctypes.data_as(_ffi.u8p), 1 if translate else 0, int(width),
                                        C.byref(self._h)))
        self.body_off = np.zeros(self.n_records + 1, dtype=np.uint64)
        self.dropped = np.zeros(max(self.n_records, 1), dtype=np.uint8)
        check(lib().gffx_hip_seq_copy_offsets(self._h, self.body_off.ctypes.data_as(u64p), self.dropped.ctypes.data_as(_ffi.u8p)))
        self.dropped = self.dropped[:self.n_records]

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_seq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def body_bytes(self) -> int:
        return int(lib().gffx_hip_seq_body_bytes(self._h))

    def emit(self, at: int = 0, n: Optional[int] = None, slot: int = 0) -> bytes:
        n = self.body_bytes - at if n is None else n
        if n == 0:
            return b""
        check(lib().gffx_hip_seq_emit_start(self._h, slot, int(at), int(n)))
        p = _ffi.u8p()
        check(lib().gffx_hip_seq_emit_wait(self._h, slot, C.byref(p)))
        return C.string_at(p, n)

    def emit_sliced(self, slice_bytes: int) -> bytes:
        """The whole concatenation in slices of ``slice_bytes``, slice k + 1 started before slice k is taken (as the command does)."""
        total, out = self.body_bytes, []
        starts = list(range(0, total, slice_bytes))
        for k, at in enumerate(starts):
            if k == 0:
                check(lib().gffx_hip_seq_emit_start(self._h, 0, at, min(slice_bytes, total - at)))
            p = _ffi.u8p()
            check(lib().gffx_hip_seq_emit_wait(self._h, k & 1, C.byref(p)))
            if k + 1 < len(starts):
                nxt = starts[k + 1]
                check(lib().gffx_hip_seq_emit_start(self._h, (k + 1) & 1, nxt, min(slice_bytes, total - nxt)))
            out.append(C.string_at(p, min(slice_bytes, total - at)))
        return b"".join(out)

    def stage_ms(self) -> Dict[str, float]:
        a, b = C.c_double(), C.c_double()
        check(lib().gffx_hip_seq_stage_ms(self._h, C.byref(a), C.byref(b)))
        return {"plan_ms": a.value, "emit_ms": b.value}


# ---- `gffx effect`: single-base substitutions against transcripts (device/effect.hip, the rules: effect_core.hpp) --------------
EFFECT_CLASSES = ("partial_codon", "coding_unknown", "stop_retained", "synonymous", "stop_gained", "stop_lost", "start_lost", "missense",
                  "noncoding_exon", "5_prime_UTR", "3_prime_UTR", "intron", "splice_donor", "splice_acceptor", "intergenic")
# what run_any may give as well (`gffx effect --indels`): the 15 above keep their numbers
EFFECT_CLASSES_ALL = EFFECT_CLASSES + ("frameshift", "inframe_insertion", "inframe_deletion", "transcript_ablation", "unclassified_model")
EFFECT_CDS, EFFECT_EXON = 0, 1  # a member row's kind
EFFECT_NO_SEQ = 0xFFFFFFFF      # an allele's sequence number when the FASTA lacks its sequence
EFFECT_RECORD = np.dtype([("q", "<u8"), ("c", "<u8"), ("transcript", "<u4"), ("cls", "u1"), ("k", "u1"), ("ref_match", "u1"), ("aa_ref", "u1"),
                          ("aa_alt", "u1"), ("codon_ref", "u1", (3,)), ("codon_alt", "u1", (3,)), ("pad", "u1")])


def effect_trim(pos: int, ref: bytes, alt: bytes):
    """The trimming of `gffx effect --indels`: (x0, d, m, R', A').  Case folded, the longest common prefix goes first, then the
    longest common suffix of what remains; x0 = pos + the prefix.  The genome is not consulted: nothing is left-aligned."""
    r, a = bytes(ref).upper(), bytes(alt).upper()
    pfx = 0
    while pfx < len(r) and pfx < len(a) and r[pfx] == a[pfx]:
        pfx += 1
    d, m = len(r) - pfx, len(a) - pfx
    while d and m and r[pfx + d - 1] == a[pfx + m - 1]:
        d, m = d - 1, m - 1
    return int(pos) + pfx, d, m, bytes(ref)[pfx:pfx + d], bytes(alt)[pfx:pfx + m]


def effect_rows_any(alleles):
    """((n, 6) u32 rows, the arena) of run_any for alleles (sequence number, x0, R', A')."""
    rows, arena = [], bytearray()
    for q, x0, ref, ins in alleles:
        rows.append((q, x0, len(ref), len(ins), len(arena) & 0xFFFFFFFF, len(arena) >> 32))
        arena += bytes(ref) + bytes(ins)
    return np.array(rows, dtype=np.uint32).reshape(-1, 6), bytes(arena)


class Effect:
    """gffx_hip_effect_*: per (allele, kept transcript whose span contains it) one EFFECT_RECORD.  ``rows``: (n, 5) u32 (transcript,
    sequence number, start - 1, end, kind) over a finished Genome; ``tr_flags[t]`` = SEQ_MINUS | phase << 1 | SEQ_DROPPED.
    ``dropped`` (u8) and ``span`` ((n_transcripts, 2) u32: first and last base) come back from the build.  ``run(alleles)`` --
    (n, 3) u32 (sequence number, x, REF | ALT << 8) -- gives (offsets[n + 1] u64, ref_match[n] u8, records)."""

    def __init__(self, genome: Genome, rows, tr_flags, max_alleles: int = 1 << 20):
        r = _u32(rows).reshape(-1, 5)
        f = np.ascontiguousarray(tr_flags, dtype=np.uint8)
        assert int(lib().gffx_hip_effect_record_bytes()) == EFFECT_RECORD.itemsize
        self._genome = genome  # (it must outlive the object)
        self.n_transcripts = int(f.shape[0])
        self.max_alleles = int(max_alleles)
        self._h = C.c_void_p()
        check(lib().gffx_hip_effect_create(genome._h, r.shape[0], _p(r), self.n_transcripts, f.ctypes.data_as(_ffi.u8p), self.max_alleles, C.byref(self._h)))
        self.dropped = np.zeros(max(self.n_transcripts, 1), dtype=np.uint8)
        self.span = np.zeros((max(self.n_transcripts, 1), 2), dtype=np.uint32)
        check(lib().gffx_hip_effect_copy_transcripts(self._h, self.dropped.ctypes.data_as(_ffi.u8p), _p(self.span)))
        self.dropped, self.span = self.dropped[:self.n_transcripts], self.span[:self.n_transcripts]

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().gffx_hip_effect_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def start(self, slot: int, alleles) -> int:
        a = _u32(alleles).reshape(-1, 3)
        check(lib().gffx_hip_effect_run_start(self._h, int(slot), _p(a), a.shape[0]))
        return int(a.shape[0])

    def wait(self, slot: int, n: int):
        """The results of the slot's chunk of n alleles, copied out of the pinned buffers."""
        off, rm, rec, pairs = u64p(), _ffi.u8p(), _ffi.u8p(), C.c_uint64()
        check(lib().gffx_hip_effect_run_wait(self._h, int(slot), C.byref(off), C.byref(rm), C.byref(rec), C.byref(pairs)))
        offsets = np.frombuffer(C.string_at(off, 8 * (n + 1)), dtype=np.uint64).copy()
        ref_match = np.frombuffer(C.string_at(rm, n), dtype=np.uint8).copy()
        records = np.frombuffer(C.string_at(rec, EFFECT_RECORD.itemsize * pairs.value), dtype=EFFECT_RECORD).copy()
        return offsets, ref_match, records

    def run(self, alleles, slot: int = 0):
        return self.wait(slot, self.start(slot, alleles))

    def run_chunked(self, alleles, chunk_rows: int):
        """All alleles in chunks of ``chunk_rows``, chunk k + 1 started before chunk k is taken (as the command does): the
        concatenated (offsets, ref_match, records)."""
        a = _u32(alleles).reshape(-1, 3)
        starts = list(range(0, a.shape[0], chunk_rows))
        offs, rms, recs, base = [np.zeros(1, dtype=np.uint64)], [], [], 0
        for k, at in enumerate(starts):
            if k == 0:
                self.start(0, a[at:at + chunk_rows])
            n = min(chunk_rows, a.shape[0] - at)
            if k + 1 < len(starts):
                self.start((k + 1) & 1, a[starts[k + 1]:starts[k + 1] + chunk_rows])
                o, m, r = self.wait(k & 1, n)
            else:
                o, m, r = self.wait(k & 1, n)
            offs.append(o[1:] + np.uint64(base))
            base += int(o[-1])
            rms.append(m)
            recs.append(r)
        return (np.concatenate(offs), np.concatenate(rms) if rms else np.zeros(0, dtype=np.uint8),
                np.concatenate(recs) if recs else np.zeros(0, dtype=EFFECT_RECORD))

    def start_any(self, slot: int, rows, arena) -> int:
        """A chunk of --indels rows: (n, 6) u32 (sequence number, x0, d, m, offset low, offset high) into ``arena`` (bytes),
        where a row's R' then A' stand."""
        a = _u32(rows).reshape(-1, 6)
        b = np.frombuffer(bytes(arena), dtype=np.uint8) if len(arena) else np.zeros(1, dtype=np.uint8)
        check(lib().gffx_hip_effect_run_any_start(self._h, int(slot), _p(a), a.shape[0], b.ctypes.data_as(_ffi.u8p), len(arena)))
        return int(a.shape[0])

    def run_any(self, rows, arena, slot: int = 0):
        return self.wait(slot, self.start_any(slot, rows, arena))

    def run_any_chunked(self, rows, arena, chunk_rows: int):
        """As run_chunked; every chunk is handed the bytes from its first row's offset to its last row's end (the rows' offsets
        ascend), its offsets rebased."""
        a = _u32(rows).reshape(-1, 6).copy()
        off = a[:, 4].astype(np.uint64) | a[:, 5].astype(np.uint64) << np.uint64(32)
        end = off + a[:, 2].astype(np.uint64) + a[:, 3].astype(np.uint64)
        starts = list(range(0, a.shape[0], chunk_rows))

        def begin(k):
            lo, hi = starts[k], min(starts[k] + chunk_rows, a.shape[0])
            b0, b1 = int(off[lo]), int(end[lo:hi].max())
            part = a[lo:hi].copy()
            rel = off[lo:hi] - np.uint64(b0)
            part[:, 4], part[:, 5] = (rel & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rel >> np.uint64(32)).astype(np.uint32)
            self.start_any(k & 1, part, arena[b0:b1])
            return hi - lo

        offs, rms, recs, base = [np.zeros(1, dtype=np.uint64)], [], [], 0
        n = begin(0) if starts else 0
        for k in range(len(starts)):
            n_next = begin(k + 1) if k + 1 < len(starts) else 0
            o, m, r = self.wait(k & 1, n)
            offs.append(o[1:] + np.uint64(base))
            base += int(o[-1])
            rms.append(m)
            recs.append(r)
            n = n_next
        return (np.concatenate(offs), np.concatenate(rms) if rms else np.zeros(0, dtype=np.uint8),
                np.concatenate(recs) if recs else np.zeros(0, dtype=EFFECT_RECORD))

    def stage_ms(self) -> Dict[str, float]:
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(lib().gffx_hip_effect_stage_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"build_ms": a.value, "pairs_ms": b.value, "classify_ms": c.value}

    def stats(self) -> Dict[str, int]:
        kept, grows = C.c_uint64(), C.c_uint64()
        check(lib().gffx_hip_effect_stats(self._h, C.byref(kept), C.byref(grows)))
        arena = C.c_uint64()
        check(lib().gffx_hip_effect_arena_grows(self._h, C.byref(arena)))
        return {"kept": kept.value, "grows": grows.value, "arena_grows": arena.value}
