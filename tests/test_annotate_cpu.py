"""`gffx annotate` where no GPU is needed: the two restatements of the definition (tests/_annotate_definition.py) agree with
each other, with the hand-written example and with the coverage definition, and the restatement over whole arrays that the large
device cases use (sparse_np) agrees with them; device/classmap_core.hpp, the code the kernels of
classmap.hip run, gives the definition's points, running sums and answers in its host build under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/classmap_check.cpp); the command line knows the command and refuses its usage errors like
clap; without a handle the C-ABI reports an error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _annotate_definition as ad
import _coverage_definition as cov
from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "classmap_check")


def test_the_restatements_give_the_hand_answers():
    assert ad.same(ad.dense(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ad.HAND_REGIONS), ad.hand())
    assert ad.same(ad.sparse(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ad.HAND_REGIONS), ad.hand())
    assert ad.expected_text() == ad.BY_HAND_TEXT and ad.expected_summary() == ad.BY_HAND_SUMMARY


@pytest.mark.parametrize("seed", range(40))
def test_the_restatements_agree_on_random_cases(seed):
    n_seq, T, rows, regions = ad.random_case(seed)
    a, b = ad.dense(n_seq, T, rows, regions, size=320), ad.sparse(n_seq, T, rows, regions)
    assert ad.same(a, b)
    assert np.array_equal(a[4].sum(1), np.where(regions[:, 1] < regions[:, 2], regions[:, 2] - regions[:, 1], 0))


def test_rows_are_a_multiset_and_bad_rows_are_refused():
    rows = ad.HAND_ROWS
    want = ad.sparse(2, 3, rows, ad.HAND_REGIONS)
    rng = np.random.default_rng(1)
    assert ad.same(ad.sparse(2, 3, rows[rng.permutation(len(rows))], ad.HAND_REGIONS), want)
    assert ad.same(ad.sparse(2, 3, np.repeat(rows, 2, 0), ad.HAND_REGIONS), want)
    for bad in ([3, 0, 1, 2], [0, 2, 1, 2], [0, 0, 2, 2], [0, 0, 3, 2]):
        with pytest.raises(ValueError):
            ad.sparse(2, 3, [bad], [])
        with pytest.raises(ValueError):
            ad.dense(2, 3, [bad], [])
    with pytest.raises(ValueError):
        ad.sparse(2, 3, rows, [[2, 0, 1]])


@pytest.mark.parametrize("seed", range(10))
def test_the_sparse_restatement_agrees_with_the_coverage_definition(seed):
    n_seq, T, rows, regions = ad.random_case(100 + seed, n=60)
    regions = regions[regions[:, 1] < regions[:, 2]]
    counts = ad.sparse(n_seq, T, rows, regions)[4].astype(np.int64)
    first = cov.merge_rows(rows[rows[:, 0] == 0][:, 1:], n_seq)
    every = cov.merge_rows(rows[:, 1:], n_seq)
    assert np.array_equal(counts[:, 0], cov.covered(first, regions[:, 0], regions[:, 1], regions[:, 2]))
    assert np.array_equal(counts[:, :T].sum(1), cov.covered(every, regions[:, 0], regions[:, 1], regions[:, 2]))


# ---- sparse_np, the restatement over whole arrays that the large device cases are held to, against sparse -------------------

def _np_agrees(n_seq, T, rows, regions=None):
    regions = ad.probe_regions(n_seq, T, rows) if regions is None else regions
    a, b = ad.sparse(n_seq, T, rows, regions), ad.sparse_np(n_seq, T, rows, regions)
    for name, x, y in zip(("p_off", "pos", "cls", "cb", "counts", "class"), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), name
    return a


def test_the_array_restatement_gives_the_hand_answers_and_refuses_what_sparse_refuses():
    assert ad.same(ad.sparse_np(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ad.HAND_REGIONS), ad.hand())
    _np_agrees(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS)
    _np_agrees(3, 4, np.zeros((0, 4), np.uint32), np.array([[0, 5, 25], [2, 0, ad.U32_MAX], [1, 9, 3]], np.uint32))  # no rows
    _np_agrees(3, 2, ad.HAND_ROWS[ad.HAND_ROWS[:, 0] < 2], np.zeros((0, 3), np.uint32))  # no regions; seqid 2 without points
    for bad in ([3, 0, 1, 2], [0, 2, 1, 2], [0, 0, 2, 2], [0, 0, 3, 2]):
        with pytest.raises(ValueError):
            ad.sparse_np(2, 3, [bad], [])
    with pytest.raises(ValueError):
        ad.sparse_np(2, 3, ad.HAND_ROWS, [[2, 0, 1]])


@pytest.mark.parametrize("seed", range(40))
def test_the_array_restatement_agrees_with_sparse_on_random_cases(seed):
    n_seq, T, rows, regions = ad.random_case(seed)
    _np_agrees(n_seq, T, rows, np.concatenate([regions, ad.probe_regions(n_seq, T, rows)]))
    rng = np.random.default_rng(seed)
    _np_agrees(n_seq, T, np.repeat(rows, 2, 0)[rng.permutation(2 * len(rows))], regions)  # a multiset: order and duplicates


def test_the_array_restatement_agrees_with_sparse_on_the_tile_edge_layouts():
    S, _, _ = engine._classmap_constants()
    for n in (2, S - 2, S, S + 2):
        _np_agrees(1, 3, ad.events_case(n, T=3))
    lead = ad.events_case(S - 16, T=32)
    P = 1 << 20
    run = np.array([[k, 0, P, P + 100 + k] for k in range(32)], np.uint32)
    _np_agrees(1, 32, np.concatenate([lead, run]))  # 32 layers toggle at one position
    both = np.array([[k, 0, P - 50, P] for k in range(32)] + [[k, 0, P, P + 50] for k in range(32)], np.uint32)
    assert P not in _np_agrees(1, 32, np.concatenate([lead, both]))[1].tolist()  # a close and an open of every layer at P: no point
    _np_agrees(2, 2, np.concatenate([ad.events_case(S, T=2, seq=0), ad.events_case(S + 2, T=2, seq=1)]))  # a seqid border
    i = np.arange(S - 1, dtype=np.int64)
    inner = np.stack([np.full(S - 1, 1), np.zeros(S - 1, np.int64), 10 + 7 * i, 13 + 7 * i], 1).astype(np.uint32)
    cover = np.array([[0, 0, 0, 1 << 20], [2, 0, 1, 1 << 20]], np.uint32)
    want = _np_agrees(1, 3, np.concatenate([inner, cover]))  # rows that cancel under a mask that is not 0: class 0 all the way
    assert want[1].tolist() == [0, 1 << 20] and want[2].tolist() == [0, 3]


def test_the_array_restatement_at_both_ends_of_32_bits():
    rows = np.array([[1, 0, 0, 1], [0, 0, ad.U32_MAX - 1, ad.U32_MAX], [1, 0, 5, ad.U32_MAX], [0, 1, 0, ad.U32_MAX]], np.uint32)
    want = _np_agrees(3, 2, rows)
    assert want[3].max() >= (1 << 32)
    regions = np.array([[0, 0, ad.U32_MAX], [1, 0, ad.U32_MAX], [1, ad.U32_MAX - 1, ad.U32_MAX], [0, ad.U32_MAX, 0], [2, 0, ad.U32_MAX]], np.uint32)
    assert _np_agrees(3, 2, rows, regions)[4].tolist() == [[1, ad.U32_MAX - 5, 4], [ad.U32_MAX, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, ad.U32_MAX]]


# ---- device/classmap_core.hpp under the sanitizers --------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "classmap_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _case_text(n_seq, T, rows, regions):
    lines = ["n_seq %d" % n_seq, "layers %d" % T]
    lines += ["row %d %d %d %d" % tuple(r) for r in np.asarray(rows).reshape(-1, 4).tolist()]
    lines += ["q %d %d %d" % tuple(r) for r in np.asarray(regions).reshape(-1, 3).tolist()]
    return "\n".join(lines) + "\n"


def _expected_lines(n_seq, T, rows, regions):
    regions = np.asarray(regions, np.uint32).reshape(-1, 3)
    ok = regions[:, 0] < n_seq
    p_off, pos, cls, cb, counts, best = ad.sparse(n_seq, T, rows, regions[ok])
    seq = np.repeat(np.arange(n_seq), np.diff(p_off.astype(np.int64)))
    out = ["p %d %d %d" % (seq[i], pos[i], cls[i]) for i in range(len(pos))]
    out += ["cb %d %s" % (i, " ".join(str(int(v)) for v in cb[:, i])) for i in range(len(pos))]
    it = iter(range(int(ok.sum())))
    for good in ok:
        if not good:
            out.append("range")
            continue
        i = next(it)
        out.append("a %s %s" % (best[i] if best[i] < T else ".", " ".join(str(int(v)) for v in counts[i])))
    out.append("points %d regions %d" % (len(pos), len(regions)))
    return out


def _wide_rows(T):
    """Every layer toggles at position 1000 (a close and an open of one layer at one position among them), coordinates 0 and
    2^32 - 1, a seqid without rows in the middle."""
    rows = [[k, 0, 1000 - 10 * (k + 1), 1000] for k in range(T)] + [[k, 0, 1000, 1000 + 10 * (k + 1)] for k in range(T)]
    rows += [[T - 1, 0, 0, 5], [0, 2, ad.U32_MAX - 7, ad.U32_MAX], [T - 1, 2, 0, ad.U32_MAX], [0, 2, 0, 1]]
    return np.array(rows, np.uint32)


CORE_CASES = {
    "hand": (ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, [[2, 0, 5], [7, 1, 1]]),
    "one_layer": (3, 1, _wide_rows(1), [[3, 0, 1]]),
    "two_layers": (3, 2, _wide_rows(2), []),
    "thirty_two_layers": (3, 32, _wide_rows(32), []),
    "no_rows": (2, 5, np.zeros((0, 4), np.uint32), [[0, 0, 9], [1, 9, 0], [2, 0, 9], [1, 0, ad.U32_MAX]]),
}


@pytest.mark.parametrize("name", sorted(CORE_CASES))
def test_the_shared_core_under_the_sanitizers(tool, tmp_path, name):
    n_seq, T, rows, extra = CORE_CASES[name]
    regions = ad.probe_regions(n_seq, T, rows, extra) if len(rows) else np.array(extra, np.uint32)
    path = tmp_path / "case.txt"
    path.write_text(_case_text(n_seq, T, rows, regions))
    r = _run_tool(tool, path)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    assert r.stdout.split("\n")[:-1] == _expected_lines(n_seq, T, rows, regions)


def test_the_shared_core_on_random_cases(tool, tmp_path):
    for seed in range(12):
        n_seq, T, rows, regions = ad.random_case(200 + seed, n=80)
        regions = np.concatenate([regions, ad.probe_regions(n_seq, T, rows)])
        path = tmp_path / "case.txt"
        path.write_text(_case_text(n_seq, T, rows, regions))
        r = _run_tool(tool, path)
        assert r.returncode == 0 and r.stdout.split("\n")[:-1] == _expected_lines(n_seq, T, rows, regions)


def test_the_core_refuses_bad_rows(tool, tmp_path):
    path = tmp_path / "case.txt"
    for row in ("2 0 1 5", "0 2 1 5", "0 0 5 5", "0 0 6 5"):
        path.write_text("n_seq 2\nlayers 2\nrow %s\n" % row)
        r = _run_tool(tool, path)
        assert r.returncode == 3 and r.stdout == "refused row\n"


# ---- the command line ------------------------------------------------------------------------------------------------

def test_annotate_is_in_the_top_usage():
    r = subprocess.run([GFFX, "help"], capture_output=True)
    assert r.returncode == 0 and b"\n  annotate   " in r.stdout
    r = subprocess.run([GFFX, "annotate", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--types <T1,T2,...>" in r.stdout and b"--summary <FILE>" in r.stdout


def test_usage_errors_exit_2_like_clap(tmp_path):
    gff, bed = str(tmp_path / "x.gff"), str(tmp_path / "x.bed")
    base = [GFFX, "annotate", "-i", gff, "-b", bed]

    def refused(cmd, what):
        r = subprocess.run(cmd, capture_output=True)
        assert r.returncode == 2 and what in r.stderr and b"Usage: gffx annotate" in r.stderr and r.stdout == b"", r.stderr

    refused(base, b"--types <T1,T2,...>")  # -T missing
    refused(base + ["-T", ""], b"an empty type name")
    refused(base + ["-T", "CDS,,exon"], b"an empty type name")
    refused(base + ["-T", "CDS,exon,"], b"an empty type name")
    refused(base + ["-T", "CDS,exon,CDS"], b"'CDS' is given twice")
    refused(base + ["-T", ",".join("t%d" % i for i in range(33))], b"more than 32 types")
    refused([GFFX, "annotate", "-b", bed, "-T", "CDS"], b"--input <FILE>")
    refused([GFFX, "annotate", "-i", gff, "-T", "CDS"], b"<--region <REGION>|--bed <BED>>")
    refused(base + ["-r", "chr1:1-2", "-T", "CDS"], b"cannot be used with")
    # 32 names are fine as far as the usage goes: the run then fails on the missing file, not on the usage
    r = subprocess.run(base + ["-T", ",".join("t%d" % i for i in range(32))], capture_output=True)
    assert r.returncode == 1 and b"Error:" in r.stderr


# ---- the ABI without a handle -------------------------------------------------------------------------------------------

def test_a_null_handle_and_bad_shapes_are_reported_not_crashed_on():
    L = _ffi.lib()
    rows = np.array([[0, 0, 1, 2]], np.uint32)
    out = np.zeros(8, np.uint32)
    out64 = np.zeros(4, np.uint64)
    d = (C.c_double * 6)()
    rcs = [L.gffx_hip_classmap_add_rows_host(None, rows.ctypes.data_as(_ffi.u32p), 1),
           L.gffx_hip_classmap_finish(None),
           L.gffx_hip_classmap_copy_points(None, out64.ctypes.data_as(_ffi.u64p), None, None),
           L.gffx_hip_classmap_copy_bases(None, out64.ctypes.data_as(_ffi.u64p)),
           L.gffx_hip_classmap_run_host(None, out.ctypes.data_as(_ffi.u32p), 1),
           L.gffx_hip_classmap_run_store(None, None, 0, 0, 0),
           L.gffx_hip_classmap_wait(None),
           L.gffx_hip_classmap_copy_counts(None, out.ctypes.data_as(_ffi.u32p)),
           L.gffx_hip_classmap_copy_class(None, None),
           L.gffx_hip_classmap_last_kernel_ms(None, d),
           L.gffx_hip_classmap_stage_ms(None, d)]
    assert rcs == [-1] * len(rcs)
    assert L.gffx_hip_classmap_n_points(None) == 0
    L.gffx_hip_classmap_destroy(None)
    h = C.c_void_p()
    assert L.gffx_hip_classmap_create(0, 4, 0, C.byref(h)) == -1 and not h.value  # the shapes are looked at before the device
    assert L.gffx_hip_classmap_create(0, 4, 33, C.byref(h)) == -1 and not h.value
    assert L.gffx_hip_classmap_create(0, 1 << 28, 32, C.byref(h)) == -1 and b"32 bits" in L.gffx_hip_last_error()
    assert L.gffx_hip_classmap_create(0, 4, 3, None) == -1
    S, B, carry = engine._classmap_constants()
    assert S >= 4 and S % 4 == 0 and B >= 64 and carry >= 64


@pytest.mark.skipif(engine.device_count() > 0, reason="checks the behaviour of a machine without a GPU")
def test_without_a_gpu_the_handle_cannot_be_created():
    h = C.c_void_p()
    assert _ffi.lib().gffx_hip_classmap_create(0, 4, 3, C.byref(h)) == -2 and not h.value
    assert b"no HIP device" in _ffi.lib().gffx_hip_last_error()
