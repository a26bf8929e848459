"""`gffx coverage --mean-depth` where no GPU is needed: the two restatements of the quantity (tests/_pileup_definition.py: the
brute-force sum and the closed form over sorted keys and prefix sums) agree on the hand shapes; device/pileup_core.hpp, the
code k_pileup_segments runs, gives the same numbers in its host build under AddressSanitizer + UndefinedBehaviorSanitizer
(tools/pileup_check.cpp); the flag is known to the command line; without a device or a handle the C-ABI reports an error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _pileup_definition as pd
from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "pileup_check")

# what the hand shapes must give, worked by hand for the small ones (the rest: the brute-force sum)
BY_HAND = {
    "touching": [10, 10, 10, 10, 2, 0, 1, 1],
    "three_full": [3 * (2 ** 32 - 1), 3],
    "seqid_without_rows": [0, 0, 9, 46, 0],
    "empty_and_inverted_segments": [0, 0, 0, 40, 90],
}


@pytest.mark.parametrize("name", sorted(pd.HAND))
def test_brute_force_equals_the_closed_form(name):
    n_seq, rows, (q, a, b) = pd.HAND[name]
    want = pd.brute(rows, q, a, b)
    assert want.dtype == np.uint64 and np.array_equal(want, pd.closed_form(rows, q, a, b))
    if name in BY_HAND:
        assert want.tolist() == BY_HAND[name]
    assert int(rows[:, 0].max()) < n_seq and int(q.max()) < n_seq


def test_the_definitions_agree_on_random_rows():
    rng = np.random.default_rng(3)
    rows = np.empty((3000, 3), np.uint32)
    rows[:, 0] = rng.integers(0, 3, 3000)
    rows[:, 1] = rng.integers(0, 5000, 3000)
    rows[:, 2] = rows[:, 1] + rng.integers(1, 400, 3000)
    q = rng.integers(0, 4, 500).astype(np.uint32)
    a = rng.integers(0, 5500, 500).astype(np.uint32)
    b = (a + rng.integers(0, 900, 500)).astype(np.uint32)
    assert np.array_equal(pd.brute(rows, q, a, b), pd.closed_form(rows, q, a, b))


@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "pileup_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _case_text(n_seq, rows, q, a, b):
    lines = ["n_seq %d" % n_seq]
    lines += ["row %d %d %d" % tuple(r) for r in np.asarray(rows).tolist()]
    lines += ["seg %d %d %d" % t for t in zip(q.tolist(), a.tolist(), b.tolist())]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("name", sorted(pd.HAND))
def test_the_shared_core_under_the_sanitizers(tool, tmp_path, name):
    n_seq, rows, (q, a, b) = pd.HAND[name]
    path = tmp_path / "case.txt"
    path.write_text(_case_text(n_seq, rows, q, a, b))
    r = _run_tool(tool, path)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    assert out[len(q)] == "rows %d segs %d" % (len(rows), len(q))
    assert [int(x.split()[1]) for x in out[: len(q)]] == pd.brute(rows, q, a, b).tolist()


def test_the_core_without_rows_and_its_refusals(tool, tmp_path):
    path = tmp_path / "case.txt"
    path.write_text("n_seq 2\nseg 0 5 9\nseg 1 0 4294967295\n")  # zero-length key arrays: any read of them would be reported
    r = _run_tool(tool, path)
    assert r.returncode == 0 and r.stdout == "bases 0\nbases 0\nrows 0 segs 2\n"
    for text, what in (("n_seq 2\nrow 2 1 5\n", "row chr"), ("n_seq 2\nrow 0 5 5\n", "row interval"), ("n_seq 2\nseg 2 1 5\n", "seg chr")):
        path.write_text(text)
        r = _run_tool(tool, path)
        assert r.returncode == 3 and r.stdout == "refused %s\n" % what


def test_coverage_help_lists_mean_depth():
    r = subprocess.run([GFFX, "coverage", "--help"], capture_output=True)
    assert r.returncode == 0 and b"      --mean-depth " in r.stdout and b"-m," not in r.stdout  # long-only


def test_mean_depth_takes_no_value(tmp_path):
    base = [GFFX, "coverage", "-i", str(tmp_path / "x.gff"), "-s", str(tmp_path / "x.bed")]
    r = subprocess.run(base + ["--mean-depth=1"], capture_output=True)
    assert r.returncode == 2 and b"unexpected value for '--mean-depth'" in r.stderr
    r = subprocess.run(base + ["--mean-depth", "1"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument '1' found" in r.stderr


def test_a_null_pileup_is_reported_not_crashed_on():
    L = _ffi.lib()
    rows = np.array([[0, 1, 2]], np.uint32)
    out = np.zeros(4, np.uint64)
    rcs = [L.gffx_hip_pileup_add_host(None, rows.ctypes.data_as(_ffi.u32p), 1),
           L.gffx_hip_pileup_add_store(None, None, 0, 0, 0),
           L.gffx_hip_pileup_copy(None, out.ctypes.data_as(_ffi.u64p)),
           L.gffx_hip_pileup_reset(None),
           L.gffx_hip_pileup_stats(None, None, None, None),
           L.gffx_hip_pileup_stage_ms(None, None, None, None, None)]
    assert rcs == [-1] * len(rcs) and b"pileup is NULL" in L.gffx_hip_last_error()
    L.gffx_hip_pileup_destroy(None)
    assert L.gffx_hip_pileup_create(0, 3, 0, None, None, None, None) == -1
    # bad segments are refused before a device is looked for
    h = C.c_void_p()
    q = np.array([0, 3], np.uint32)
    z = np.zeros(2, np.uint32)
    p = lambda x: x.ctypes.data_as(_ffi.u32p)  # noqa: E731
    assert L.gffx_hip_pileup_create(0, 3, 2, p(q), p(z), p(z), C.byref(h)) == -1 and not h.value
    assert b"segment 1 has chr 3 >= 3" in L.gffx_hip_last_error()
    assert L.gffx_hip_pileup_create(0, 3, 2, None, p(z), p(z), C.byref(h)) == -1 and not h.value


def test_the_constants_come_from_the_library():
    L = _ffi.lib()
    assert engine.PILEUP_FOLD == L.gffx_hip_pileup_fold_rows() and engine.PILEUP_SCAN_TILE == L.gffx_hip_pileup_scan_tile()
    assert engine.PILEUP_SCAN_TILE % 256 == 0 and engine.PILEUP_FOLD % engine.PILEUP_SCAN_TILE == 0
    assert engine.PILEUP_FOLD < 2 ** 28  # one fold's sums stay below 2^28 rows x 2^32


@pytest.mark.skipif(engine.device_count() > 0, reason="checks the behaviour of a machine without a GPU")
def test_without_a_gpu_the_pileup_cannot_be_created():
    h = C.c_void_p()
    assert _ffi.lib().gffx_hip_pileup_create(0, 3, 0, None, None, None, C.byref(h)) == -2 and not h.value
    with pytest.raises(_ffi.GffxHipError) as ei:
        engine.Pileup(3, [0], [1], [9])
    assert ei.value.code == -2
