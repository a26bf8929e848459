"""`gffx coverage --thresholds / --bedgraph` where no GPU is needed: the two restatements of the canonical depth profile
(tests/_profile_definition.py: an array over the bases, and a sparse sweep over a dict of deltas) agree with each other, with
answers worked by hand, with the union's definition at depth >= 1 and with the pileup's definition as sum of depth x length;
device/profile_core.hpp, the rules the kernels run, gives the same points, spans and covered bases in its host build under
AddressSanitizer + UndefinedBehaviorSanitizer (tools/profile_check.cpp); the flags are known to the command line and their
usage errors are reported before a device is touched; without a device or a handle the C-ABI reports an error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _coverage_definition as cd
import _pileup_definition as pile
import _profile_definition as pf
from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "profile_check")
SMALL = sorted(n for n in pf.HAND if int(pf.HAND[n][1][:, 2].max()) < 5000)  # the shapes an array over the bases can hold


def _random_rows(seed, n=2500, n_seq=3, span=4000, width=300):
    rng = np.random.default_rng(seed)
    rows = np.empty((n, 3), np.uint32)
    rows[:, 0] = rng.integers(0, n_seq, n)
    rows[:, 1] = rng.integers(0, span, n)
    rows[:, 2] = rows[:, 1] + rng.integers(1, width, n)
    return rows


def _segments(points, n_seq, extra=()):
    """Segments that begin and end on points, inside runs and outside every run, an empty and an inverted one."""
    q, a, b = [], [], []
    p_off, pos, _ = points
    for c in range(n_seq):
        ps = [int(x) for x in pos[int(p_off[c]):int(p_off[c + 1])]]
        for lo, hi in zip(ps, ps[1:]):
            for s, e in ((lo, hi), (lo, min(hi + 3, pf.U32_MAX)), (max(lo - 2, 0), hi), (lo + (hi - lo) // 2, hi), (lo, lo), (hi, lo)):
                q.append(c), a.append(s), b.append(e)
        if ps:
            q.append(c), a.append(0), b.append(pf.U32_MAX)
            q.append(c), a.append(ps[-1]), b.append(min(ps[-1] + 10, pf.U32_MAX))  # behind every run
    for t in extra:
        q.append(t[0]), a.append(t[1]), b.append(t[2])
    return np.array(q, np.uint32), np.array(a, np.uint32), np.array(b, np.uint32)


@pytest.mark.parametrize("name", sorted(pf.HAND))
def test_the_sweep_gives_the_hand_worked_points(name):
    n_seq, rows = pf.HAND[name]
    got = pf.sweep(rows, n_seq)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    if name in pf.BY_HAND:
        assert pf.same(got, pf.hand_points(name))
    if name == "equal_starts":  # 300 equal starts give ONE point up, then 300 single steps down
        assert got[1][0] == 100 and got[2][0] == 300 and len(got[1]) == 301 and got[2][-1] == 0
    if name == "equal_ends":
        assert len(got[1]) == 301 and got[1][-1] == 1000 and got[2][-2] == 300 and got[2][-1] == 0
    # canonical form, whatever the shape
    p_off, pos, dep = got
    for c in range(n_seq):
        p, d = pos[int(p_off[c]):int(p_off[c + 1])].astype(np.int64), dep[int(p_off[c]):int(p_off[c + 1])].astype(np.int64)
        if len(p):
            assert (np.diff(p) > 0).all() and d[0] != 0 and d[-1] == 0 and (np.diff(d) != 0).all()


@pytest.mark.parametrize("name", SMALL)
def test_brute_force_equals_the_sweep_on_the_small_hand_shapes(name):
    n_seq, rows = pf.HAND[name]
    assert pf.same(pf.brute(rows, n_seq), pf.sweep(rows, n_seq))


def test_the_small_hand_shapes_are_most_of_them():
    assert set(pf.HAND) - set(SMALL) == {"full_range", "extremes"}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_definitions_agree_on_random_rows(seed):
    rows = _random_rows(seed)
    a, b = pf.brute(rows, 4), pf.sweep(rows, 4)
    assert pf.same(a, b) and len(a[1]) > 1000
    # ... in any order, and whatever the grouping: the profile is a function of the multiset
    assert pf.same(b, pf.sweep(rows[np.random.default_rng(seed).permutation(len(rows))], 4))
    assert pf.same(b, pf.sweep_np(rows, 4))  # the numpy restatement the GPU tests use for many rows


@pytest.mark.parametrize("name", sorted(pf.HAND))
def test_the_numpy_sweep_equals_the_sweep_on_the_hand_shapes(name):
    n_seq, rows = pf.HAND[name]
    assert pf.same(pf.sweep(rows, n_seq), pf.sweep_np(rows, n_seq))


@pytest.mark.parametrize("name", sorted(pf.HAND) + ["random"])
def test_depth_at_least_one_is_the_union(name):
    n_seq, rows = pf.HAND[name] if name != "random" else (4, _random_rows(7))
    got, want = pf.spans_at_least(pf.sweep(rows, n_seq), 1), cd.merge_rows(rows, n_seq)
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(w).astype(np.uint64))


@pytest.mark.parametrize("name", sorted(pf.HAND) + ["random"])
def test_depth_times_length_is_the_pileup(name):
    n_seq, rows = pf.HAND[name] if name != "random" else (4, _random_rows(8, n=600))
    points = pf.sweep(rows, n_seq)
    q, a, b = _segments(points, n_seq)
    if len(q) > 400:
        keep = np.random.default_rng(0).choice(len(q), 400, replace=False)
        q, a, b = q[keep], a[keep], b[keep]
    assert pf.weighted_bases(points, q, a, b) == [int(x) for x in pile.brute(rows, q, a, b)]


def test_thresholds_and_depth_at_by_hand():
    points = pf.hand_points("nested")  # 10:1 40:2 45:3 50:2 60:1 100:0
    assert [tuple(map(int, x)) for x in zip(*pf.spans_at_least(points, 2)[1:3])] == [(40, 60)]
    assert [tuple(map(int, x)) for x in zip(*pf.spans_at_least(points, 3)[1:3])] == [(45, 50)]
    assert len(pf.spans_at_least(points, 4)[1]) == 0
    q, a, b = np.zeros(4, np.uint32), np.array([0, 42, 50, 60], np.uint32), np.array([200, 47, 50, 40], np.uint32)
    assert pf.covered_at_least(points, 1, q, a, b).tolist() == [90, 5, 0, 0]
    assert pf.covered_at_least(points, 2, q, a, b).tolist() == [20, 5, 0, 0]
    assert pf.covered_at_least(points, 3, q, a, b).tolist() == [5, 2, 0, 0]
    assert [pf.depth_at(points, 0, x) for x in (0, 9, 10, 39, 40, 44, 45, 49, 50, 59, 60, 99, 100, pf.U32_MAX)] == [0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 1, 1, 0, 0]
    points = pf.hand_points("cancelling")  # 0:1 5:2 15:1 20:0
    assert [tuple(map(int, x)) for x in zip(*pf.spans_at_least(points, 1)[1:3])] == [(0, 20)]
    assert [tuple(map(int, x)) for x in zip(*pf.spans_at_least(points, 2)[1:3])] == [(5, 15)]


# ------------------------------------------------------------------------------------------------ the shared core, sanitized
@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "profile_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _case_text(n_seq, rows, thresholds, segs, ats):
    lines = ["n_seq %d" % n_seq]
    lines += ["row %d %d %d" % tuple(r) for r in np.asarray(rows).tolist()]
    lines += ["thr %d" % t for t in thresholds]
    lines += ["seg %d %d %d" % t for t in zip(*(x.tolist() for x in segs))]
    lines += ["at %d %d" % t for t in ats]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("name", sorted(pf.HAND))
def test_the_shared_core_under_the_sanitizers(tool, tmp_path, name):
    n_seq, rows = pf.HAND[name]
    points = pf.sweep(rows, n_seq)
    top = pf.max_depth(points)
    thresholds = sorted({1, 2, top, top + 1})
    q, a, b = _segments(points, n_seq)
    q, a, b = q[:200], a[:200], b[:200]
    ats = [(c, x) for c in range(n_seq) for p in points[1][int(points[0][c]):int(points[0][c + 1])][:40].tolist()
           for x in (max(p - 1, 0), p, min(p + 1, pf.U32_MAX))] + [(0, 0), (n_seq - 1, pf.U32_MAX)]
    path = tmp_path / "case.txt"
    path.write_text(_case_text(n_seq, rows, thresholds, (q, a, b), ats))
    r = _run_tool(tool, path)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    out = r.stdout.split("\n")
    want = ["point %d %d %d" % (c, int(points[1][i]), int(points[2][i])) for c in range(n_seq) for i in range(int(points[0][c]), int(points[0][c + 1]))]
    for T in thresholds:
        u_off, us, ue, _ = pf.spans_at_least(points, T)
        want += ["span %d %d %d %d" % (T, c, int(us[i]), int(ue[i])) for c in range(n_seq) for i in range(int(u_off[c]), int(u_off[c + 1]))]
    for T in thresholds:
        want += ["covered %d %d" % (T, int(x)) for x in pf.covered_at_least(points, T, q, a, b)]
    want += ["depth %d" % pf.depth_at(points, c, x) for c, x in ats]
    want += ["rows %d points %d" % (len(rows), len(points[1])), ""]
    assert out == want


def test_the_core_without_rows_and_its_refusals(tool, tmp_path):
    path = tmp_path / "case.txt"
    path.write_text("n_seq 2\nthr 1\nseg 0 5 9\nat 1 4294967295\n")  # zero-length arrays: any read of them would be reported
    r = _run_tool(tool, path)
    assert r.returncode == 0 and r.stdout == "covered 1 0\ndepth 0\nrows 0 points 0\n"
    for text, what in (("n_seq 2\nrow 2 1 5\n", "row chr"), ("n_seq 2\nrow 0 5 5\n", "row interval"), ("n_seq 2\nrow 0 6 5\n", "row interval"),
                       ("n_seq 2\nseg 2 1 5\n", "seg chr"), ("n_seq 2\nat 2 1\n", "at chr"), ("n_seq 2\nthr 0\n", "thr")):
        path.write_text(text)
        r = _run_tool(tool, path)
        assert r.returncode == 3 and r.stdout == "refused %s\n" % what


# ------------------------------------------------------------------------------------------------ the command line, the C-ABI
def test_coverage_help_lists_the_flags():
    r = subprocess.run([GFFX, "coverage", "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"      --thresholds <T1,T2,...>" in r.stdout and b"      --bedgraph <FILE>" in r.stdout
    assert b"bases_ge1 can exceed breadth" in r.stdout


@pytest.mark.parametrize("value", ["0", "1,1", "x", "", "1,2,3,4,5,6,7,8,9", "1,,2", "4294967296", "-1", "1,0", "3,"])
def test_a_bad_thresholds_list_is_a_usage_error(tmp_path, value):
    # (the files do not exist: the arguments are refused before anything is opened or a device is touched)
    base = [GFFX, "coverage", "-i", str(tmp_path / "x.gff"), "-s", str(tmp_path / "x.bed")]
    for args in (["--thresholds", value], ["--thresholds=" + value]):
        r = subprocess.run(base + args, capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--thresholds" in r.stderr and r.stdout == b"", (args, r.stderr)


def test_a_good_thresholds_list_gets_past_the_parser(tmp_path):
    base = [GFFX, "coverage", "-i", str(tmp_path / "x.gff"), "-s", str(tmp_path / "x.bed")]
    r = subprocess.run(base + ["--thresholds", "1,2,3,4,5,6,7,4294967295", "--bedgraph", str(tmp_path / "o.bg")], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--thresholds" not in r.stderr  # (the GFF does not exist)
    r = subprocess.run(base + ["--thresholds"], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"a value is required for '--thresholds'" in r.stderr


def test_a_null_profile_is_reported_not_crashed_on():
    L = _ffi.lib()
    rows = np.array([[0, 1, 2]], np.uint32)
    off = np.zeros(2, np.uint64)
    h = C.c_void_p()
    rcs = [L.gffx_hip_profile_add_host(None, rows.ctypes.data_as(_ffi.u32p), 1),
           L.gffx_hip_profile_add_store(None, None, 0, 0, 0),
           L.gffx_hip_profile_add_points(None, off.ctypes.data_as(_ffi.u64p), None, None),
           L.gffx_hip_profile_finish(None),
           L.gffx_hip_profile_copy_points(None, None, None, None),
           L.gffx_hip_profile_union_at_least(None, 1, C.byref(h)),
           L.gffx_hip_profile_reset(None),
           L.gffx_hip_profile_stats(None, None, None, None),
           L.gffx_hip_profile_stage_ms(None, None, None, None, None)]
    assert rcs == [-1] * len(rcs) and b"profile is NULL" in L.gffx_hip_last_error() and not h.value
    assert L.gffx_hip_profile_n_points(None) == 0
    L.gffx_hip_profile_destroy(None)
    assert L.gffx_hip_profile_create(0, 3, None) == -1


def test_the_constants_come_from_the_library():
    L = _ffi.lib()
    assert engine.PROFILE_FOLD == L.gffx_hip_profile_fold_rows() and engine.PROFILE_SCAN_TILE == L.gffx_hip_profile_scan_tile()
    assert engine.PROFILE_SCAN_TILE % 256 == 0 and engine.PROFILE_FOLD % engine.PROFILE_SCAN_TILE == 0
    assert 2 * engine.PROFILE_FOLD < 2 ** 30  # one fold's events stay below the device sort's limit


@pytest.mark.skipif(engine.device_count() > 0, reason="checks the behaviour of a machine without a GPU")
def test_without_a_gpu_the_profile_cannot_be_created():
    h = C.c_void_p()
    assert _ffi.lib().gffx_hip_profile_create(0, 3, C.byref(h)) == -2 and not h.value
    with pytest.raises(_ffi.GffxHipError) as ei:
        engine.DepthProfile(3)
    assert ei.value.code == -2
