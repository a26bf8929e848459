"""`gffx closest` where no GPU is needed: the brute-force definition (tests/_closest_definition.py) gives the hand-written
answers on the hand cases; device/closest_core.hpp, the code k_closest_count / k_closest_emit run, gives the definition's
answers in its host build under AddressSanitizer + UndefinedBehaviorSanitizer (tools/closest_check.cpp); the command line knows
the command and refuses its usage errors like clap; without a device or a handle the C-ABI reports an error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _closest_definition as cd
from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "closest_check")


@pytest.mark.parametrize("combo", cd.COMBOS, ids=lambda c: "%s-%s" % ("ignore" if c[0] else "default", c[1]))
def test_the_table_by_hand(combo):
    got = cd.answers(1, cd.TABLE_ROOTS, cd.TABLE_REGIONS, *combo)
    assert [[(cd.TABLE_NAMES[f], d) for f, d in row] for row in got] == cd.TABLE_BY_HAND[combo]


def test_the_other_sentences_of_the_definition():
    # side=right on [220,240): C and D at +61; side=left on [0,50): nothing
    assert cd.answers(1, cd.TABLE_ROOTS, [[0, 220, 240]], False, "right") == [[(2, 61), (3, 61)]]
    assert cd.answers(1, cd.TABLE_ROOTS, [[0, 0, 50]], False, "left") == [[]]
    with pytest.raises(ValueError):
        cd.brute(1, cd.TABLE_ROOTS, [[1, 0, 50]])


@pytest.mark.parametrize("case,combo", sorted(cd.BY_HAND), ids=lambda x: x if isinstance(x, str) else "%s-%s" % ("ignore" if x[0] else "default", x[1]))
def test_the_hand_cases_by_hand(case, combo):
    n_seq, roots, regions = cd.HAND[case]
    assert cd.answers(n_seq, roots, regions, *combo) == cd.BY_HAND[(case, combo)]


def test_ties_come_in_index_position_order_and_gaps_fit_32_bits():
    for name in ("forty_roots_with_one_start", "forty_roots_with_one_end"):
        n_seq, roots, regions = cd.HAND[name]
        for combo in cd.COMBOS:
            counts, offsets, triples, gaps, pos, dist = cd.brute(n_seq, roots, regions, *combo)
            # (41: the forty tied roots on one side and one root as far away on the other; a side that removes the tied
            #  roots' class leaves single answers)
            assert counts.max() >= 40 or combo[1] != "both"
            for i in range(len(counts)):
                p = pos[int(offsets[i]):int(offsets[i + 1])]
                assert np.all(np.diff(p) > 0)
    # a root at [0, 0) seen from the last base: the largest gap there is
    _, _, _, gaps, _, dist = cd.brute(1, [[0, 0, 0]], [[0, cd.U32_MAX - 1, cd.U32_MAX]])
    assert gaps.tolist() == [cd.U32_MAX] and dist.tolist() == [-cd.U32_MAX]
    _, _, _, gaps, _, dist = cd.brute(1, [[0, cd.U32_MAX, cd.U32_MAX]], [[0, 0, 1]])
    assert gaps.tolist() == [cd.U32_MAX] and dist.tolist() == [cd.U32_MAX]


def test_the_end_table_of_the_definition():
    e_end, e_pos = cd.end_table(1, cd.TABLE_ROOTS)
    # positions: A 0, B 1, C 2, D 3; by end: B 160, A 200, D 350, C 400
    assert e_end.tolist() == [160, 200, 350, 400] and e_pos.tolist() == [1, 0, 3, 2]
    n_seq, roots, _ = cd.HAND["forty_roots_with_one_end"]
    e_end, e_pos = cd.end_table(n_seq, roots)
    run = e_pos[e_end == 9000]
    assert len(run) == 40 and np.all(np.diff(run) > 0)  # equal ends keep ascending position


# ---- device/closest_core.hpp under the sanitizers ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "closest_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _vector_text(n_seq, roots, regions):
    lines = ["n_seq %d" % n_seq]
    lines += ["root %d %d %d" % tuple(r) for r in np.asarray(roots).tolist()]
    for combo in cd.COMBOS:
        f = cd.flags_of(*combo)
        lines += ["q %d %d %d %d" % (f, r[0], r[1], r[2]) for r in np.asarray(regions).tolist()]
    return "\n".join(lines) + "\n"


def _expected_lines(n_seq, roots, regions):
    out = []
    for combo in cd.COMBOS:
        counts, offsets, _, gaps, pos, _ = cd.brute(n_seq, roots, regions, *combo)
        for i in range(len(counts)):
            p = pos[int(offsets[i]):int(offsets[i + 1])]
            out.append("a %d %s" % (counts[i], " ".join([str(int(gaps[i]))] + [str(int(x)) for x in p]) if counts[i] else "-"))
    return out


@pytest.mark.parametrize("name", sorted(cd.HAND))
def test_the_shared_core_under_the_sanitizers(tool, tmp_path, name):
    n_seq, roots, regions = cd.HAND[name]
    path = tmp_path / "case.txt"
    path.write_text(_vector_text(n_seq, roots, regions))
    r = _run_tool(tool, path)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    out = r.stdout.split("\n")
    want = _expected_lines(n_seq, roots, regions)
    assert out[len(want)] == "roots %d regions %d" % (len(roots), 6 * len(regions))
    assert out[: len(want)] == want


def test_the_shared_core_on_random_regions(tool, tmp_path):
    n_seq, roots, regions = cd.random_world()
    path = tmp_path / "case.txt"
    path.write_text(_vector_text(n_seq, roots, regions))
    r = _run_tool(tool, path)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    want = _expected_lines(n_seq, roots, regions)
    assert len(want) == 6 * 3000 and r.stdout.split("\n")[: len(want)] == want
    # the set is worth its name: every class of answer occurs
    counts = cd.brute(n_seq, roots, regions)[0]
    assert (counts == 0).sum() == 0 and (counts > 1).sum() > 100


def test_the_core_without_roots_and_its_refusals(tool, tmp_path):
    path = tmp_path / "case.txt"
    path.write_text("n_seq 2\nq 0 0 5 9\nq 1 1 0 4294967295\nq 0 2 1 5\nq 6 0 1 5\nq 8 0 1 5\n")  # zero-length arrays: any read is reported
    r = _run_tool(tool, path)
    assert r.returncode == 0 and r.stdout == "a 0 -\na 0 -\nrange\nflags\nflags\nroots 0 regions 5\n"
    for text in ("n_seq 2\nroot 2 1 5\n", "n_seq 2\nroot 0 5 4\n"):
        path.write_text(text)
        r = _run_tool(tool, path)
        assert r.returncode == 3 and r.stdout == "refused root\n"


# ---- the command line ------------------------------------------------------------------------------------------------

def test_closest_is_in_the_top_usage():
    r = subprocess.run([GFFX, "help"], capture_output=True)
    assert r.returncode == 0 and b"\n  closest    " in r.stdout
    r = subprocess.run([GFFX, "nearest"], capture_output=True)
    assert r.returncode == 2 and b"unrecognized subcommand 'nearest'" in r.stderr and b"closest" in r.stderr


def test_closest_help_says_what_the_coordinates_are():
    r = subprocess.run([GFFX, "closest", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--ignore-overlaps" in r.stdout and b"--side <SIDE>" in r.stdout
    assert b"0-based, half-open" in r.stdout


def test_usage_errors_exit_2_like_clap(tmp_path):
    gff, bed = str(tmp_path / "x.gff"), str(tmp_path / "x.bed")
    r = subprocess.run([GFFX, "closest", "-r", "chr1:1-2"], capture_output=True)
    assert r.returncode == 2 and b"error: the following required arguments were not provided:\n  --input <FILE>" in r.stderr
    r = subprocess.run([GFFX, "closest", "-i", gff, "-b", bed, "-r", "chr1:1-2"], capture_output=True)
    assert r.returncode == 2 and b"error: the argument '--region <REGION>' cannot be used with '--bed <BED>'" in r.stderr
    r = subprocess.run([GFFX, "closest", "-i", gff, "-r", "chr1:1-2", "--side", "up"], capture_output=True)
    assert r.returncode == 2 and b"error: invalid value 'up' for '--side <SIDE>'" in r.stderr and b"[possible values: both, left, right]" in r.stderr
    r = subprocess.run([GFFX, "closest", "-i", gff], capture_output=True)
    assert r.returncode == 2 and b"<--region <REGION>|--bed <BED>>" in r.stderr
    assert b"Usage: gffx closest" in r.stderr and r.stdout == b""


# ---- the ABI without a device ------------------------------------------------------------------------------------------

def test_a_null_handle_and_bad_flags_are_reported_not_crashed_on():
    L = _ffi.lib()
    rows = np.array([[0, 1, 2]], np.uint32)
    out = np.zeros(8, np.uint32)
    out64 = np.zeros(4, np.uint64)
    d = C.c_double()
    rcs = [L.gffx_hip_closest_run_host(None, rows.ctypes.data_as(_ffi.u32p), 1, 0),
           L.gffx_hip_closest_run_store(None, None, 0, 0, 0, 0),
           L.gffx_hip_closest_wait(None),
           L.gffx_hip_closest_total_pairs(None, out64.ctypes.data_as(_ffi.u64p)),
           L.gffx_hip_closest_copy_counts(None, out.ctypes.data_as(_ffi.u32p)),
           L.gffx_hip_closest_copy_offsets(None, out64.ctypes.data_as(_ffi.u64p)),
           L.gffx_hip_closest_copy_triples(None, out.ctypes.data_as(_ffi.u32p)),
           L.gffx_hip_closest_copy_gaps(None, out.ctypes.data_as(_ffi.u32p)),
           L.gffx_hip_closest_copy_end_table(None, None, None),
           L.gffx_hip_closest_last_kernel_ms(None, C.byref(d)),
           L.gffx_hip_closest_last_grid(None, None, None),
           L.gffx_hip_closest_stats(None, None, None)]
    assert rcs == [-1] * len(rcs) and b"closest is NULL" in L.gffx_hip_last_error()
    L.gffx_hip_closest_destroy(None)
    assert L.gffx_hip_closest_create(None, 8, None) == -1
    # the flags' rule is looked at first: both _ONLY bits, an unknown bit
    for bad in (cd.LEFT_ONLY | cd.RIGHT_ONLY, 7, 8, 1 << 31):
        assert L.gffx_hip_closest_run_host(None, rows.ctypes.data_as(_ffi.u32p), 1, bad) == -1
        assert b"bad flags" in L.gffx_hip_last_error()
        assert L.gffx_hip_closest_run_store(None, None, 0, 0, 0, bad) == -1 and b"bad flags" in L.gffx_hip_last_error()
    with pytest.raises(ValueError):
        engine.closest_flags(False, "up")
    assert [engine.closest_flags(*c) for c in cd.COMBOS] == [cd.flags_of(*c) for c in cd.COMBOS] == [0, 2, 4, 1, 3, 5]


def test_the_signed_distances_of_the_python_helper():
    regions = cd.TABLE_REGIONS
    for combo in cd.COMBOS:
        counts, _, triples, gaps, _, dist = cd.brute(1, cd.TABLE_ROOTS, regions, *combo)
        got = engine.closest_distances(regions, counts, triples, gaps)
        assert got.dtype == np.int64 and np.array_equal(got, dist)


@pytest.mark.skipif(engine.device_count() > 0, reason="checks the behaviour of a machine without a GPU")
def test_without_a_gpu_the_handle_cannot_be_created():
    h = C.c_void_p()
    assert _ffi.lib().gffx_hip_closest_create(None, 8, C.byref(h)) == -2 and not h.value
    assert b"no HIP device" in _ffi.lib().gffx_hip_last_error()
