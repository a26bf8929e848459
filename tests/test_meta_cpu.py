"""`gffx meta` where no GPU is needed: the definition (tests/_meta_definition.py) twice against itself, on the hand-written
example, under its mirror law and its row-sum law; device/meta_core.hpp with pileup_core.hpp, evaluated the way k_pileup_meta
does, gives the definition's numbers in its host build under AddressSanitizer + UndefinedBehaviorSanitizer
(tools/meta_check.cpp) at the length, flank, clamp and 32-bit edges; the strand / ID helper on a hand-written GFF; the command
line knows the command and refuses its usage errors like clap; without a handle the C-ABI reports an error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _meta_definition as md
import _pileup_definition as pd
from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "meta_check")

LAYOUTS = [md.point(4, 4, 2), md.point(6, 0, 3, md.TES), md.point(0, 8, 4, md.CENTER), md.point(10, 5, 5, md.CENTER), md.scaled(4, 4, 2, 3),
           md.scaled(0, 0, 1, 5), md.scaled(6, 0, 3, 1), md.scaled(0, 6, 2, 7)]


# ---- definition against definition ------------------------------------------------------------------------------------

def test_the_layouts_and_their_offsets():
    assert [md.columns(y) for y in LAYOUTS] == [4, 2, 2, 3, 7, 5, 3, 10]
    for bad in [md.point(4, 4, 0), md.point(5, 4, 2), md.point(4, 5, 2), md.point(0, 0, 2), md.scaled(4, 4, 2, 0), md.point(4, 4, 2, 3), (2, 0, 4, 4, 2, 1)]:
        assert md.columns(bad) == 0
    assert md.offsets(md.point(4, 4, 2, md.CENTER), 7) == [-1, 1, 3, 5, 7]  # a0 = 7 // 2
    assert md.offsets(md.point(4, 2, 2, md.TES), 7) == [3, 5, 7, 9]
    assert md.offsets(md.scaled(2, 2, 2, 4), 2) == [-2, 0, 0, 1, 1, 2, 4]  # L < M: body columns of length 0
    assert md.offsets(md.scaled(0, 0, 1, 2), 2 ** 32 - 2) == [0, 2 ** 31 - 1, 2 ** 32 - 2]
    # a minus feature's tss column starts at its last base and runs downwards; its center is the plus one's mirror image
    assert md.bounds(md.point(0, 2, 1), 20, 27, True) == [(26, 27), (25, 26)]
    assert md.bounds(md.point(0, 1, 1, md.CENTER), 20, 27, False) == [(23, 24)] and md.bounds(md.point(0, 1, 1, md.CENTER), 20, 27, True) == [(23, 24)]
    assert md.bounds(md.point(0, 1, 1, md.CENTER), 20, 26, False) == [(23, 24)] and md.bounds(md.point(0, 1, 1, md.CENTER), 20, 26, True) == [(22, 23)]


@pytest.mark.parametrize("name", sorted(md.HAND))
def test_the_definition_gives_the_hand_answers(name):
    lay, seq_len, bases, width, col_bases, col_len, col_features = md.HAND[name]
    for way in (md.dense, md.sparse):
        got = way(md.HAND_N_SEQ, md.HAND_ROWS, md.HAND_FEATS, lay, seq_len)
        assert got.dtype == np.uint64 and got.tolist() == bases
    w = md.lens(md.HAND_FEATS, lay, seq_len)
    assert w.tolist() == width
    cb, cl, cf = md.totals(np.array(bases, np.uint64), w)
    assert (cb.tolist(), cl.tolist(), cf.tolist()) == (col_bases, col_len, col_features)
    if name == "point":
        assert md.summary_text(lay, cb, cl, cf) == md.HAND_POINT_SUMMARY
    if name == "scaled":
        assert md.summary_text(lay, cb, cl, cf) == md.HAND_SCALED_SUMMARY


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("lo", [100, 0])
def test_the_two_restatements_agree(seed, lo):
    n_seq, rows, feats = md.random_case(seed, lo=lo)
    for k, lay in enumerate(LAYOUTS):
        seq_len = [450, 300] if (seed + k) % 3 == 0 else None
        assert np.array_equal(md.dense(n_seq, rows, feats, lay, seq_len), md.sparse(n_seq, rows, feats, lay, seq_len)), (lay, seq_len)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("lo", [100, 0])
def test_the_mirror_law(seed, lo):
    """Every coordinate x -> C - x and every strand flipped: the matrices are equal.  lo = 100: no clamp in reach; lo = 0: the
    clamp at 0 cuts windows, and its mirror image is a seqid C long."""
    n_seq, rows, feats = md.random_case(10 + seed, lo=lo)
    C_ = 1000
    m_rows, m_feats = md.mirror(rows, feats, C_)
    clamped = 0
    for lay in LAYOUTS:
        a = md.sparse(n_seq, rows, feats, lay)
        b = md.sparse(n_seq, m_rows, m_feats, lay, [C_] * n_seq)
        assert np.array_equal(a, b) and np.array_equal(md.lens(feats, lay), md.lens(m_feats, lay, [C_] * n_seq))
        assert np.array_equal(b, md.dense(n_seq, m_rows, m_feats, lay, [C_] * n_seq))
        clamped += int((md.lens(feats, lay) < np.diff(np.array([md.offsets(lay, int(e - s)) for _, s, e, _ in feats]), axis=1)).sum())
    assert (clamped > 0) == (lo == 0)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("lo", [100, 0])
def test_the_row_sum_law(seed, lo):
    """sum_j bases[i][j] = the pileup's bases on the feature's whole clamped window."""
    n_seq, rows, feats = md.random_case(20 + seed, lo=lo)
    for lay in LAYOUTS:
        q, a, b = [], [], []
        for c, s, e, minus in feats.tolist():
            cols = md.bounds(lay, s, e, minus)
            q.append(c), a.append(min(x for x, _ in cols)), b.append(max(y for _, y in cols))
        assert np.array_equal(md.sparse(n_seq, rows, feats, lay).sum(1, dtype=np.uint64), pd.brute(rows, q, a, b))


# ---- device/meta_core.hpp under the sanitizers ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "meta_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _case_text(n_seq, rows, feats, lay, seq_len):
    lines = ["n_seq %d" % n_seq, "layout %d %d %d %d %d %d" % tuple(lay)]
    lines += ["len %d %d" % (c, v) for c, v in enumerate(seq_len or [])]
    lines += ["row %d %d %d" % tuple(r) for r in np.asarray(rows).reshape(-1, 3).tolist()]
    lines += ["feat %d %d %d %d" % tuple(f) for f in np.asarray(feats).reshape(-1, 4).tolist()]
    return "\n".join(lines) + "\n"


def _expected_lines(n_seq, rows, feats, lay, seq_len):
    bases, width = md.sparse(n_seq, rows, feats, lay, seq_len), md.lens(feats, lay, seq_len)
    out = []
    for i in range(len(bases)):
        out.append("bases " + " ".join(str(int(v)) for v in bases[i]))
        out.append("len " + " ".join(str(int(v)) for v in width[i]))
    for name, v in zip(("col_bases", "col_len", "col_features"), md.totals(bases, width)):
        out.append(name + " " + " ".join(str(int(x)) for x in v))
    return out + ["rows %d feats %d columns %d" % (len(np.asarray(rows).reshape(-1, 3)), len(bases), md.columns(lay))]


def _both_strands(feats):
    return [tuple(f) + (m,) for f in feats for m in (0, 1)]


BIG = md.U32_MAX
_ROWS_SMALL = [(0, 0, 3), (0, 2, 9), (0, 5, 6), (0, 5, 40), (0, 38, 60), (0, 55, 56), (0, 90, 120), (1, 1, 2)]
_ROWS_BIG = [(0, BIG - 50, BIG), (0, BIG - 9, BIG - 1), (0, BIG - 1, BIG), (0, 0, BIG), (0, BIG - 2000, BIG - 30), (0, 2 ** 31, 2 ** 31 + 5)]
# name -> (n_seq, rows, features without strand (both are run), layout, seq_len)
CORE_CASES = {
    "hand_point": (1, md.HAND_ROWS, [(0, 10, 16), (0, 20, 27)], md.HAND_POINT, None),
    "hand_scaled_len_30": (1, md.HAND_ROWS, [(0, 10, 16), (0, 20, 27)], md.HAND_SCALED, [30]),
    "length_1": (2, _ROWS_SMALL, [(0, 5, 6), (0, 39, 40), (1, 1, 2)], md.scaled(4, 4, 2, 3), None),
    "length_below_m": (2, _ROWS_SMALL, [(0, 5, 8), (0, 38, 42)], md.scaled(2, 2, 1, 7), None),
    "length_equals_m": (2, _ROWS_SMALL, [(0, 5, 12), (0, 38, 45)], md.scaled(2, 2, 1, 7), None),
    "up_0": (2, _ROWS_SMALL, [(0, 5, 12), (0, 38, 56)], md.point(0, 12, 3), None),
    "down_0": (2, _ROWS_SMALL, [(0, 5, 12), (0, 38, 56)], md.point(12, 0, 4, md.TES), None),
    "up_0_down_0_scaled": (2, _ROWS_SMALL, [(0, 5, 12), (0, 38, 56), (1, 0, 9)], md.scaled(0, 0, 5, 4), None),
    "center": (2, _ROWS_SMALL, [(0, 5, 12), (0, 38, 56), (0, 90, 91)], md.point(6, 6, 2, md.CENTER), None),
    "window_crosses_0": (2, _ROWS_SMALL, [(0, 1, 4), (0, 0, 9), (0, 5, 7)], md.point(10, 10, 2), None),
    "window_crosses_0_scaled": (2, _ROWS_SMALL, [(0, 1, 4), (0, 0, 9)], md.scaled(6, 6, 3, 2), None),
    "window_crosses_len": (2, _ROWS_SMALL, [(0, 50, 58), (0, 57, 60), (0, 30, 59), (1, 0, 2)], md.point(8, 8, 2), [60, 2]),
    "window_crosses_len_scaled": (2, _ROWS_SMALL, [(0, 50, 58), (0, 57, 60)], md.scaled(8, 8, 4, 3), [60, 2]),
    "feature_beyond_len": (2, _ROWS_SMALL, [(0, 50, 70), (0, 65, 80)], md.scaled(4, 4, 2, 3), [60, 2]),
    "end_at_u32_max": (1, _ROWS_BIG, [(0, BIG - 40, BIG), (0, BIG - 1, BIG), (0, 0, BIG)], md.point(100, 100, 10), None),
    "end_at_u32_max_tes": (1, _ROWS_BIG, [(0, BIG - 40, BIG), (0, BIG - 1, BIG)], md.point(100, 100, 10, md.TES), None),
    "end_at_u32_max_scaled": (1, _ROWS_BIG, [(0, BIG - 40, BIG), (0, 0, BIG)], md.scaled(20, 20, 10, 6), None),
    "j_times_l_beyond_32_bits": (1, _ROWS_BIG, [(0, 0, BIG), (0, 7, BIG - 1), (0, 2 ** 31 - 3, BIG)], md.scaled(0, 0, 1, 1000), None),
    "m_4096": (1, _ROWS_BIG, [(0, 0, BIG), (0, BIG - 3000, BIG - 10)], md.scaled(0, 0, 1, 4096), None),
    "seqid_without_rows": (3, _ROWS_SMALL, [(2, 5, 12), (0, 5, 12), (1, 0, 3)], md.point(4, 4, 2), None),
}


@pytest.mark.parametrize("name", sorted(CORE_CASES))
def test_the_shared_core_under_the_sanitizers(tool, tmp_path, name):
    n_seq, rows, feats, lay, seq_len = CORE_CASES[name]
    feats = _both_strands(feats)
    path = tmp_path / "case.txt"
    path.write_text(_case_text(n_seq, rows, feats, lay, seq_len))
    r = _run_tool(tool, [path])
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    want = _expected_lines(n_seq, rows, feats, lay, seq_len)
    assert r.stdout.split("\n")[:-1] == want
    if name.startswith("window_crosses") or name.startswith("end_at") or name == "feature_beyond_len":  # the clamp did cut something
        full = np.diff(np.array([md.offsets(lay, e - s) for _, s, e, _ in feats]), axis=1)
        assert (md.lens(feats, lay, seq_len).astype(np.int64) < full).any()
    if name == "length_below_m":
        assert (md.lens(feats, lay, seq_len)[:, 2:9] == 0).any()


@pytest.mark.parametrize("seed", range(3))
def test_the_core_on_random_cases(tool, tmp_path, seed):
    n_seq, rows, feats = md.random_case(40 + seed, n_rows=200, n_feat=30, lo=0 if seed else 100)
    for k, lay in enumerate(LAYOUTS):
        seq_len = [430, 470] if k % 2 else None
        path = tmp_path / ("case%d.txt" % k)
        path.write_text(_case_text(n_seq, rows, feats, lay, seq_len))
        r = _run_tool(tool, [path])
        assert r.returncode == 0 and r.stdout.split("\n")[:-1] == _expected_lines(n_seq, rows, feats, lay, seq_len), lay


def test_the_core_refuses_what_the_engine_refuses(tool, tmp_path):
    path = tmp_path / "case.txt"
    for lay, rows, feats, want in [(md.point(4, 4, 0), [], [(0, 1, 2, 0)], "refused layout\n"), (md.point(4, 3, 2), [], [(0, 1, 2, 0)], "refused layout\n"),
                                   (md.point(0, 0, 2), [], [], "refused layout\n"), (md.scaled(2, 2, 2, 0), [], [], "refused layout\n"),
                                   (md.point(4, 4, 2), [(0, 1, 2)], [(1, 1, 2, 0)], "refused feat\n"), (md.point(4, 4, 2), [], [(0, 2, 2, 1)], "refused feat\n"),
                                   (md.point(4, 4, 2), [(0, 3, 2)], [], "refused row\n")]:
        path.write_text(_case_text(1, rows, feats, lay, None))
        r = _run_tool(tool, [path])
        assert r.returncode == 3 and r.stdout == want, (lay, r.stdout)


# ---- the strand and the ID of a line ---------------------------------------------------------------------------------------

STRAND_GFF = (b"##gff-version 3\n"
              b"chrA\tt\tgene\t11\t16\t.\t+\t.\tID=gP;gene_name=P\n"
              b"chrA\tt\tgene\t21\t27\t.\t-\t.\tgene_name=Q;ID=gQ\r\n"
              b"\n"
              b"# a comment\n"
              b"chrA\tt\tgene\t31\t40\t.\t.\t.\tID=gDot\n"
              b"chrA\tt\tgene\t41\t50\t.\t?\t.\tName=none\r\n"
              b"chrA\tt\tgene\t51\t60\t.\t-\t.\tID=;Name=empty\n"
              b"chrA\tt\tgene\t61\t70\t.\t+-\t.\tID=odd strand;x=1\n"
              b"chrA\tt\tgene\t71\t80\t.\t-\n"
              b"chrA\tt\tgene\t81\t85\t.\t+\t.\tgeneID=no;Parent_ID=neither;ID=yes;xID=nor\n"
              b"chrA\tt\tgene\t86\t88\t.\t+\t.\tgeneID=only\n"
              b"chrA\tt\tgene\t81\t90\t.\t-\t.\tID=last")


def test_the_strand_and_id_helper(tool, tmp_path):
    path = tmp_path / "s.gff"
    path.write_bytes(STRAND_GFF)
    r = _run_tool(tool, ["--strand-id", path])
    assert r.returncode == 0
    assert r.stdout.split("\n")[:-1] == ["+ 1 gP", "- 1 gQ", "+ 0 gDot", "+ 0 .", "- 1 .", "+ 0 odd strand", "- 1 .", "+ 1 yes", "+ 1 .", "- 1 last"]


# ---- the command line ------------------------------------------------------------------------------------------------

def test_meta_is_in_the_top_usage():
    r = subprocess.run([GFFX, "help"], capture_output=True)
    assert r.returncode == 0 and b"\n  meta       " in r.stdout and b"\n  enrich     " in r.stdout
    r = subprocess.run([GFFX, "meta", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--anchor <ANCHOR>" in r.stdout and b"--scale <M>" in r.stdout and b"--matrix <FILE>" in r.stdout


def test_usage_errors_exit_2_like_clap(tmp_path):
    gff, bed = str(tmp_path / "x.gff"), str(tmp_path / "x.bed")
    base = [GFFX, "meta", "-i", gff, "-s", bed]
    cap = engine.meta_constants()[0]

    def refused(cmd, what):
        r = subprocess.run(cmd, capture_output=True)
        assert r.returncode == 2 and what in r.stderr and b"Usage: gffx meta" in r.stderr and r.stdout == b"", r.stderr

    refused(base + ["--anchor", "tes", "--scale", "10"], b"'--anchor <ANCHOR>' cannot be used with '--scale <M>'")
    refused(base + ["-w", "0"], b"--bin <BIN>")
    refused(base + ["-u", "2005"], b"--upstream <UP>")
    refused(base + ["-d", "15", "-u", "20"], b"--downstream <DOWN>")
    refused(base + ["-u", "0", "-d", "0"], b"there is no column")
    refused(base + ["--scale", "0"], b"--scale <M>")
    refused(base + ["-u", str(10 * cap), "-d", "10"], b"columns exceed the limit of %d" % cap)
    refused(base + ["-u", "0", "-d", "0", "--scale", str(cap + 1)], b"columns exceed the limit of %d" % cap)
    refused([GFFX, "meta", "-i", gff], b"--source <SOURCE>")
    refused([GFFX, "meta", "-s", bed], b"--input <FILE>")
    refused(base + ["--anchor", "middle"], b"possible values: tss, tes, center")
    refused(base + ["-T", "gene,,mRNA"], b"an empty type name")
    refused(base + ["-w", "ten"], b"--bin <BIN>")
    # the limits themselves are fine as far as the usage goes: the run then fails on the missing file, not on the usage
    for ok in (["-u", str(10 * cap - 10), "-d", "10"], ["-u", "0", "-d", "0", "--scale", str(cap)], ["-u", "0", "-d", "7", "-w", "7", "--anchor", "center"]):
        r = subprocess.run(base + ok, capture_output=True)
        assert r.returncode == 1 and b"Error:" in r.stderr, r.stderr


# ---- the ABI without a handle -------------------------------------------------------------------------------------------

def test_a_null_handle_is_reported_not_crashed_on():
    L = _ffi.lib()
    w32, w64, w8, d = np.zeros(8, np.uint32), np.zeros(8, np.uint64), np.zeros(8, np.uint8), C.c_double()
    lay = engine.MetaLayout.point(4, 4, 2)
    p32, p64 = w32.ctypes.data_as(_ffi.u32p), w64.ctypes.data_as(_ffi.u64p)
    rcs = [L.gffx_hip_pileup_meta_set(None, 1, p32, p32, p32, w8.ctypes.data_as(_ffi.u8p), None, C.byref(lay), 0),
           L.gffx_hip_pileup_meta_copy(None, p64, p64, p64, None),
           L.gffx_hip_pileup_meta_ms(None, C.byref(d))]
    assert rcs == [-1] * len(rcs) and b"pileup is NULL" in L.gffx_hip_last_error()
    assert L.gffx_hip_pileup_meta_columns(None) == 0
    cap, tile = engine.meta_constants()
    assert cap >= 400 and tile >= 1


def test_the_layouts_columns_match_the_definition():
    for lay in LAYOUTS + [md.point(4, 4, 0), md.point(5, 4, 2), md.point(0, 0, 2), md.scaled(4, 4, 2, 0), md.point(4, 4, 2, 3), (2, 0, 4, 4, 2, 1),
                          md.scaled(BIG - 1, BIG - 1, 1, BIG)]:
        assert engine.MetaLayout(*lay).columns == md.columns(lay), lay
