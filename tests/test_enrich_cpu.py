"""`gffx enrich` where no GPU is needed: the published vectors of mix64, the definition (tests/_enrich_definition.py) on the
hand-written example, its two invariants and its two ways to count against each other; device/enrich_core.hpp, the code
k_classmap_permute runs, gives the definition's matrices in its host build under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/enrich_check.cpp) at the length and width edges; the command line knows the command, refuses
its usage errors like clap and a bad -g file before it touches a device; without a handle the C-ABI reports an error."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _annotate_definition as ad
import _enrich_definition as ed
from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")
TOOL = os.path.join(ROOT, "gffx_amd", "bin", "enrich_check")


def test_mix64_gives_the_published_vectors():
    for n, want in ed.MIX_VECTORS:
        assert ed.mix64(ed.GOLD * n) == want
    assert ed.key(0, 0) == ed.mix64(0) == 0 and ed.key(5, 1) == ed.mix64(5 + ed.GOLD)
    assert ed.draw(0, 0, 0) == ed.MIX_VECTORS[0][1]  # key(0, 0) = 0, row 0: mix64(GOLD * 1)


def test_the_placement_rule():
    top = ed.MASK
    assert ed.place(top, 100, 7, 7) == (ed.EMPTY, 7) and ed.place(top, 100, 9, 3) == (ed.EMPTY, 9)
    assert ed.place(top, 10, 0, 11) == (ed.UNPLACEABLE, 0) and ed.place(top, 0, 4, 5) == (ed.UNPLACEABLE, 4)
    assert ed.place(top, 10, 3, 13) == (ed.PLACED, 0) and ed.place(0, 10, 3, 13) == (ed.PLACED, 0)  # span 1
    assert ed.place(top, 10, 3, 4) == (ed.PLACED, 9) and ed.place(0, 10, 3, 4) == (ed.PLACED, 0)  # the last start is L - w
    assert ed.place(1 << 63, ed.EDGE_L, 0, 1) == (ed.PLACED, (ed.EDGE_L) >> 1)


def test_the_definition_gives_the_hand_answers():
    for fast in (False, True):
        for seed in (0, 1, 0xDEADBEEFCAFEF00D):
            got = ed.totals(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ed.HAND_LEN, ed.HAND_REGIONS, ed.HAND_N_PERM, seed, fast=fast)
            assert ed.same(got, ed.hand())
    B, R, _ = ed.hand()
    assert ed.perms_text(B, R) == ed.BY_HAND_PERMS and ed.table_matches(ed.BY_HAND_TABLE, ad.LAYER_NAMES, B, R)
    assert not ed.table_matches(ed.BY_HAND_TABLE.replace(b"0.705882", b"0.705892"), ad.LAYER_NAMES, B, R)
    assert not ed.table_matches(ed.BY_HAND_TABLE.replace(b"\t2\t0\t1\t", b"\t2\t1\t1\t", 1), ad.LAYER_NAMES, B, R)


@pytest.mark.parametrize("seed", range(6))
def test_the_invariants_and_the_two_ways_to_count(seed):
    n_seq, T, rows, seq_len, regions = ed.random_case(seed)
    slow = ed.totals(n_seq, T, rows, seq_len, regions, 5, seed * 977)
    assert ed.same(slow, ed.totals(n_seq, T, rows, seq_len, regions, 5, seed * 977, fast=True))
    B, R, unplaced = slow
    width = int(np.where(regions[:, 1] < regions[:, 2], regions[:, 2].astype(np.int64) - regions[:, 1], 0).sum())
    assert np.all(R.sum(1) == len(regions)) and np.all(B.sum(1) == width)
    assert unplaced == int((regions[:, 2].astype(np.int64) - regions[:, 1] > seq_len[regions[:, 0]]).sum()) > 0
    assert not np.array_equal(B[1], B[2])  # the permutations differ from each other
    # any split into runs adds up, given the right first_row
    a = ed.totals(n_seq, T, rows, seq_len, regions[:7], 5, seed * 977)
    b = ed.totals(n_seq, T, rows, seq_len, regions[7:], 5, seed * 977, first_row=7)
    assert ed.same(ed.add(a, b), slow)


def test_the_edge_cases_of_the_definition():
    n_seq, T, rows, seq_len, regions = ed.edge_case()
    slow = ed.totals(n_seq, T, rows, seq_len, regions, 3, 11)
    assert ed.same(slow, ed.totals(n_seq, T, rows, seq_len, regions, 3, 11, fast=True))
    assert slow[2] == 4  # [1, 0, 100], [2, 0, 12346], [3, 0, 1], [3, 0, 7]
    B, R, _ = ed.totals(*ed.big_totals_case(), 2, 3)
    assert B[:, 0].tolist() == [8 << 31] * 3 and B[:, 1].tolist() == [0] * 3 and R[:, 0].tolist() == [8] * 3


def test_a_class_that_covers_everything_takes_every_base():
    n_seq, T, rows, seq_len, regions = ed.random_case(21, T=3)
    rows = np.concatenate([rows, [[0, c, 0, int(seq_len[c])] for c in range(n_seq)]]).astype(np.uint32)
    regions = regions[regions[:, 2].astype(np.int64) - regions[:, 1] <= seq_len[regions[:, 0]]]  # (what stays put may stick out of [0, L))
    regions = regions[regions[:, 2] <= seq_len[regions[:, 0]]]
    B, R, unplaced = ed.totals(n_seq, T, rows, seq_len, regions, 6, 5)
    width = int(np.where(regions[:, 1] < regions[:, 2], regions[:, 2].astype(np.int64) - regions[:, 1], 0).sum())
    assert unplaced == 0 and B[:, 0].tolist() == [width] * 7 and not B[:, 1:].any()


def test_the_statistics():
    s = ed.stats([5, 1, 5, 9])
    assert s[:2] == (5, 5.0) and s[2] == 4.0 and s[3] == 0.0 and s[4] == 1.0 and s[5:] == (2, 2, 0.75, 0.75)
    s = ed.stats([3, 7])
    assert s[1] == 7.0 and math.isnan(s[2]) and math.isnan(s[3]) and s[5:] == (1, 0, 1.0, 0.5)
    big = (1 << 53) - 1  # three times this is no double: one value in every permutation still gives it as the mean, and sd 0
    s = ed.stats([big - 2, big, big, big])
    assert s[1] == float(big) and s[2] == 0.0 and math.isnan(s[3]) and s[5:] == (3, 0, 1.0, 0.25)
    s = ed.stats([3, 0, 0])
    assert s[2] == 0.0 and math.isnan(s[3]) and math.isnan(s[4])


# ---- device/enrich_core.hpp under the sanitizers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gffx_amd", "csrc"), "enrich_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _run_tool(tool, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([tool, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode not in (86, 87), r.stderr[-3000:]
    return r


def _case_text(n_seq, T, rows, seq_len, regions, n_perm, seed, first_row=0):
    p_off, pos, cls, cb = ad.sparse(n_seq, T, rows, np.zeros((0, 3), np.uint32))[:4]
    seq = np.repeat(np.arange(n_seq), np.diff(p_off.astype(np.int64)))
    lines = ["n_seq %d" % n_seq, "layers %d" % T, "perms %d" % n_perm, "seed %d" % seed, "first_row %d" % first_row]
    lines += ["len %d %d" % (c, int(seq_len[c])) for c in range(n_seq)]
    lines += ["p %d %d %d" % (seq[i], pos[i], cls[i]) for i in range(len(pos))]
    lines += ["cb %d %s" % (i, " ".join(str(int(v)) for v in cb[:, i])) for i in range(len(pos))]
    lines += ["q %d %d %d" % tuple(r) for r in np.asarray(regions).reshape(-1, 3).tolist()]
    return "\n".join(lines) + "\n"


def _expected_lines(want, nq):
    B, R, unplaced = want
    out = ["mix " + " ".join("%016X" % v for _, v in ed.MIX_VECTORS)]
    for p in range(len(B)):
        out.append("B %d %s" % (p, " ".join(str(int(v)) for v in B[p])))
        out.append("R %d %s" % (p, " ".join(str(int(v)) for v in R[p])))
    return out + ["unplaced %d" % unplaced, "regions %d perms %d" % (nq, len(B) - 1)]


def _hand_case():
    return ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ed.HAND_LEN, ed.HAND_REGIONS


CORE_CASES = {
    "hand": (_hand_case, 2, 0, 0),
    "hand_no_permutations": (_hand_case, 0, 9, 0),
    "random": (lambda: ed.random_case(31, n=80, nq=120), 7, 0x9E3779B97F4A7C15, 0),
    "random_far_rows": (lambda: ed.random_case(32), 4, (1 << 64) - 1, (1 << 40) + 3),
    "edges": (ed.edge_case, 5, 1, 0),
    "totals_above_32_bits": (ed.big_totals_case, 3, 2, 0),
    "thirty_two_layers": (lambda: ed.random_case(33, T=32, n=200), 3, 4, 0),
}


@pytest.mark.parametrize("name", sorted(CORE_CASES))
def test_the_shared_core_under_the_sanitizers(tool, tmp_path, name):
    case, n_perm, seed, first_row = CORE_CASES[name]
    n_seq, T, rows, seq_len, regions = case()
    path = tmp_path / "case.txt"
    path.write_text(_case_text(n_seq, T, rows, seq_len, regions, n_perm, seed, first_row))
    r = _run_tool(tool, path)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    want = ed.totals(n_seq, T, rows, seq_len, regions, n_perm, seed, first_row)
    if name.startswith("hand"):
        assert ed.same(want, tuple(x[:n_perm + 1] if i < 2 else x for i, x in enumerate(ed.hand())))
    assert r.stdout.split("\n")[:-1] == _expected_lines(want, len(regions))


def test_the_core_refuses_a_seqid_out_of_range(tool, tmp_path):
    path = tmp_path / "case.txt"
    path.write_text(_case_text(ad.HAND_N_SEQ, ad.HAND_T, ad.HAND_ROWS, ed.HAND_LEN, [[0, 1, 2], [2, 0, 5]], 2, 0))
    r = _run_tool(tool, path)
    assert r.returncode == 3 and r.stdout == "range\n"


# ---- the command line ------------------------------------------------------------------------------------------------

def test_enrich_is_in_the_top_usage():
    r = subprocess.run([GFFX, "help"], capture_output=True)
    assert r.returncode == 0 and b"\n  enrich     " in r.stdout and b"\n  annotate   " in r.stdout
    r = subprocess.run([GFFX, "enrich", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--permutations <N>" in r.stdout and b"--genome <FILE>" in r.stdout and b"understates" in r.stdout
    assert b"--region" not in r.stdout


def test_usage_errors_exit_2_like_clap(tmp_path):
    gff, bed = str(tmp_path / "x.gff"), str(tmp_path / "x.bed")
    base = [GFFX, "enrich", "-i", gff, "-b", bed]

    def refused(cmd, what):
        r = subprocess.run(cmd, capture_output=True)
        assert r.returncode == 2 and what in r.stderr and b"Usage: gffx enrich" in r.stderr and r.stdout == b"", r.stderr

    refused(base + ["-n", "10"], b"--types <T1,T2,...>")
    refused(base + ["-T", "CDS"], b"--permutations <N>")
    refused([GFFX, "enrich", "-b", bed, "-T", "CDS", "-n", "10"], b"--input <FILE>")
    refused([GFFX, "enrich", "-i", gff, "-T", "CDS", "-n", "10"], b"--bed <BED>")
    refused(base + ["-T", "CDS,,exon", "-n", "10"], b"an empty type name")
    refused(base + ["-T", "CDS,CDS", "-n", "10"], b"'CDS' is given twice")
    refused(base + ["-T", ",".join("t%d" % i for i in range(33)), "-n", "10"], b"more than 32 types")
    refused(base + ["-T", "CDS", "-n", "0"], b"1 to 1048576 are possible")
    refused(base + ["-T", "CDS", "-n", "1048577"], b"1 to 1048576 are possible")
    refused(base + ["-T", "CDS", "-n", "ten"], b"--permutations <N>")
    refused(base + ["-T", "CDS", "-n", "10", "--seed", "-1"], b"--seed <S>")
    refused(base + ["-T", "CDS", "-n", "10", "--seed", "18446744073709551616"], b"--seed <S>")
    refused(base + ["-T", "CDS", "-n", "10", "--seed", "7x"], b"--seed <S>")
    refused(base + ["-T", "CDS", "-n", "10", "-r", "chr1:1-2"], b"-r")  # -r is not offered
    # the largest values are fine as far as the usage goes: the run then fails on the missing file, not on the usage
    r = subprocess.run(base + ["-T", "CDS", "-n", "1048576", "--seed", "18446744073709551615"], capture_output=True)
    assert r.returncode == 1 and b"Error:" in r.stderr


def test_a_bad_genome_file_ends_the_run_before_the_device(tmp_path):
    gff, bed, genome = str(tmp_path / "hand.gff"), str(tmp_path / "q.bed"), str(tmp_path / "genome.txt")
    open(gff, "w").write(ad.GFF)
    open(bed, "wb").write(ed.BED)
    r = subprocess.run([GFFX, "index", "-i", gff], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    base = [GFFX, "enrich", "-i", gff, "-b", bed, "-T", "CDS,exon,gene", "-n", "2", "-g", genome]

    def fails(text, what):
        open(genome, "wb").write(text)
        r = subprocess.run(base, capture_output=True, timeout=120)
        errors = [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")]
        assert r.returncode == 1 and len(errors) == 1 and what in errors[0] and r.stdout == b"", r.stderr

    fails(b"chrA\t400\n", b"no length for seqid 'chrB'")
    fails(b"chrA\t400\nchrUn\t5\n# chrB\t20\n", b"no length for seqid 'chrB'")
    fails(b"chrA\t400\nchrB 20\n", b"line 2: expected name<TAB>length")
    fails(b"chrA\t400\nchrB\t\n", b"line 2: the length is not a number below 2^32")
    fails(b"chrA\t400\nchrB\t2e1\n", b"line 2: the length is not a number below 2^32")
    fails(b"chrA\t400\n\nchrB\t4294967296\n", b"line 3: the length is not a number below 2^32")
    os.remove(genome)
    r = subprocess.run(base, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Cannot open genome file" in r.stderr


# ---- the ABI without a handle -------------------------------------------------------------------------------------------

def test_a_null_handle_is_reported_not_crashed_on():
    L = _ffi.lib()
    w32, w64, d = np.zeros(8, np.uint32), np.zeros(8, np.uint64), C.c_double()
    rcs = [L.gffx_hip_classmap_perm_begin(None, w32.ctypes.data_as(_ffi.u32p), 3, 0),
           L.gffx_hip_classmap_perm_run_host(None, w32.ctypes.data_as(_ffi.u32p), 1, 0),
           L.gffx_hip_classmap_perm_run_store(None, None, 0, 0, 0, 0),
           L.gffx_hip_classmap_perm_wait(None),
           L.gffx_hip_classmap_perm_copy_totals(None, w64.ctypes.data_as(_ffi.u64p), None, None),
           L.gffx_hip_classmap_perm_last_kernel_ms(None, C.byref(d))]
    assert rcs == [-1] * len(rcs)
    G, block = engine._enrich_constants()
    assert 1 <= G <= 64 and block >= 64
