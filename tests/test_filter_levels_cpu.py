"""The two levels of the window index's coverage filter (engine_index.hip: build_window_filter, build_window_filter_fine) against a
brute-force loop over the roots, on the CPU: `win_index_check filter` (tools/win_index_check.hip, which includes the engine's
builder).  Three seqids -- one without roots, one with a single root that ends on a cell boundary, one with empty intervals --; for
both levels bit x of a seqid is set exactly when a root holds a base of cell x; the fine level's cell never lets a region of width
wmax span more than 31 cells; a fine budget of 0 gives no fine level; a fine level folded into a room it misses by a few bytes still
sets every bit brute force sets."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gffx_amd", "bin", "win_index_check")


def test_filter_levels_equal_brute_force():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN, "filter"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok filter ("), r.stdout[-800:] + r.stderr[-500:]
