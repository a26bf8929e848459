"""The case builders of tests/test_depth_edges_gpu.py without a GPU: every case's presence checks hold, the rule applied to its
intended hit set and its hand-worked numbers equal the numpy definition, and the hand-written GFF of the CLI case gives the
literal rows through the oracle."""
import numpy as np
import pytest

from oracle import binding as ob

import test_depth_edges_gpu as edges
from _depth_definition import hand_table


def test_a_window_region_overlaps_exactly_the_lines_tagged_with_it():
    rng = np.random.default_rng(1)
    blocks = [[3, 1], [70], [], [1] * 9]
    tags = [[int(rng.integers(-2, 6)) for _ in range(sum(b))] for b in blocks]
    T = hand_table(blocks, tags)
    for b in range(len(blocks)):
        for lo in range(6):
            for hi in range(lo, 6):
                assert T.lines_hit(b, T.window(b, lo, hi)) == [k for k, t in enumerate(tags[b]) if lo <= t <= hi]
        assert T.lines_hit(b, T.whole(b)) == list(range(sum(blocks[b]))) and T.lines_hit(b, T.quiet(b)) == []
        assert T.roots_hit(T.quiet(b)) == [b] and T.roots_hit(T.gap(b)) == []
    assert len(np.unique(T.ls)) > len(T.ls) // 2 and len(np.unique(T.le - T.ls)) > 10  # lines differ in start and length


def test_the_family_of_run_and_chunk_edges():
    T = edges.family_table()
    assert (len(T.roots["fid"]), len(T.ls), T.n_groups) == (12, 975, 277)
    for b, name in edges.FAMILY:
        edges.case_family_one(T, b, name)
    for order in (1, -1):
        c = edges.case_family_all(T, order)
        assert int(c.want[0].sum()) > 300
    assert {name for _, name in edges.FAMILY} == {"first", "last", "line63", "line64", "lines63+64", "third_chunk",
                                                  "chunks_one_and_three", "every", "none"}


@pytest.mark.parametrize("case", [edges.case_named_literals, edges.case_lines_that_touch_the_region,
                                  edges.case_extent_over_the_overlapped_lines_only, edges.case_pair_step, edges.case_state])
def test_the_small_cases_and_their_literals(case):
    case()


def test_pairing_nq_and_pass_shape_cases():
    T = edges.pairing_table()
    for name in edges.PAIRINGS:
        edges.case_pairing(T, name)
    F = edges.family_table()
    for nq in edges.NQS:
        for late in (False, True):
            edges.case_nq(F, nq, late)
    edges.shapes_world()
    edges.capacity_world()


def test_the_hand_written_gff_through_the_oracle(tmp_path):
    gff, bed, n_rows = edges.write_cli_inputs(str(tmp_path))
    ob.build_index(gff)
    out = str(tmp_path / "want.tsv")
    rc, msg = ob.depth_run(gff, bed, out)
    assert rc == 0, msg
    rows = edges._tsv_rows(open(out, "rb").read())
    for row in (edges.CDS_ROW, edges.SHARED_ROW, edges.OUT_ROW):
        assert row in rows, rows[:5]
    assert len(rows) == 1 + 1 + 1 + 1 + 1 + 1 + 1 + 3  # cdsA, geneA, mA, shared, geneB, mB, out, exB63 .. exB65
