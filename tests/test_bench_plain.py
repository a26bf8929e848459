"""bench.py without --full: the run times the headline and prints its line, and none of the legs that take runs of their own."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_LEGS = ("roofline", "group_launch", "serial", "roofline_10m", "roofline_10m_contained", "roofline_cold", "wide_regions",
             "wide_regions_contained", "mixed_widths", "sorted_bed", "cli_pass", "t_xfer", "t_e2e", "join_b", "depth", "cpu_baseline")


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse_args()
    assert not a.full and (a.gpus, a.steps, a.warmup) == (1, 3, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--full", "--quick"])
    a = bench.parse_args()
    assert a.full and a.quick


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--repeats", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = json.loads(r.stdout)
    assert r.stdout.count("\n") == 1, r.stdout[-2000:]
    assert line["metric"].startswith("BED overlap queries/sec") and line["unit"] == "queries/s" and line["dtype"] == "u32"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
    assert line["config"]["regions_total"] == 1_000_000 and line["config"]["kept_pairs_total"] > 0
    assert not [k for k in FULL_LEGS if k in line], sorted(line)
