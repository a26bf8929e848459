"""`gffx coverage --gpus` and the union builder's C-ABI where no GPU is needed: the option is known to the command line,
and without a device (or a handle) every entry point reports an error instead of computing or crashing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gffx_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFFX = os.path.join(ROOT, "gffx_amd", "bin", "gffx")


def test_coverage_help_lists_gpus():
    r = subprocess.run([GFFX, "coverage", "--help"], capture_output=True)
    assert r.returncode == 0 and b"--gpus <N>" in r.stdout and b"--stats-json <FILE>" in r.stdout


def test_coverage_gpus_needs_a_number(tmp_path):
    r = subprocess.run([GFFX, "coverage", "-i", str(tmp_path / "x.gff"), "-s", str(tmp_path / "x.bed"), "--gpus", "x"],
                       capture_output=True)
    assert r.returncode == 2 and b"invalid value 'x' for '--gpus <N>'" in r.stderr
    r = subprocess.run([GFFX, "coverage", "-i", str(tmp_path / "x.gff"), "-s", str(tmp_path / "x.bed"), "--gpus"],
                       capture_output=True)
    assert r.returncode == 2


def test_a_null_union_is_reported_not_crashed_on():
    L = _ffi.lib()
    rows = np.array([[0, 1, 2]], np.uint32)
    out = np.zeros(4, np.uint64)
    rcs = [L.gffx_hip_union_add_host(None, rows.ctypes.data_as(_ffi.u32p), 1),
           L.gffx_hip_union_add_store(None, None, 0, 0, 0),
           L.gffx_hip_union_add_spans(None, out.ctypes.data_as(_ffi.u64p), None, None),
           L.gffx_hip_union_finish(None),
           L.gffx_hip_union_copy_spans(None, out.ctypes.data_as(_ffi.u64p), None, None, None),
           L.gffx_hip_union_segments_covered(None, 0, None, None, None, None),
           L.gffx_hip_union_stats(None, None, None, None)]
    assert rcs == [-1] * len(rcs) and b"union is NULL" in L.gffx_hip_last_error()
    assert L.gffx_hip_union_n_spans(None) == 0
    L.gffx_hip_union_destroy(None)
    assert L.gffx_hip_union_create(0, 3, None) == -1


@pytest.mark.skipif(engine.device_count() > 0, reason="checks the behaviour of a machine without a GPU")
def test_without_a_gpu_the_union_cannot_be_created():
    h = C.c_void_p()
    assert _ffi.lib().gffx_hip_union_create(0, 3, C.byref(h)) == -2 and not h.value
    with pytest.raises(_ffi.GffxHipError) as ei:
        engine.RegionUnion(3)
    assert ei.value.code == -2
