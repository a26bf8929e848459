"""The argument checks of the string-table handles (device/ids.hip, device/search.hip): every refusal here is decided before
any device call, so the library answers it on a machine without a GPU.  Each returns -1, leaves *out NULL where there is one
and leaves its message, with the name of the function that refused, in gffx_hip_last_error()."""
import ctypes as C

import numpy as np
import pytest

from gffx_amd import _ffi

OFF_OK = [0, 3]
BYTES = np.frombuffer(b"abc", np.uint8).copy()


def refused(fn, *args):
    L = _ffi.lib()
    assert getattr(L, fn)(*args) == -1, fn
    return L.gffx_hip_last_error().decode()


def u64s(v):
    a = np.array(v, dtype=np.uint64)
    return a, a.ctypes.data_as(_ffi.u64p)


def ids_create(n, names, off, hash_bits=-1, out=True):
    h = C.c_void_p(1)
    keep, p = u64s(off) if off is not None else (None, None)
    msg = refused("gffx_hip_ids_create", 0, n, None if names is None else names.ctypes.data_as(_ffi.u8p), p, 0, None, hash_bits,
                  C.byref(h) if out else None)
    assert not out or h.value is None
    return msg


def attrs_create(n, values, off, hash_bits=-1, dfa_path=0, key=b"", key_len=0, out=True):
    h = C.c_void_p(1)
    keep, p = u64s(off) if off is not None else (None, None)
    kb = None if key is None else C.cast(C.create_string_buffer(key, len(key) + 1), _ffi.u8p)
    msg = refused("gffx_hip_attrs_create", 0, n, None if values is None else values.ctypes.data_as(_ffi.u8p), p, 0, None, 0, None, kb, key_len,
                  hash_bits, dfa_path, C.byref(h) if out else None)
    assert not out or h.value is None
    return msg


@pytest.mark.parametrize("create,who,off_name,bytes_name", [(ids_create, "gffx_hip_ids_create", "name_off", "names"),
                                                            (attrs_create, "gffx_hip_attrs_create", "value_off", "values")])
def test_create_refusals(create, who, off_name, bytes_name):
    assert create(1, BYTES, OFF_OK, out=False) == "%s: out is NULL" % who
    assert create(1, BYTES, None) == "%s: %s is NULL" % (who, off_name)
    assert create(1, BYTES, [1, 3]) == "%s: %s[0] is not 0" % (who, off_name)
    assert create(2, BYTES, [0, 5, 3]) == "%s: %s is not ascending at 1" % (who, off_name)
    assert create(1, BYTES, OFF_OK, hash_bits=33) == "%s: hash_bits 33 (0 to 32; negative: all 32)" % who
    msg = create((1 << 28) + 1, BYTES, OFF_OK)  # (refused by the count alone: the offsets are not read)
    assert msg.startswith("%s: %d " % (who, (1 << 28) + 1)) and msg.endswith("(at most 2^28 each)")
    assert create(1, None, OFF_OK) == "%s: %s is NULL" % (who, bytes_name)


def test_attrs_create_refuses_a_dfa_path_and_a_missing_key():
    assert attrs_create(1, BYTES, OFF_OK, dfa_path=3) == "gffx_hip_attrs_create: dfa_path 3 (0: by size, 1: LDS, 2: global)"
    assert attrs_create(1, BYTES, OFF_OK, key=None, key_len=1) == "gffx_hip_attrs_create: key is NULL"


def test_a_null_handle_is_refused_under_the_functions_own_name():
    off, offp = u64s(OFF_OK)
    bp = BYTES.ctypes.data_as(_ffi.u8p)
    w32 = np.zeros(4, np.uint32)
    w32p = w32.ctypes.data_as(_ffi.u32p)
    lines = (None, bp, 3, 1, offp, w32p, 0, 0, None, None, bp)
    calls = [("gffx_hip_attrs_match_exact", (None, 1, bp, offp)),
             ("gffx_hip_ids_resolve", (None, 1, bp, offp, w32p, w32p)),
             ("gffx_hip_ids_filter_lines", lines), ("gffx_hip_attrs_filter_lines", lines),
             ("gffx_hip_ids_reset", (None,)), ("gffx_hip_attrs_reset", (None,))]
    calls += [("gffx_hip_%s_bitmap" % k, (None, offp, 2)) for k in ("ids_copy_root", "ids_copy_requested", "attrs_copy_matched",
                                                                     "attrs_copy_fid", "attrs_copy_root", "attrs_copy_invalid")]
    assert len(calls) == 12
    for fn, args in calls:
        assert refused(fn, *args) == "%s: NULL handle" % fn
