"""Shared by tests/test_scan_instance_host.py and tests/test_gpu_lean_scan.py: fz_debug_scan_instance through ctypes."""
import ctypes

from fuzzysearch_amd import _native

LEV, SUBS = 1, 2
REPEATED = b"ACGTAC" * 3 + b"GT"                      # three equal 6-grams at k = 2


def scan_instance(mode, p, k, buf_len=1 << 30, n_cus=256):
    """-> (launches, [launch i is lean], verify form)."""
    L = _native.load_library()
    nl, mask, form = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = L.fz_debug_scan_instance(mode, bytes(p), len(p), k, buf_len, n_cus, ctypes.byref(nl), ctypes.byref(mask), ctypes.byref(form))
    assert rc == 0
    return nl.value, [bool(mask.value >> i & 1) for i in range(nl.value)], form.value


def reload_switches():
    _native.load_library().fz_debug_reload_switches()
