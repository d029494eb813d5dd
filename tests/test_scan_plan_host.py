"""fz_debug_scan_plan (no device): the plan of a scan launched while another search of the context is in flight against the
plan of the same scan alone.  Only a fused in-memory scan is planned as overlapped; every other plan, and every plan of a
launch without a predecessor, is the one a synchronous call gets."""
import ctypes
import random

import numpy as np

from fuzzysearch_amd import _native

TILE = 16 << 10
TITER_MAX = (1 << 14) - 1
FORM_FUSED_BAND, FORM_KERNEL = 1, 5


def _plan(p, k, buf_len, n_cus, shares_chip):
    L = _native.load_library()
    grid, form, n = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    ov = ctypes.c_int(0)
    tab = np.zeros(4 * 8, dtype=np.uint64)
    rc = L.fz_debug_scan_plan(p, len(p), k, buf_len, n_cus, shares_chip, ctypes.byref(grid), ctypes.byref(form), ctypes.byref(ov),
                              ctypes.byref(n), ctypes.c_void_p(tab.ctypes.data))
    assert rc == 0
    return grid.value, form.value, bool(ov.value), [tuple(int(x) for x in tab[4 * r:4 * r + 4]) for r in range(n.value)]


def _regions(ntiles, grid, n_cus):
    L = _native.load_library()
    n = ctypes.c_uint32(0)
    tab = np.zeros(4 * 8, dtype=np.uint64)
    assert L.fz_debug_scan_regions(ntiles, grid, n_cus, 4, 0.25, 7, ctypes.byref(n), ctypes.c_void_p(tab.ctypes.data)) == 0
    return [tuple(int(x) for x in tab[4 * r:4 * r + 4]) for r in range(n.value)]


def _grid_alone(buf_len, n_cus):
    """The grid rule of a scan alone on the chip (fzhip.hip: plan_scan): whole rounds of 6 workgroups per CU of ~9.5 tiles
    each below 120 rounds, 12 tiles per workgroup beyond."""
    ntiles = (buf_len + TILE - 1) // TILE
    resident = n_cus * 6
    max_grid = max(resident, ntiles // 12)
    if ntiles < resident * 120:
        max_grid = resident * max(1, (2 * ntiles + resident * 19 // 2) // (resident * 19))
    return ntiles, max(1, -(-ntiles // TITER_MAX), min(ntiles, max_grid))


def _grid_overlapped(buf_len, n_cus):
    """... and of a scan next to its predecessor: 16 tiles per workgroup, at least 6 workgroups per CU."""
    ntiles = (buf_len + TILE - 1) // TILE
    return ntiles, max(1, -(-ntiles // TITER_MAX), min(ntiles, max(n_cus * 6, ntiles // 16)))


def test_headline_plan_without_a_predecessor_is_unchanged():
    """|p| = 20, k = 2 on 256 CUs: 1 GiB = 4 whole rounds (6 144 workgroups) with the tapered last round, 4 GiB = 12 tiles
    per workgroup (21 845); a launch behind a search in flight is overlapped (16 tiles per workgroup, no taper), a launch
    without one is not."""
    p = b"ACGTTGCAACGGTACCATGA"
    for mib, grid in ((1024, 6144), (4096, 21845)):
        n = mib << 20
        g, form, ov, regs = _plan(p, 2, n, 256, 0)
        assert (g, form, ov) == (grid, FORM_FUSED_BAND, False)
        assert regs == _regions(n // TILE, grid, 256) and len(regs) == 5
        assert _plan(p, 2, n, 256, 1) == (n // TILE // 16, form, True, [])


def test_plans_match_the_rule_alone_and_only_fused_scans_overlap():
    rnd = random.Random(7)
    for _ in range(300):
        m = rnd.choice([8, 12, 20, 24, 40, 64, 100, 150, 300])
        k = rnd.randint(0, min(m - 1, 30))
        p = bytes(rnd.choice(b"ACGT" if rnd.random() < 0.5 else b"abcdefghijklmnopqrstuvwxyz") for _ in range(m))
        n_cus = rnd.choice([8, 64, 104, 256, 304])
        buf_len = rnd.choice([1, 4096, 1 << 20, rnd.randint(1, 1 << 34), 1 << 30, 4 << 30])
        ntiles, grid = _grid_alone(buf_len, n_cus)
        g, form, ov, regs = _plan(p, k, buf_len, n_cus, 0)
        assert (g, ov) == (grid, False)
        assert regs == _regions(ntiles, grid, n_cus)
        g1, form1, ov1, regs1 = _plan(p, k, buf_len, n_cus, 1)
        assert form1 == form
        assert ov1 == (form != FORM_KERNEL)
        if not ov1:
            assert (g1, regs1) == (g, regs)
        else:
            assert (g1, regs1) == (_grid_overlapped(buf_len, n_cus)[1], [])


def test_unfused_scan_is_never_overlapped():
    """A scan behind a hit list (a verification kernel of its own follows) shares d_hits with nothing: it stays behind its
    predecessor on the same stream, with the plan of a scan alone."""
    p = bytes(random.Random(3).choice(b"ACGT") for _ in range(300))
    alone = _plan(p, 40, 1 << 30, 256, 0)
    assert alone[1] == FORM_KERNEL
    assert _plan(p, 40, 1 << 30, 256, 1) == alone
