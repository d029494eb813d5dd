"""The scan kernel's tile walk in both directions, no device: fz_debug_scan_plan gives the plan of a launch and
fz_debug_scan_walk - through fz_scan_walk / fz_walk_tile of fz_device.h, the functions the kernel itself calls - the tile of
the buffer that (workgroup, iteration) reads, forward and reversed.  For 1, 4 and 256 CUs, alone and behind another search,
and buffers of 1, 2, 3 tiles, one tile either side of the smallest grid, the smallest buffer whose plan has regions and one
tile more: every tile has exactly one (workgroup, iteration) in each direction, the reversed walk is the mirror of the
forward one, iterations stay below FZ_TITER_MAX.  The same cases once more through a stand-alone program that compiles the
header for the host (tests/scan_walk_emul.cpp), plain and under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from fuzzysearch_amd import _native
from tests import seam_case as sc

HERE = os.path.dirname(os.path.abspath(__file__))
P, K = b"ACGTTGCAACGTACGGTCAT", 2
TITER_MAX = (1 << (32 - 14 - 4)) - 1                  # fz_kernels.h: FZ_TITER_MAX
NONE = (1 << 64) - 1


def plan(ntiles, n_cus, shares):
    return sc.scan_plan(P, K, ntiles * sc.TILE, n_cus, shares)


def first_with_regions(n_cus):
    """The smallest tile count whose plan (a scan alone) has regions."""
    for ntiles in range(1, 1 << 17):
        if plan(ntiles, n_cus, 0)[3]:
            return ntiles
    raise AssertionError("no plan with regions below 2 GiB on %d CUs" % n_cus)


_sizes = {}


def sizes(n_cus):
    if n_cus not in _sizes:
        small = 6 * n_cus                                 # the smallest grid a buffer of that many tiles or more gets
        reg = first_with_regions(n_cus)
        _sizes[n_cus] = sorted(set([1, 2, 3, small - 1, small, small + 1, reg, reg + 1]) - {0})
    return _sizes[n_cus]


def walk(ntiles, grid, regions, reversed_):
    """-> (tile -> (workgroup, iteration)) as two arrays, most iterations of a workgroup."""
    L = _native.load_library()
    tab = np.array([x for r in regions for x in r], dtype=np.uint64) if regions else np.zeros(4, dtype=np.uint64)
    owner = np.full(ntiles, -1, dtype=np.int64)
    it_of = np.full(ntiles, -1, dtype=np.int64)
    tile = ctypes.c_uint64(0)
    fn, ref, tabp, most = L.fz_debug_scan_walk, ctypes.byref(tile), ctypes.c_void_p(tab.ctypes.data), 0
    for wg in range(grid):
        it = 0
        while True:
            assert fn(ntiles, grid, len(regions), tabp, wg, it, reversed_, ref) == 0
            if tile.value == NONE:
                break
            assert tile.value < ntiles, (wg, it, tile.value)
            assert owner[tile.value] < 0, ("tile read twice", tile.value, wg, it)
            owner[tile.value], it_of[tile.value] = wg, it
            it += 1
        most = max(most, it)
    return owner, it_of, most


@pytest.mark.parametrize("shares", [0, 1], ids=["alone", "behind"])
@pytest.mark.parametrize("n_cus", [1, 4, 256])
def test_every_tile_has_one_owner_in_each_direction_and_the_reversed_walk_is_the_mirror(n_cus, shares):
    grids, with_regions = set(), 0
    for ntiles in sizes(n_cus):
        grid, _form, overlapped, regions = plan(ntiles, n_cus, shares)
        assert 1 <= grid <= ntiles and overlapped == bool(shares)
        fo, fi, most = walk(ntiles, grid, regions, 0)
        ro, ri, most_r = walk(ntiles, grid, regions, 1)
        assert (fo >= 0).all() and (ro >= 0).all(), (ntiles, "tiles never read")
        assert most == most_r < TITER_MAX
        # the mirror: tile T forward and tile ntiles - 1 - T reversed are the same step of the same workgroup
        assert np.array_equal(fo, ro[::-1]) and np.array_equal(fi, ri[::-1]), ntiles
        # ... and forward the walk is what the seam tests take it for
        for T in sorted(set([0, ntiles // 2, ntiles - 1])):
            assert (fo[T], fi[T]) == sc.tile_owner(T, ntiles, grid, regions)[:2]
        assert fo[0] == 0 and ro[ntiles - 1] == 0 and fi[0] == 0      # workgroup 0 starts at the first / the last tile
        grids.add((ntiles > grid) - (ntiles < grid))
        with_regions += bool(regions)
    assert grids == {0, 1}                                             # buffers of exactly one grid, and of more
    assert with_regions >= (0 if shares else 2)


def test_the_walk_hook_refuses_what_is_not_a_plan():
    L = _native.load_library()
    tile = ctypes.c_uint64(0)
    assert L.fz_debug_scan_walk(4, 2, 0, None, 2, 0, 0, ctypes.byref(tile)) != 0       # workgroup outside the grid
    assert L.fz_debug_scan_walk(4, 0, 0, None, 0, 0, 0, ctypes.byref(tile)) != 0
    assert L.fz_debug_scan_walk(4, 2, 9, None, 0, 0, 0, ctypes.byref(tile)) != 0       # more regions than a launch has
    assert L.fz_debug_scan_walk(4, 2, 0, None, 1, 1, 1, ctypes.byref(tile)) == 0 and tile.value == 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_header_s_walk_compiled_for_the_host(flags):
    cases = []
    for n_cus in (1, 4, 256):
        for shares in (0, 1):
            for ntiles in sizes(n_cus):
                grid, _form, _ov, regions = plan(ntiles, n_cus, shares)
                cases.append((ntiles, grid, regions))
    stem = os.path.join(tempfile.gettempdir(), "fz_scan_walk_emul_%d_%d" % (os.getpid(), len(flags)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + [os.path.join(HERE, "scan_walk_emul.cpp"), "-o", stem])
    try:
        with open(stem + ".cases", "w") as f:
            for ntiles, grid, regions in cases:
                f.write("%d %d %d %s\n" % (ntiles, grid, len(regions), " ".join(str(x) for r in regions for x in r)))
        out = subprocess.run([stem, stem + ".cases"], capture_output=True, text=True, timeout=300)
    finally:
        for path in (stem, stem + ".cases"):
            if os.path.exists(path):
                os.unlink(path)
    assert out.returncode == 0, out.stderr
    rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
    assert [(r[0], r[1]) for r in rows] == [(c[0], c[1]) for c in cases]
    assert all(r[2] == r[0] and r[3] < TITER_MAX for r in rows)


def test_rounds_plan_lays_the_first_and_last_round_down_in_address_order(monkeypatch):
    """FZ_SCAN_ROUNDS=1, 1 GiB behind another search on 256 CUs: {first resident front | middle | last front}.  Iteration i of
    the first front reads the tiles [i W, (i + 1) W) and the last front's ranges end at the buffer's end, so the launch
    begins and ends with 448 MiB read in address order, one front (28 MiB) at a time; a scan alone keeps its plan."""
    L = _native.load_library()
    alone = plan(65536, 256, 0)
    monkeypatch.setenv("FZ_SCAN_ROUNDS", "1")
    L.fz_debug_reload_switches()
    try:
        assert plan(65536, 256, 0) == alone
        assert not plan(32768, 256, 1)[3]                        # fewer than two fronts of workgroups: nreg = 0 as before
        grid, _form, overlapped, regions = plan(65536, 256, 1)
        W = 256 * 7
        assert overlapped and grid == 4096 and [r[:2] for r in regions] == [(0, W), (W, grid - 2 * W), (grid - W, W)]
        assert regions[0][2] == 0 and regions[-1][3] == 65536 and all(a[3] == b[2] for a, b in zip(regions, regions[1:]))
        fo, fi, most = walk(65536, grid, regions, 0)
        ro, ri, _ = walk(65536, grid, regions, 1)
        assert (fo >= 0).all() and np.array_equal(fo, ro[::-1]) and np.array_equal(fi, ri[::-1]) and most == 16
        for wg0, nwg, t0, t1 in (regions[0], regions[-1]):
            assert (t1 - t0) * sc.TILE >= 256 << 20
            for it in range((t1 - t0) // nwg):
                tiles = np.flatnonzero((fo >= wg0) & (fo < wg0 + nwg) & (fi == it))
                assert len(tiles) == nwg and tiles[0] == t0 + it * nwg and tiles[-1] == tiles[0] + nwg - 1
    finally:
        monkeypatch.delenv("FZ_SCAN_ROUNDS")
        L.fz_debug_reload_switches()
