"""-m gpu: the scan kernel's LAYOUT logic against the oracle (tests/seam_case.py).  An occurrence of the pattern at every
offset d in [-(m + k) - 1, k + 1] across every kind of seam - lane, wave, row, tile, the first tile's end (clamped prefetch
path -> scalar path), the start and the end of the text (last tiles of 1, 15, 16, 17 bytes), the edges of the tapered
regions - for every instantiation of fz_scan_kernel, on a quiet background (complete expected stream from oracle runs
around the plants) and a noisy one (full queues, block-range passes, mid-scan flushes; oracle on the whole text), in every
regime plan_scan has: one tile per workgroup, tile iterations 0 .. 2 with the pipelined reload, the tapered plan of 1 GiB,
the plan of a scan launched behind another one, tiles beyond byte 2^32, a shard whose buffer starts off the tile grid.
Every case: the full ordered raw stream, stats()["verify_form"], and the coverage conditions for the plan that the
DEVICE's CU count gives.  Each case prints the coverage it asserted (pytest -s / -rP)."""
import os
import subprocess
import sys

import pytest

from tests import gpu_cases
from tests import seam_case as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cus = []


def device_cus():
    """Compute units of device 0 as the HIP runtime reports them: hipDeviceAttributeMultiprocessorCount, the
    multiProcessorCount that fz_create sizes the scan grids by.  Asked of the very runtime library the engine has loaded
    (found in the process's mappings): the C-ABI has no call for it, and the native sources are pinned to the committed
    bench line (tests/test_bench_contract.py), so a hook for the sake of a test would cost a re-measured bench."""
    if not _cus:
        import ctypes
        from fuzzysearch_amd import _native
        _native.load_library()
        with open("/proc/self/maps") as f:
            paths = sorted(set(ln.split()[-1] for ln in f if "libamdhip64.so" in ln))
        assert paths, "the engine's library has not loaded the HIP runtime"
        hip = ctypes.CDLL(paths[0])
        value = ctypes.c_int(0)
        HIP_ATTR_MULTIPROCESSOR_COUNT = 63                     # hip_runtime_api.h: hipDeviceAttribute_t, fixed within the ABI
        assert hip.hipDeviceGetAttribute(ctypes.byref(value), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0
        assert 8 <= value.value <= 1024, value.value
        _cus.append(value.value)
    return _cus[0]


def route(name):
    return next(r for r in sc.ROUTES if r.name == name)


@pytest.mark.parametrize("r", [r for r in sc.ROUTES if not r.env], ids=lambda r: r.name)
def test_one_tile_per_workgroup(engine, r):
    line, n_search, n_rows = gpu_cases.run_seam_route(engine, r, device_cus())
    print("%s | %d CUs, %d searches, %d rows" % (line, device_cus(), n_search, n_rows))
    assert n_search >= 2 and n_rows > 0


@pytest.mark.parametrize("r", [r for r in sc.ROUTES if r.env], ids=lambda r: r.name)
def test_one_tile_per_workgroup_under_a_switch(r):
    """The forms a process-wide switch selects, in a fresh interpreter: the small texts and the one-tile-per-workgroup text,
    then the text with several tiles per workgroup (gpu_cases.run_seam_route_iterations)."""
    e = dict(os.environ)
    e.update(r.env)
    res = subprocess.run([sys.executable, "-m", "tests.gpu_cases", "seams", r.name, str(device_cus())], cwd=ROOT, env=e,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = res.stdout.decode()
    assert res.returncode == 0 and "OK " in out, out[-3000:]
    print(out.strip())


def _many(r, n, background, text=None, keep=(), classes=sc.MANY, copies=2, phase=0, **kw):
    return sc.build(sc.route_pattern(r), r.k, n, device_cus(), background, phase=phase,
                    text=text, keep=keep, pattern_alphabet=r.alpha, **dict(sc.route_args(r), classes=classes, copies=copies, **kw))


NOISY_64 = ("band-L6-k2", "bits32-20-4", "bits32-12-3", "bits64-54-8", "subs-dense-20-4", "subs-L6-k3", "exact-8", "exact-20",
            "generic-20")


def test_tile_iterations_with_the_pipelined_reload_noisy(engine):
    """64 MiB on 256 CUs (the size comes from the plan hook: some workgroup gets three tiles): tile iterations 0 .. 2, the next
    tile's rows 0-1 loaded while rows 2-3 are tested.  Noisy background, oracle on the whole text, for the routes whose
    oracle is cheap at this size."""
    n = sc.size_with_iterations(device_cus(), 3, (64 << 20) + 4099)
    ntiles = (n + sc.TILE - 1) // sc.TILE
    for name in NOISY_64:
        r = route(name)
        case = _many(r, n, "noisy")
        assert max(o[1] for o in case.coverage["tile"]["tiles"]) >= 2
        want = sc.expected(r.kind, case)
        sc.check_exact_copies_found(r.kind, case, want)
        sc.check_coverage(case.coverage, r.m, r.k, sc.MANY, case.plan, ntiles)
        rows = gpu_cases.check_seam_case(engine, r, case, want, "noisy %d MiB" % (n >> 20))
        print("%s | %d CUs, grid %d, %d rows" % (sc.coverage_line(name, case.coverage, r.form), device_cus(), case.plan[0], rows))


def test_tile_iterations_with_the_pipelined_reload_quiet(engine):
    """The same regime on the quiet background for EVERY route that needs no switch (one text, re-planted route by route);
    the routes under a switch run it in their subprocess (test_one_tile_per_workgroup_under_a_switch)."""
    text = bg = None
    for r in sc.ROUTES:
        if not r.env:
            line, rows, text, bg = gpu_cases.run_seam_route_iterations(engine, r, device_cus(), text, bg)
            print("%s | %d CUs, %d rows" % (line, device_cus(), rows))


GIB_ROUTES = ("band-L6-k2", "bits32-20-4", "bits64-54-8", "bits128-65-10", "cells16-150-5", "subs-L6-k3", "exact-20")


def test_tapered_regions_and_the_overlapped_plan():
    """1 GiB + an odd tail, quiet: the tapered plan (about ten tile iterations, shrinking shares in the last resident round).
    One text with the tile sweep of every route (iterations 0, 1 and last) - searched one at a time, then two at a time in
    mixed kinds, where the younger search runs on the plan of a scan behind another one (16 tiles per workgroup, no taper,
    other stream, own counters), and once more after set_streams(1).  (That the younger search took that plan is not
    observable: stats() does not tell the plan, as in tests/test_gpu_overlap_default.py; what is asserted is that the plants
    reach iterations 0, 1 and last of the plan fz_debug_scan_plan gives for a launch that shares the chip, and both
    streams.)  Then, route by route, the full sweep over both seams
    of the first and last tile of every region, spread over as many texts as the route's sweep needs."""
    from fuzzysearch_amd import _native
    n = (1 << 30) + 12345
    ntiles = (n + sc.TILE - 1) // sc.TILE
    eng = _native.Engine([0])
    try:
        text, plants, cases = None, [], {}
        for name in GIB_ROUTES:
            case = _many(route(name), n, "quiet", text=text, keep=plants, classes=("tile",), copies=1, seed=3)
            text, plants = case.text, case.plants
            cases[name] = case
        h = eng.upload(text)
        wants = {}
        for name, case in cases.items():
            r = route(name)
            wants[name] = sc.sparse_expected(r.kind, case._replace(plants=plants))
            sc.check_exact_copies_found(r.kind, case._replace(plants=[pl for pl in plants if pl.data == case.pattern]), wants[name])
            sc.check_coverage(case.coverage, r.m, r.k, ("tile",), case.plan, ntiles, edited=False)
            got = gpu_cases.seam_search(eng, h, r.kind, case.pattern, r.k)
            assert got == wants[name], (name, len(got), len(wants[name]))
            assert eng.stats()["verify_form"] == r.form, name
            print("%s | %d CUs, grid %d, %d regions, %d rows" % (sc.coverage_line(name, case.coverage, r.form), device_cus(),
                                                                  case.plan[0], len(case.plan[3]), len(got)))
        for streams in (2, 1):
            eng.set_streams(streams)
            for a, b in (("band-L6-k2", "subs-L6-k3"), ("bits64-54-8", "band-L6-k2"), ("subs-L6-k3", "bits32-20-4"),
                         ("bits128-65-10", "bits128-65-10")):
                for name in (a, b):
                    r = route(name)
                    (eng.lev_ngrams_begin if r.kind == "lev" else eng.subs_ngrams_begin)(h, cases[name].pattern, r.k)
                assert eng.search_end() == wants[a], (a, "older of two in flight", streams)
                assert eng.search_end() == wants[b], (b, "younger of two in flight", streams)
        eng.set_streams(2)
        # the younger search's plan: the iterations the same plants reach there
        case = cases["band-L6-k2"]._replace(plants=plants)
        over = sc.scan_plan(case.pattern, 2, n, device_cus(), 1)
        assert over[2] and not over[3]
        under = sc.tiles_under(case, over)
        assert {0, 1} <= set(o[1] for o in under) and any(o[3] and o[1] > 1 for o in under)
        print("overlapped plan: grid %d, iterations %s planted" % (over[0], sorted(set(o[1] for o in under))))
        h.release()
        bg = cases["band-L6-k2"].bg
        bg.restore(text, plants)
        regions = cases["band-L6-k2"].plan[3]
        n_seams = len(sc.region_seams(ntiles, regions, n))
        for name in GIB_ROUTES if regions else ():
            r = route(name)
            covers = []
            for phase in range(sc.phases("region", r.m, r.k, n_seams) // 2):
                case = _many(r, n, "quiet", text=text, bg=bg, classes=("region",), copies=1, phase=phase, seed=3)
                want = sc.sparse_expected(r.kind, case)
                sc.check_exact_copies_found(r.kind, case, want)
                h = eng.upload(text)
                got = gpu_cases.seam_search(eng, h, r.kind, case.pattern, r.k)
                h.release()
                assert got == want, (name, "regions, text", phase, len(got), len(want))
                bg.restore(text, case.plants)
                covers.append(case.coverage)
            cov = sc.merge_coverage(covers)
            sc.check_coverage(cov, r.m, r.k, ("region",), case.plan, ntiles, edited=False)
            print("%s | %d CUs, %d regions, %d seams, %d texts" % (sc.coverage_line(name, cov, r.form), device_cus(), len(regions),
                                                                   n_seams, len(covers)))
    finally:
        eng.close()


def test_tiles_beyond_byte_2_to_the_32(engine):
    """4 GiB + 16 KiB + 5, quiet, one text re-planted turn by turn.  Every turn holds one copy at the seam 2^32 itself (the
    queue code's tile walk in 64 bits, the scalar window base and `(offset - reach) & ~3` where the carry into the high word
    happens) and one item of the end class, where the last tile holds 5 bytes: band - the WHOLE sweep of d across byte
    2^32; a bit-vector form and exact search - the straddling offsets d = -1, -L, -m/2, -m, -(m + k), -(m + k) - 1, 0 and
    k + 1, and as many more turns as their end class has items (copies ending at n, n - 1, .., truncated copies, exact and
    edited).  The first turn of a route also holds its tile sweep on the seams just below 2^32."""
    n = (4 << 30) + sc.TILE + 5
    seam = 1 << 32
    edge = seam // sc.TILE
    text = bg = None
    for name in ("band-L6-k2", "bits32-20-4", "exact-20"):
        r = route(name)
        offs = sc.sweep_offsets(r.m, r.k)
        L = r.m // (r.k + 1)
        end_turns = sc.phases("end", r.m, r.k)
        if name == "band-L6-k2":
            turns = list(range(max(len(offs), end_turns)))
        else:
            chosen = set(offs.index(d) for d in (-1, -L, -(r.m // 2), -r.m, -(r.m + r.k), -(r.m + r.k) - 1, 0, r.k + 1))
            turns = sorted(chosen | set(range(end_turns)))
        covers, rows = [], 0
        for i, turn in enumerate(turns):
            classes = ("first", "end") if turn < end_turns else ("first",)
            pool = [edge - 1 - j for j in range(len(offs) + 2)] if i == 0 else None
            case = _many(r, n, "quiet", text=text, bg=bg, classes=classes + (("tile",) if i == 0 else ()), copies=1, phase=turn,
                         tile_pool=pool, first_seam=seam, seed=5)
            text, bg = case.text, case.bg
            try:
                at = [pl for pl in case.plants if pl.cls == "first"]
                assert len(at) == 1 and at[0].seam == seam and at[0].d == offs[turn % len(offs)]
                want = sc.sparse_expected(r.kind, case)
                sc.check_exact_copies_found(r.kind, case, want)
                rows += gpu_cases.check_seam_case(engine, r, case, want, "4 GiB, turn %d (d = %d at 2^32)" % (turn, at[0].d))
            finally:
                bg.restore(text, case.plants)
            covers.append(case.coverage)
        cov = sc.merge_coverage(covers)
        sc.check_coverage(cov, r.m, r.k, ("end", "tile"), edited=False)
        assert set(offs.index(d) for d in cov["first"]["exact"]) >= set(t for t in turns if t < len(offs))
        if name == "band-L6-k2":
            sc.check_coverage(cov, r.m, r.k, ("first",))
        straddling = [d for d in cov["first"]["exact"] if -r.m < d < 0]
        assert len(straddling) >= 3, straddling
        print("%s | %d CUs, grid %d, %d texts, %d rows; at 2^32: d = %s" % (sc.coverage_line(name, cov, r.form), device_cus(),
                                                                            case.plan[0], len(turns), rows, sorted(cov["first"]["exact"])))


def test_shard_local_tile_seams():
    """Two shards on one device, 8 MiB quiet, the boundary not a multiple of 16: the second shard's buffer starts at
    own_lo - (m + k), so its tiles lie at buf_global_off + T * 16 384 of the text.  Tile seams of BOTH shards' grids, one
    band and one bit-vector search."""
    from fuzzysearch_amd import _native
    n = (8 << 20) + 333
    cut = (4 << 20) + 5
    eng = _native.Engine([0, 0])
    try:
        for name in ("band-L6-k2", "bits64-54-8"):
            r = route(name)
            p = sc.route_pattern(r)
            halo = r.m + r.k
            off1 = cut - halo
            case0 = _many(r, n, "quiet", classes=("tile",), tile_pool=range(2, cut // sc.TILE), seed=7)
            pool1 = range((cut - off1) // sc.TILE + 2, (n - off1) // sc.TILE)
            case = _many(r, n, "quiet", text=case0.text, keep=case0.plants, classes=("tile",), tile_base=off1, tile_pool=pool1, seed=8)
            for c in (case0, case):
                assert c.coverage["tile"]["exact"] == c.coverage["tile"]["edited"] == set(sc.sweep_offsets(r.m, r.k))
            assert off1 % 16 and all((pl.seam - off1) % sc.TILE == 0 for pl in set(case.plants) - set(case0.plants))
            want = sc.sparse_expected(r.kind, case)
            seq = eng.new_sequence(n)
            eng.add_shard(seq, 0, case.text[:cut + halo], 0, 0, cut)
            eng.add_shard(seq, 1, case.text[off1:], off1, cut, n)
            got = eng.lev_ngrams(seq, p, r.k)
            assert got == want, (name, len(got), len(want))
            assert eng.stats()["verify_form"] == r.form
            seq.release()
            print("%s | shard 1 buffer at byte %d (%% 16 = %d), %d rows" % (sc.coverage_line(name, case.coverage, r.form), off1, off1 % 16, len(got)))
    finally:
        eng.close()
