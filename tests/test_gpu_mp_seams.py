"""-m gpu: the multi-pattern pass at every seam of its layout and of its launch shapes (tests/mp_seam_case.py; the construction
is checked on the CPU by tests/test_mp_seam_case.py).  fz_mp_filter_kernel<DH = 1..5>, fz_mp_verify_kernel,
fz_mp_verify_subs_kernel, fz_mp_verify_cls_kernel and the three fz_mp_batch_verify_* twins, each route a LIST of patterns
that rides one pass as one group: a copy of every carrier at every offset d in [-(m + k) - 1, k + 1] across wave, row and
tile seams, the first seams of a small text, its start and its end (last lane rows of 1, 15, 16, 17 bytes), quiet and
noisy; tile iterations 0, 1 and last of the filter's grid-stride walk with the wave queue carried from tile to tile; the
verification kernels' second and third sweep of a hit list; a shard cut off the 16-byte grid; the ragged instances at every
seam between the sequences of a batch.  Every comparison: every pattern's full ordered raw stream against the oracle
(oracle.lev_ngrams_raw, oracle.subs_ngrams_raw) or the class model (tests/classes_model.py::raw_rows),
stats()["verify_form"] == 5 and stats()["raw_matches"].  Each test prints the coverage it asserted (pytest -s / -rP).

On an engine of the module's own: the pass's hit lists and record buffer only grow, and tests of other modules count on the
shared engine's first sizing (tests/test_gpu_multi.py::test_dense_case_and_overflow)."""
import time

import pytest

from fuzzysearch_amd import _native
from tests import gpu_cases
from tests import mp_seam_case as mc
from tests import seam_case as sc
from tests.test_gpu_scan_seams import device_cus

pytestmark = pytest.mark.gpu
force_pass = pytest.fixture(gpu_cases.force_pass)

LEV_SUBS = [r for r in mc.ROUTES if r.mode != "cls"]
BY_NAME = dict(ids=lambda r: r.name)


@pytest.fixture(autouse=True)
def ride_a_pass(force_pass):
    """Every list of this module rides a pass, whatever the cost rule expects of it (class lists always do)."""
    force_pass(True)


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine([0])
    yield e
    e.close()


def _ntiles(n):
    return (n + sc.TILE - 1) // sc.TILE


@pytest.mark.parametrize("r", mc.ROUTES, **BY_NAME)
def test_wave_row_and_tile_seams_quiet(eng, r):
    """One tile per workgroup: the whole sweep of every carrier, exact and edited, across wave, row and tile seams of one
    quiet text; the expected stream of every pattern of the list from the oracle around the plants."""
    n = mc.text_bytes(r)
    case = mc.build(r, n, device_cus())
    assert mc.one_group(r, case.patterns) and case.plan[0] == _ntiles(n) <= mc.FILTER_WG_PER_CU * device_cus()
    want = mc.sparse_expected(case)
    mc.check_exact_copies_found(case, want)
    mc.check_coverage(case, sc.MANY, _ntiles(n))
    rows = gpu_cases.check_mp_case(eng, case, want, "quiet")
    print("%s | %d CUs, %d rows" % (mc.coverage_line(case), device_cus(), rows))


@pytest.mark.parametrize("r", mc.ROUTES, **BY_NAME)
def test_first_seams_start_and_end_quiet(eng, r):
    """Small texts (a tile per carrier, two more and a tail of 777, 1, 15, 16, 17 bytes - the last lane row short, its halo
    load reading the padding): carrier i's sweep across the seam behind tile i, one text per d; the start and end items of
    every carrier: whole copies 0 .. k + 1 bytes off the edge and copies that lost up to k characters to it."""
    cases, rows = [], 0
    for case in mc.edge_cases(r, device_cus()):
        want = mc.sparse_expected(case)
        mc.check_exact_copies_found(case, want)
        rows += gpu_cases.check_mp_case(eng, case, want, "edge n = %d, d = %s" % (len(case.text), [(pl.cls, pl.d) for pl in case.plants]))
        cases.append(case)
    cover = mc.merge_coverage(cases)
    for i, m in enumerate(r.lengths):
        assert set(cover[i]) == {"first", "start", "end"}
        mc.check_edge_coverage(cover[i], m, r.k)
    assert set(len(c.text) % sc.TILE for c in cases) == set(sc.EDGE_TAILS)
    print("%s | %d CUs, %d texts, %d rows" % (mc.coverage_line(cases[0], cover), device_cus(), len(cases), rows))


@pytest.mark.parametrize("r", mc.ROUTES, **BY_NAME)
def test_wave_row_and_tile_seams_noisy(eng, r):
    """The same sweep on a background over the patterns' own alphabet: hits of every pattern at the background's rate, the
    wave queues carrying them between the plants' (the lists of four-character n-grams over DNA fill a queue and flush it
    inside a tile); the oracle - the class model - on the whole text, for every pattern of the list."""
    t0 = time.perf_counter()
    n = mc.text_bytes(r)
    case = mc.build(r, n, device_cus(), "noisy")
    want = mc.expected(case)
    mc.check_exact_copies_found(case, want)
    mc.check_coverage(case, sc.MANY, _ntiles(n))
    rows = gpu_cases.check_mp_case(eng, case, want, "noisy")
    print("%s | %d CUs, noisy, %d rows, %.2f s" % (mc.coverage_line(case), device_cus(), rows, time.perf_counter() - t0))


_big = {}


def _big_text():
    """One quiet text with more than two tiles per filter workgroup (80 MiB on 256 CUs), built once and re-planted route by
    route."""
    grid = mc.FILTER_WG_PER_CU * device_cus()
    n = (2 * grid + grid // 2) * sc.TILE + 4099
    return n, _big.get("text"), _big.get("bg")


@pytest.mark.parametrize("r", LEV_SUBS + [mc.route("cls-L6-k1")], **BY_NAME)
def test_tile_iterations(eng, r):
    """The grid-stride step of the filter (tile += gridDim.x), the wave queue carried from one tile into the next and the
    final flush after several tiles: the tile sweep of every carrier, exact and edited, on tiles of the iterations 0, 1 and
    last of the walk."""
    t0 = time.perf_counter()
    n, text, bg = _big_text()
    case = mc.build(r, n, device_cus(), classes_=("tile",), text=text, bg=bg, seed=2)
    _big["text"], _big["bg"] = case.text, case.bg
    try:
        assert _ntiles(n) > 2 * case.plan[0] and case.plan[0] == mc.FILTER_WG_PER_CU * device_cus()
        mc.check_coverage(case, ("tile",), _ntiles(n))
        for i in case.own:
            assert {0, 1, 2} <= set(o[1] for o in case.coverage[i]["tile"]["tiles"])
        want = mc.sparse_expected(case)
        mc.check_exact_copies_found(case, want)
        rows = gpu_cases.check_mp_case(eng, case, want, "quiet, %d MiB" % (n >> 20))
    finally:
        case.bg.restore(case.text, case.plants)
    print("%s | %d CUs, %d MiB, %d rows, %.2f s" % (mc.coverage_line(case), device_cus(), n >> 20, rows, time.perf_counter() - t0))


@pytest.mark.parametrize("mode", ["lev", "subs", "cls"])
def test_second_sweep_of_a_hit_list(mode):
    """Every offset of an all-`A` text is a hit of both patterns: every one of the 16 hit lists holds more than two sweeps of
    the verification launch (16 x CUs waves x 64 candidates), so every wave steps q0 += waves * 64 at least twice; the
    filter's queues fill and flush many times per tile; the first sizing of the lists overflows.  On an engine of its own:
    the lists only grow."""
    cus = device_cus()
    pats, cases = mc.dense_case(mode, cus)
    r = mc.Route("dense-" + mode, mode, 2, (20,), sc.DNA)
    assert mc.one_group(r, pats)
    want = [sc.sparse_expected(mode, c) for c in cases]
    for i, (c, w) in enumerate(zip(cases, want)):
        sc.check_exact_copies_found(mode, c._replace(plants=[pl for pl in c.plants if pl.d == i]), w)
    e = _native.Engine([0])
    try:
        h = e.upload(cases[0].text)
        got = gpu_cases.mp_search(e, h, r, pats)
        st = e.stats()
        h.release()
    finally:
        e.close()
    rows = gpu_cases.check_mp_streams(r, pats, got, want, st, "all A")
    per_list = st["ngram_hits"] / mc.LISTS / len(pats)
    print("mp dense %s: %d CUs, %d bytes, %d n-gram hits (%.0f per list and pattern, %.2f sweeps of %d), %d launches, %d rows"
          % (mode, cus, len(cases[0].text), st["ngram_hits"], per_list, per_list / mc.verify_sweep(cus), mc.verify_sweep(cus),
             st["filter_launches"], rows))
    assert st["ngram_hits"] / 16 > 2 * 1024 * cus and per_list > 2 * mc.verify_sweep(cus), "the third batch of every list was reached"
    assert st["filter_launches"] >= 2, "the first sizing should not have held this"
    assert rows >= len(cases[0].plants) // 2


@pytest.mark.parametrize("name", ["lev-L6-k2", "subs-L8-k3", "cls-L4-k1"])
def test_shard_cut(eng, name):
    """2 tiles + 301 bytes, cut at byte 16 384 + 150 - no multiple of 16 -, the second shard's buffer starting a halo before
    it: the full sweep of every carrier across the cut, exact and edited (own_lo / own_hi decide who reports a hit, buf_off
    where a tile lies)."""
    r = mc.route(name)
    cut, n = sc.TILE + 150, 2 * sc.TILE + 301
    assert cut % 16
    covers, texts, rows = gpu_cases.run_mp_shard_cut(eng, r, cut, n)
    print("mp shard cut %s: %d texts, %d rows; d per carrier: %s" % (
        name, texts, rows, ["%d+%d" % (len(c["first"]["exact"]), len(c["first"]["edited"])) for c in covers.values()]))


@pytest.mark.parametrize("name", ["lev-L6-k2", "subs-L4-k8", "cls-L8-k3"])
def test_ragged_instances(eng, name):
    """fz_mp_batch_verify_kernel, fz_mp_batch_verify_subs_kernel, fz_mp_batch_verify_cls_kernel: the seam classes of
    tests/batch_seam_case.py for every carrier, the whole list searched, raw and reduced."""
    t0 = time.time()
    line, n_search, n_rows = gpu_cases.run_mp_batch_seams(eng, mc.route(name))
    print("%s | %d searches, %d rows, %.1f s" % (line, n_search, n_rows, time.time() - t0))
    assert n_search >= 2 and n_rows > 0
