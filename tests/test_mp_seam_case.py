"""tests/mp_seam_case.py on the CPU: the licence for holding the multi-pattern pass against the SPARSE expected stream at
sizes where the oracle never runs on the whole text, and the conditions the built inputs have to meet - for every route
(list of patterns) of the device tests, at small sizes."""
import random

import numpy as np
import pytest

from fuzzysearch_amd import _native
from tests import classes_model
from tests import gpu_cases
from tests import mp_seam_case as mc
from tests import seam_case as sc

N_CUS = 256
force_pass = pytest.fixture(gpu_cases.force_pass)


def test_launch_shape_mirrors_the_host_code():
    assert mc.launch_shape() == (mc.FILTER_WG_PER_CU, mc.VERIFY_WG_PER_CU) == (8, 4)
    # the plan seam_case.build() takes in place of the scan plan: one tile per workgroup up to 8 x CUs tiles, then the stride
    assert mc.mp_plan(5 * sc.TILE + 1, 256) == (6, mc.FORM_KERNEL, False, [])
    assert mc.mp_plan((32 << 20) + 1, 256)[0] == 2048 == mc.mp_plan(1 << 30, 256)[0]
    assert sc.tile_owner(2048 + 7, 5000, 2048, []) == (7, 1, -1, False) and sc.tile_owner(4999, 5000, 2048, [])[3]
    assert mc.verify_sweep(256) == 262144


def test_routes_cover_every_filter_instance():
    for mode in ("lev", "subs"):
        rs = [r for r in mc.ROUTES if r.mode == mode]
        assert sorted(set(mc.dh(r.lengths[0] // (r.k + 1)) for r in rs)) == [1, 2, 3, 4, 5]
        assert any(r.lengths[0] // (r.k + 1) > 8 and r.k == 8 and 128 in r.lengths for r in rs)          # FZ_MP_MAX_K, FZ_MP_MAX_M
        assert any(r.lengths[0] // (r.k + 1) == 4 and r.lengths[0] // 4 == 9 for r in rs)                # nine blocks
    cls = [r for r in mc.ROUTES if r.mode == "cls"]
    assert sorted(r.lengths[0] // (r.k + 1) for r in cls) == [4, 6, 8, 14]
    assert set(m % 4 for r in cls for m in r.lengths) == {0, 1, 2, 3}


@pytest.mark.parametrize("r", mc.ROUTES, ids=lambda r: r.name)
def test_list_is_one_group_with_shared_blocks(force_pass, r):
    force_pass(True)
    pats, carriers = mc.list_of(r)
    nc = len(r.lengths)
    L = r.lengths[0] // (r.k + 1)
    assert mc.one_group(r, pats), "the list rides one pass as one group"
    assert [len(pats[i]) for i in carriers] == list(r.lengths) and len(pats) == 2 * nc + 3 and len(set(pats)) == len(pats)
    assert all(len(p) // (r.k + 1) == L for p in pats)
    for i in carriers:
        c, d = pats[i], pats[nc + i]
        assert d[:L] == c[:L] and len(d) != len(c), "block 0 shared, another length in the wave"
        assert all(d[g:g + L] != c[g:g + L] for g in range(L, min(len(c), len(d)) - L + 1, L))
    c, d = pats[nc - 1], pats[2 * nc]
    g = (len(c) // L - 1) * L
    assert d[g:g + L] == c[g:g + L] and all(d[q:q + L] != c[q:q + L] for q in range(0, g, L))
    if r.mode == "cls":
        where = set()
        for i in carriers:
            p, m = pats[i], len(pats[i])
            for q in (q for q in range(m) if p[q] in mc.IUPAC):
                where |= {"first"} if q == 0 else set()
                where |= {"last"} if q == m - 1 else set()
                where |= {"tail"} if q >= (m // L) * L else set()
                where |= {"hashed"} if q < (m // L) * L and (q % L < 4 or q % L >= mc.dh(L)) and q % L < 8 else set()
                where |= {"beyond 8"} if q < (m // L) * L and q % L >= 8 else set()
        assert where >= {"first", "last", "hashed"} | ({"beyond 8"} if L > 8 else set())
        assert "tail" in where or all(m % L == 0 for m in r.lengths)


@pytest.mark.parametrize("r", mc.ROUTES, ids=lambda r: r.name)
def test_sparse_stream_is_the_full_oracle_stream(r):
    """The wave and row sweep of every carrier in one quiet text that holds it and little more (0.6 to 6 MiB): the sparse
    stream of EVERY pattern of the list equals the oracle on the whole text, order included; every d of both classes as an
    exact and an edited copy for every carrier; every exact copy has its row.  (That equality does not depend on the kind of
    seam a copy lies on; the tile class, which needs a tile per copy, is held against the whole-text oracle for one route in
    test_tile_iterations_under_the_multi_pattern_plan.)"""
    classes = ("wave", "row")
    n = mc.text_bytes(r, classes_=classes)
    case = mc.build(r, n, N_CUS, classes_=classes)
    want = mc.sparse_expected(case)
    assert want == mc.expected(case)
    mc.check_exact_copies_found(case, want)
    mc.check_coverage(case, classes, (n + sc.TILE - 1) // sc.TILE)
    assert len(case.plants) == sum(len(classes) * 2 * len(sc.sweep_offsets(m, r.k)) for m in r.lengths)


@pytest.mark.parametrize("r", mc.ROUTES, ids=lambda r: r.name)
def test_device_text_holds_every_sweep(r):
    """The text of the device tests (text_bytes: the wave, row and tile sweep of every carrier): no plant skipped, every d of
    every class exact and edited for every carrier, the plants apart, every exact copy has its row in the sparse stream."""
    n = mc.text_bytes(r)
    case = mc.build(r, n, N_CUS)
    mc.check_coverage(case, sc.MANY, (n + sc.TILE - 1) // sc.TILE)
    assert len(case.plants) == sum(len(sc.MANY) * 2 * len(sc.sweep_offsets(m, r.k)) for m in r.lengths)
    assert sum(len(v) for v in case.own.values()) == len(case.plants)
    for a, b in zip(case.plants, case.plants[1:]):
        assert a.start + len(a.data) + sc.GRAIN <= b.start
    mc.check_exact_copies_found(case, mc.sparse_expected(case))


@pytest.mark.parametrize("r", mc.ROUTES, ids=lambda r: r.name)
def test_edge_texts_sparse_stream_and_coverage(r):
    """The few-seam classes on their small texts: over the phases every d of `first`, `start` and `end`, exact AND edited, for
    every carrier; every tail of EDGE_TAILS; every exact copy has its row.  sparse == full for every pattern on the first ten
    texts and on every seventh one after them (7 and the five tails are coprime: every tail is among them)."""
    cases = []
    for ph, case in enumerate(mc.edge_cases(r, N_CUS)):
        want = mc.sparse_expected(case)
        if ph < 10 or ph % 7 == 0:
            assert want == mc.expected(case)
        mc.check_exact_copies_found(case, want)
        cases.append(case)
    cover = mc.merge_coverage(cases)
    assert sorted(cover) == list(range(len(r.lengths)))
    for i, m in enumerate(r.lengths):
        assert set(cover[i]) == {"first", "start", "end"}
        mc.check_edge_coverage(cover[i], m, r.k)
    assert set(len(c.text) % sc.TILE for c in cases) == set(sc.EDGE_TAILS)
    assert set(len(c.text) % sc.TILE for ph, c in enumerate(cases) if ph % 7 == 0) == set(sc.EDGE_TAILS) or len(cases) < 35


def test_edge_coverage_check_notices_a_missing_edited_half():
    """check_edge_coverage fails where seam_case.check_coverage alone passes: the exact phases only."""
    r = mc.route("subs-L4-k1")
    cases = list(mc.edge_cases(r, N_CUS))
    m = r.lengths[0]
    full = mc.merge_coverage(cases)[0]
    mc.check_edge_coverage(full, m, r.k)
    for cls in ("first", "start", "end"):
        cut = {c: dict(v) for c, v in full.items()}
        cut[cls]["edited"] = set(sorted(full[cls]["edited"])[1:])
        sc.check_coverage(cut, m, r.k, ("first", "start", "end"))
        with pytest.raises(AssertionError):
            mc.check_edge_coverage(cut, m, r.k)


def test_tile_iterations_under_the_multi_pattern_plan():
    """A text of more than two tiles per filter workgroup: the tile sweep of every carrier reaches the iterations 0, 1 and
    last of the multi-pattern plan; for the substitutions route (the cheapest oracle) the sparse stream of the tile class
    is the oracle's on the whole text."""
    n_cus = 16
    n = (2 * mc.FILTER_WG_PER_CU * n_cus + mc.FILTER_WG_PER_CU * n_cus // 2) * sc.TILE + 4099
    ntiles = (n + sc.TILE - 1) // sc.TILE
    for r in (mc.route("lev-L6-k2"), mc.route("subs-L4-k1"), mc.route("cls-L6-k1")):
        case = mc.build(r, n, n_cus, classes_=("tile",))
        assert case.plan == (mc.FILTER_WG_PER_CU * n_cus, mc.FORM_KERNEL, False, []) and ntiles > 2 * case.plan[0]
        mc.check_coverage(case, ("tile",), ntiles)
        for i in case.own:
            assert set(o[1] for o in case.coverage[i]["tile"]["tiles"]) == {0, 1, 2}
        want = mc.sparse_expected(case)
        mc.check_exact_copies_found(case, want)
        if r.mode == "subs":
            assert want == mc.expected(case)


def _raw_rows_by_windows(p, text, k, A):
    """classes_model.raw_rows as its docstring defines it, over window_matches()'s [windows, len(p)] array."""
    m = len(p)
    L = m // (k + 1)
    acc = classes_model.window_matches(p, text, A)
    dist = m - acc.sum(axis=1)
    rows = []
    for g in range(m // L):
        ok = (dist <= k) & acc[:, g * L:g * L + L].all(axis=1)
        rows += [(int(i), int(i) + m, int(dist[i]), g) for i in np.nonzero(ok)[0]]
    return rows


def test_raw_rows_is_the_window_formulation():
    """classes_model.raw_rows sums and ands its columns as vectors over the windows; the definition is the array of
    window_matches().  Random patterns with IUPAC letters (tails behind the last block among them) over texts of n < m,
    n = m, a few windows and a few thousand, with planted spellings, non-base bytes and lower case."""
    rnd = random.Random(19)
    A = sc.iupac_accept()
    rows = 0
    for it in range(300):
        k = rnd.randint(1, 8)
        L = rnd.randint(1, 6)
        m = (k + 1) * L + rnd.randint(0, L - 1)
        p = bytes(rnd.choices(b"ACGTNRYKB", k=m))
        n = rnd.choice([0, 1, m - 1, m, m + 1, 300, 3000])
        t = bytearray(rnd.choices(b"ACGTN\x00a", k=n))
        for _ in range(3):
            if n >= m:
                at = rnd.randint(0, n - m)
                t[at:at + m] = mc.spell(rnd, p)
                if rnd.random() < 0.5:
                    t[at + rnd.randrange(m)] = rnd.choice(b"ACGTn")
        got = classes_model.raw_rows(p, bytes(t), k, A)
        assert got == _raw_rows_by_windows(p, bytes(t), k, A), (it, p, k, n)
        rows += len(got)
    assert rows > 300


@pytest.mark.parametrize("mode", ["lev", "subs", "cls"])
def test_dense_text_rows_lie_around_the_plants(mode):
    """The all-`A` text of the verification kernels' second sweep, at a small CU count: the sparse stream is the oracle's on
    the whole text; exact copies and copies with k edits of both patterns; hits per list beyond 2.2 sweeps."""
    n_cus = 8
    pats, cases = mc.dense_case(mode, n_cus)
    n = len(cases[0].text)
    assert n // sc.TILE // mc.LISTS * sc.TILE > 2.2 * mc.verify_sweep(n_cus) and n // sc.TILE <= mc.FILTER_WG_PER_CU * n_cus
    assert all(p[:6] == b"AAAAAA" and b"A" not in p[6:] for p in pats)
    assert (mode == "cls") == any(c in mc.IUPAC for p in pats for c in p)
    for p, case in zip(pats, cases):
        want = sc.sparse_expected(mode, case)
        assert want == sc.expected(mode, case)
        sc.check_exact_copies_found(mode, case._replace(plants=[pl for pl in case.plants if pl.d == pats.index(p)]), want)
        assert any(row[2] == 2 if mode != "lev" else row[2] > 0 for row in want), "a copy with k edits has its row"
    assert set(pl.start % 16 for pl in cases[0].plants) == set(range(16)) or n < (16 << 16)
    assert np.count_nonzero(cases[0].text != ord("A")) <= 21 * len(cases[0].plants)
    assert _native.MODE_SUBS == mc.MODES["cls"]
