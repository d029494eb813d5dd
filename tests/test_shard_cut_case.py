"""tests/shard_cut_case.py on the CPU: the licence for holding two shards against the SPARSE expected stream of the whole text
(sparse stream == oracle on the whole text, on a sample of texts per kind), the coverage conditions of the main cut for every
route, the shard buffers as slices of the text, and the LP cases' expected lists (they are conditions, not measurements)."""
import pytest

from tests import seam_case as sc
from tests import shard_cut_case as cc

BY_NAME = dict(ids=lambda r: r.name)


def test_constants_mirror_the_sources():
    assert cc.lp_starts() == cc.LP_STARTS == 256
    assert cc.N == 2 * sc.TILE + 301 and cc.CUT == sc.TILE + 150 and cc.CUT % 16
    assert cc.LP_N == 3 * 256 + 77


def test_the_full_sweeps_add_up():
    """One text per (d, exact or edited): 2 340 texts over the routes with m <= 64."""
    short = [r for r in cc.ROUTES if r.m <= 64]
    assert all(cc.edited_too(r) for r in short)
    assert sum(2 * len(cc.offsets(r)) for r in short) == 2340
    for r in cc.ROUTES:
        if r.m > 64:
            L, nb = cc.blocks(r.m, r.k)
            D = set(cc.offsets(r))
            assert set(cc.named_offsets(r.m, r.k)) <= D
            assert all({-j * L - 1, -j * L} <= D for j in range(nb))
            assert all(set(range(-j * L - 8, -j * L + 2)) <= D for j in (0, nb - 1))


def test_minimal_halo_per_kind():
    for r in cc.ROUTES:
        assert cc.halo(r) == (r.m + r.k if r.kind == "lev" or r.kind[0] == "generic" else r.m)
        assert r.kind in ("lev", "subs", "exact") or r.kind[0] == "generic"
    for r in cc.LP_ROUTES:
        assert cc.lp_halo(r) == (r.m if r.kind == "subs_lp" else r.m + r.k)


@pytest.mark.parametrize("route", cc.ROUTES, **BY_NAME)
def test_main_cut_coverage_and_buffers(route):
    """Every text of the main cut: the plant lies at cut + d; the coverage conditions hold over the route's texts (every d of
    D as an exact and - where planted - as an edited copy, every block's index at cut - 1 and at cut and on both sides, rows
    across the cut); the shard buffers are the stated slices of the text."""
    cases = list(cc.texts(route))
    rows = []
    h = cc.halo(route)
    for c in cases:
        want = cc.expected(route, c)
        if c.exact:
            sc.check_exact_copies_found(route.kind, c.case, want)
        rows += want
        text = c.case.text.tobytes()
        (a, a_off, a_lo, a_hi), (b, b_off, b_lo, b_hi) = cc.buffers(text, c.cut, h)
        assert a == text[:cc.CUT + h] and (a_off, a_lo, a_hi) == (0, 0, cc.CUT)
        assert b == text[cc.CUT - h:] and (b_off, b_lo, b_hi) == (cc.CUT - h, cc.CUT, cc.N)
    assert len(cases) == len(cc.offsets(route)) * (2 if cc.edited_too(route) else 1)
    cover, nb, across = cc.check_coverage(route, cases, rows)
    print(cc.coverage_line(route, cover, nb, across, len(cases)))


@pytest.mark.parametrize("route", cc.ROUTES, **BY_NAME)
def test_sparse_stream_is_the_full_oracle_stream(route):
    """A sample of the texts of every kind - main cut exact and edited (the named offsets), the tile-seam cuts, the clamped
    buffers, the cuts 0 and n, the automatic split's even text: the sparse expected stream is the oracle's on the whole text,
    order included.  (kernel-hbm-1030-2, whose oracle is quadratic in m: one text per kind.)"""
    named = cc.named_offsets(route.m, route.k)
    few = route.m > 300
    sample = list(cc.texts(route, offs=named[4:5] if few else named))
    sec = list(cc.secondary(route))
    sample += sec[::9] + sec[-2:] if few else sec
    sample += list(cc.split_texts(route))[:1 if few else None]
    kinds = set()
    for c in sample:
        assert cc.expected(route, c) == sc.expected(route.kind, c.case), (route.name, c.cut, c.d, c.exact)
        kinds.add((c.cut, c.exact))
    cuts = set(cut for cut, _exact in kinds)
    assert (cc.CUT, True) in kinds and ((cc.CUT, False) in kinds) == cc.edited_too(route) and (cc.N + 1) // 2 in cuts
    assert cuts & set(cc.tile_cuts()) and cuts & set(cc.end_cuts(route)) and cuts & set(cc.empty_cuts())
    if not few:
        assert cuts >= set(cc.tile_cuts() + cc.end_cuts(route) + cc.empty_cuts())


@pytest.mark.parametrize("route", cc.ROUTES, **BY_NAME)
def test_secondary_cuts(route):
    """The reduced set: the cuts' values, exact copies only, every copy inside the text, the buffers clamped to it; a shard
    that owns nothing at the cuts 0 and n."""
    h = cc.halo(route)
    sec = list(cc.secondary(route))
    cuts = [c.cut for c in sec]
    assert set(cuts) == set(cc.tile_cuts() + cc.end_cuts(route) + cc.empty_cuts())
    assert set(cc.end_cuts(route)) == {1, h - 1, h, h + 1, cc.N - h - 1, cc.N - h, cc.N - h + 1, cc.N - 1}
    named = cc.named_offsets(route.m, route.k)
    for cut in cc.tile_cuts():
        assert [c.d for c in sec if c.cut == cut] == named
    for cut in cc.end_cuts(route):                                 # (m = 1: the cut halo - 1 is the cut 0 as well)
        assert -(route.m // 2) in [c.d for c in sec if c.cut == cut]
    for c in sec:
        (pl,) = c.case.plants
        assert c.exact and pl.data == c.case.pattern and 0 <= pl.start and pl.start + route.m <= cc.N
        assert c.case.text[pl.start:pl.start + route.m].tobytes() == c.case.pattern
        a, b = cc.shards(cc.N, c.cut, h)
        assert a == (0, min(cc.N, c.cut + h), 0, c.cut) and b == (max(0, c.cut - h), cc.N, c.cut, cc.N)
        assert (a.own_hi == a.own_lo) == (c.cut == 0) and (b.own_hi == b.own_lo) == (c.cut == cc.N)
    for cut in cc.empty_cuts():
        assert len([c for c in sec if c.cut == cut]) >= 2       # (the copies moved into the text: at its edge, and k, k + 1 off it)


@pytest.mark.parametrize("route", cc.ROUTES, **BY_NAME)
def test_both_sides(route):
    """The text with a copy well inside either shard: sparse == oracle on the whole text, and every block has rows that
    shard A owns and rows that shard B owns (the merge has to put A's run first)."""
    c = cc.both_sides(route)
    want = cc.expected(route, c)
    assert want == sc.expected(route.kind, c.case)
    sc.check_exact_copies_found(route.kind, c.case, want)
    L, nb = cc.blocks(route.m, route.k)
    if route.kind == "exact":
        assert min(want) < c.cut <= max(want)
    else:
        for g in range(nb):
            idx = [row[0] for row in want if row[3] == g]
            assert idx and min(idx) + route.m + route.k < c.cut < max(idx) - route.k, (route.name, "block", g)
    assert all(abs(pl.start - c.cut) > cc.halo(route) + route.m for pl in c.case.plants)


@pytest.mark.parametrize("r", cc.LP_ROUTES, **BY_NAME)
def test_lp_cases(r):
    """The oracle's list on the whole text: non-empty, a row at every planted copy, rows across the cuts at bytes 256 and 512
    (and across as many others as the noise gives); the cuts are every position 0 .. n."""
    c = cc.lp_case(r)
    assert len(c.text) == cc.LP_N and len(c.pattern) == r.m and set(c.text) <= set(sc.DNA)
    assert all(c.text[s:s + r.m] == c.pattern for s in c.starts)
    assert c.starts[0] == 0 and c.starts[-1] + r.m == cc.LP_N
    assert c.starts[1] < cc.LP_STARTS < c.starts[1] + r.m and c.starts[2] < 2 * cc.LP_STARTS < c.starts[2] + r.m
    across = cc.check_lp_case(c)
    assert list(cc.lp_cuts()) == list(range(cc.LP_N + 1))
    assert set(cut % cc.LP_STARTS for cut in cc.lp_cuts()) == set(range(cc.LP_STARTS))     # (B's windows start at own_lo = cut)
    print("lp shard cut %-20s | %d bytes, %d rows, %d of %d cuts with a row across them" % (r.name, cc.LP_N, len(c.want), across, cc.LP_N + 1))


def test_lp_route_set():
    assert [(r.kind, r.m, r.k) for r in cc.LP_ROUTES if r.kind != "generic_lp"] == [
        ("lev_lp", 3, 1), ("lev_lp", 5, 2), ("lev_lp", 8, 3), ("subs_lp", 5, 1), ("subs_lp", 7, 3)]
    assert [(r.m, r.limits) for r in cc.LP_ROUTES if r.kind == "generic_lp"] == [(7, (2, 1, 1, 2)), (5, (1, 1, 0, 1))]
