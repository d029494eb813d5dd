"""Shard-cut sweep inputs for every SINGLE-pattern route and form (tests/seam_case.py: ROUTES) and for the linear-programming
routes, and their expected streams.

A sharded sequence hands every hit at global index idx to the ONE shard with own_lo <= idx < own_hi (fz_device.h:
fz_hit_in_range / fz_hit_in_range_s; fz_kernels.h: the tiling of fz_lp_kernel from own_lo, lo / hi of fz_hamming_kernel); the
host checks the halo (fzhip.hip: check_halo), merges the shards' streams and consolidates groups that lie across the cut.  An
off-by-one in any of them duplicates or drops rows only where a hit lies exactly at the cut, so this module puts one there:

    texts(route)             one text per (d, exact / edited): a copy of the route's pattern at cut + d for every d of
                             offsets(route) - seam_case.build's class `first` with the cut for its seam -, quiet background,
                             n = 2 tiles + 301 bytes, cut = 16 384 + 150 (off the 16-byte grid)
    secondary(route)         the named offsets, exact copies, at cuts around the tile seam, at cuts where a shard's buffer
                             clamps at an end of the text, and at the cuts 0 and n where one shard owns nothing
    both_sides(route)        a copy well inside either shard: rows of every block from both shards, for the order of the merge
    shards(n, cut, halo)     the two shards' geometry at the route's MINIMAL halo: m + k for Levenshtein and generic searches
                             and their LP forms, m for substitutions, exact search and subs_lp
    lp_case(route)           a noisy text of 3 x 256 + 77 bytes over four letters for an LP route and the oracle's list on it;
                             the cuts are every position 0 .. n

tests/test_shard_cut_case.py checks the construction on the CPU; tests/test_gpu_shard_cuts.py runs it on the device."""
import collections
import os
import random
import re

import numpy as np

import oracle
from fuzzysearch_amd import _native
from tests import seam_case as sc

N = 2 * sc.TILE + 301
CUT = sc.TILE + 150
ROUTES = sc.ROUTES
LP_STARTS = 256                                       # mirrored from fzhip.hip: kLpStarts (lp_starts())
PLAN = (3, None, False, [])                           # one tile per workgroup: the plan plays no part at a shard cut

CutCase = collections.namedtuple("CutCase", "case cut d exact")
Shard = collections.namedtuple("Shard", "lo hi own_lo own_hi")       # buffer = text[lo:hi], buf_global_off = lo
LpRoute = collections.namedtuple("LpRoute", "name kind m k limits")
LpCase = collections.namedtuple("LpCase", "route pattern text want starts")


def lp_starts():
    """Start positions per window of the LP kernels as fzhip.hip defines them, from its source line."""
    path = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "fzhip.hip")
    with open(path) as f:
        found = re.findall(r"^constexpr uint32_t kLpStarts = (\d+);", f.read(), re.M)
    assert len(found) == 1, found
    return int(found[0])


# -- geometry ----------------------------------------------------------------------------------------------------------------
def halo(route):
    """The smallest halo check_halo accepts for the route's search."""
    return route.m + (route.k if route.kind == "lev" or route.kind[0] == "generic" else 0)


def shards(n, cut, h):
    """Shard A = text[:cut + h] owning [0, cut), shard B = text[cut - h:] owning [cut, n), both clamped to the text."""
    return Shard(0, min(n, cut + h), 0, cut), Shard(max(0, cut - h), n, cut, n)


def buffers(text, cut, h):
    """-> ((bytes, buf_global_off, own_lo, own_hi) of A, the same of B)."""
    return tuple((text[s.lo:s.hi], s.lo, s.own_lo, s.own_hi) for s in shards(len(text), cut, h))


# -- offsets -----------------------------------------------------------------------------------------------------------------
def named_offsets(m, k):
    """Both ends of the verification window, of the copy and of the first block on the cut; the copy halved by it."""
    return sorted(set([-(m + k) - 1, -(m + k), -m - 1, -m, -(m // 2), -1, 0, k, k + 1]))


def blocks(m, k):
    """(L, number of n-gram blocks) of a pattern of m characters with budget k."""
    L = m // (k + 1)
    return L, m // L


def offsets(route):
    """D(route): the whole sweep for m <= 64; for longer patterns (the oracle's verification is quadratic in m) the named
    offsets, every block's index at cut - 1 and at cut, and ten offsets around that for the first and the last block."""
    m, k = route.m, route.k
    if m <= 64:
        return sc.sweep_offsets(m, k)
    L, nb = blocks(m, k)
    out = set(named_offsets(m, k))
    for j in range(nb):
        out |= {-j * L - 1, -j * L}
    for j in (0, nb - 1):
        out |= set(range(-j * L - 8, -j * L + 2))
    assert out <= set(sc.sweep_offsets(m, k))
    return sorted(out)


def edited_too(route):
    return route.copies == 2


# -- texts -------------------------------------------------------------------------------------------------------------------
def _build(route, p, cut, d, exact, n=N):
    """seam_case.build: one copy at cut + d (class `first`, its seam the cut); phase j and j + phases // 2 place the same d as
    an exact and as an edited copy."""
    offs = sc.sweep_offsets(route.m, route.k)
    phase = offs.index(d) + (0 if exact else len(offs))
    assert sc.phases("first", route.m, route.k) == 2 * len(offs)
    case = sc.build(p, route.k, n, 1, "quiet", pattern_alphabet=route.alpha, plan=PLAN,
                    **dict(sc.route_args(route), classes=("first",), first_seam=cut, phase=phase, seed=29 + phase))
    (pl,) = case.plants
    assert pl.d == d and pl.exact == exact and pl.start == cut + d and pl.seam == cut
    return CutCase(case, cut, d, exact)


def _moved(route, p, cut, d, n=N):
    """One exact copy at cut + d, moved into the text where it does not fit (cuts near an end of the text)."""
    bg = sc.Background("quiet", sc.quiet_alphabet(p), 29)
    text = bg.fill(n)
    start = min(max(0, cut + d), n - len(p))
    text[start:start + len(p)] = np.frombuffer(p, dtype=np.uint8)
    plant = sc.Plant(start, p, "first", d, cut, True, True)
    cover = {"first": {"exact": {d}, "edited": set(), "tiles": set(), "seams": {cut}}}
    return CutCase(sc.Case(p, text, [plant], cover, PLAN, 1, route.k, bg), cut, d, True)


def both_sides(route, cut=CUT, n=N):
    """Two exact copies, one owned by either shard, well apart from the cut: both shards hold rows of EVERY block, so the
    merged stream is in the reference's order only if, block by block, A's run comes before B's."""
    p = sc.route_pattern(route)
    bg = sc.Background("quiet", sc.quiet_alphabet(p), 31)
    text = bg.fill(n)
    gap = 2 * (route.m + route.k) + sc.GRAIN
    plants = []
    for start in (cut - gap - route.m, cut + gap):
        text[start:start + len(p)] = np.frombuffer(p, dtype=np.uint8)
        plants.append(sc.Plant(start, p, "first", start - cut, cut, True, True))
    cover = {"first": {"exact": set(pl.d for pl in plants), "edited": set(), "tiles": set(), "seams": {cut}}}
    return CutCase(sc.Case(p, text, plants, cover, PLAN, 1, route.k, bg), cut, plants[0].d, True)


def texts(route, cut=CUT, offs=None, edited=None, n=N):
    """The route's texts for one cut: every d of `offs` (default: offsets(route)) as an exact copy, then - where the route
    plants them, or as `edited` says - as an edited one."""
    p = sc.route_pattern(route)
    offs = offsets(route) if offs is None else offs
    for exact in (True, False) if (edited_too(route) if edited is None else edited) else (True,):
        for d in offs:
            yield _build(route, p, cut, d, exact, n)


def tile_cuts():
    """A's second tile holds nothing but halo (or one byte of its own)."""
    return [sc.TILE - 1, sc.TILE, sc.TILE + 1]


def end_cuts(route, n=N):
    """A buffer clamps at an end of the text: B's at the start, A's at the end."""
    h = halo(route)
    return [1, h - 1, h, h + 1, n - h - 1, n - h, n - h + 1, n - 1]


def empty_cuts(n=N):
    """One shard owns nothing."""
    return [0, n]


def secondary(route, n=N):
    """The reduced set: exact copies only.  Cuts at the tile seam and the cuts 0 and n: the named offsets (at 0 and n the
    copies that do not fit are moved into the text); cuts where a buffer clamps: one copy at d = -(m // 2), moved likewise."""
    p = sc.route_pattern(route)
    for cut in tile_cuts():
        for d in named_offsets(route.m, route.k):
            yield _build(route, p, cut, d, True, n)
    for cut in end_cuts(route, n):
        yield _moved(route, p, cut, -(route.m // 2), n)
    for cut in empty_cuts(n):
        seen = set()
        for d in named_offsets(route.m, route.k):
            c = _moved(route, p, cut, d, n)
            if c.case.plants[0].start not in seen:
                seen.add(c.case.plants[0].start)
                yield c


def split_texts(route):
    """The automatic split of a two-device engine cuts an even text in its middle: the named offsets, exact copies, there,
    and the text with a copy on either side."""
    n = N + 1
    assert n % 2 == 0
    yield from texts(route, n // 2, named_offsets(route.m, route.k), False, n)
    yield both_sides(route, n // 2, n)


def expected(route, cc):
    return sc.sparse_expected(route.kind, cc.case)


def straddling(rows, cut):
    """Rows with start < cut < end."""
    return [r for r in rows if r[0] < cut < r[1]]


def straddling_d(route):
    """The d whose copy lies across the cut, half of it either side."""
    return -(route.m // 2)


# -- coverage ----------------------------------------------------------------------------------------------------------------
def check_coverage(route, cases, want_rows, cut=CUT):
    """The conditions of the main cut, from the plants: the full D as exact copies (and as edited ones where the route plants
    them); every block's index idx_j = cut + d + j * L at cut - 1 and at cut and further off on either side; at least one
    expected row across the cut.  `want_rows`: the expected rows of all the cases together."""
    D = set(offsets(route))
    cover = sc.merge_coverage(c.case.coverage for c in cases)
    assert cover["first"]["exact"] == D, (route.name, "exact copies missing at d =", sorted(D - cover["first"]["exact"])[:8])
    if edited_too(route):
        assert cover["first"]["edited"] == D, (route.name, "edited copies missing at d =", sorted(D - cover["first"]["edited"])[:8])
    assert cover["first"]["seams"] == {cut}
    L, nb = blocks(route.m, route.k)
    starts = sorted(c.case.plants[0].start for c in cases if c.exact)
    assert starts == sorted(cut + d for d in D)
    for j in range(nb):
        rel = set(s + j * L - cut for s in starts)
        assert {-1, 0} <= rel and min(rel) < -1 and max(rel) > 0, (route.name, "block", j, sorted(rel)[:8])
    if route.kind == "exact":
        across = [s for s in want_rows if s < cut < s + route.m]
        assert across or route.m == 1, (route.name, "no expected row across the cut")
    else:
        across = straddling(want_rows, cut)
        assert across, (route.name, "no expected row across the cut")
    return cover, nb, len(across)


def coverage_line(route, cover, nb, across, n_texts):
    c = cover["first"]
    return "shard cut %-22s form %s | %d texts, d %d exact + %d edited, %d blocks at cut - 1 and cut, %d rows across the cut" % (
        route.name, route.form, n_texts, len(c["exact"]), len(c["edited"]), nb, across)


# -- the linear-programming routes -------------------------------------------------------------------------------------------
LP_ROUTES = (
    [LpRoute("lev_lp-%d-%d" % mk, "lev_lp", mk[0], mk[1], None) for mk in ((3, 1), (5, 2), (8, 3))] +
    [LpRoute("subs_lp-%d-%d" % mk, "subs_lp", mk[0], mk[1], None) for mk in ((5, 1), (7, 3))] +
    [LpRoute("generic_lp-%d-%s" % (m, "".join(map(str, lim))), "generic_lp", m, lim[3], lim)
     for (m, lim) in ((7, (2, 1, 1, 2)), (5, (1, 1, 0, 1)))]
)
LP_N = 3 * LP_STARTS + 77


def lp_halo(r):
    return r.m + (0 if r.kind == "subs_lp" else r.k)


def lp_oracle(r, p, t):
    if r.kind == "lev_lp":
        return oracle.lev_lp_raw(p, t, r.k)
    if r.kind == "subs_lp":
        return oracle.subs_lp_raw(p, t, r.k)
    return oracle.generic_lp_raw(p, t, *r.limits)


_lp = {}


def lp_case(r):
    """One noisy text over four letters with copies of the pattern at both ends of the text and across bytes 256 and 512
    (the whole text's window seams), and the oracle's list on the whole text; computed once per route."""
    if r.name not in _lp:
        rnd = random.Random(len(r.name) * 7919 + r.m * 31 + r.k)
        p = bytes(rnd.choice(sc.DNA) for _ in range(r.m))
        t = bytearray(rnd.choice(sc.DNA) for _ in range(LP_N))
        starts = [0, LP_STARTS - r.m // 2, 2 * LP_STARTS - r.m // 2, LP_N - r.m]
        for s in starts:
            t[s:s + r.m] = p
        t = bytes(t)
        _lp[r.name] = LpCase(r, p, t, lp_oracle(r, p, t), starts)
    return _lp[r.name]


def lp_cuts():
    """Every position: every residue mod 256 of shard B's window grid against the whole text's, A's last window of every
    partial length, both degenerate cuts."""
    return range(LP_N + 1)


def check_lp_case(c):
    """The expected list is non-empty, holds a row for every planted copy's start and rows across the cuts; -> cuts with a
    row across them."""
    assert c.want, c.route.name
    starts = set(r[0] for r in c.want)
    if c.route.kind == "subs_lp":
        assert all((s, s + c.route.m, 0) in set(r[:3] for r in c.want) for s in c.starts), c.route.name
    else:
        assert all(any(abs(s - q) <= c.route.k for q in starts) for s in c.starts), c.route.name
    across = [cut for cut in lp_cuts() if any(r[0] < cut < r[1] for r in c.want)]
    assert LP_STARTS in across and 2 * LP_STARTS in across, (c.route.name, len(across))      # (the planted copies')
    return len(across)
