"""Seam-sweep inputs for the MULTI-PATTERN pass (fz_kernels.h: fz_mp_filter_kernel<DH = 1..5>, fz_mp_verify_kernel,
fz_mp_verify_subs_kernel, fz_mp_verify_cls_kernel and their fz_mp_batch_verify_* twins) and their expected streams, on top
of tests/seam_case.py.

The filter streams the sequence in the scan kernel's layout - a 16-byte lane row with an 8-byte halo, the 1 KiB wave, the
4 KiB row, the 16 KiB tile - but with a launch shape of its own: min(ntiles, 8 x CUs) workgroups, each walking tile,
tile + grid, .. with ONE wave queue carried from tile to tile; the verification kernels are 4 x CUs workgroups whose 16 x CUs
waves walk each of the 16 hit lists 64 candidates at a time.  mp_plan() states the filter's tile walk in the form
seam_case.build(plan=) takes, so that the tile class reaches the iterations 0, 1 and last of THAT walk.

A route is a LIST of patterns that rides one pass (list_of): one carrier per length (all of one n-gram length L, so one
group), per carrier a decoy that shares its block 0 (two table entries under one hash: the filter's `cnt > 1` loop; and a
lane with another length in the wave), one decoy that shares the last carrier's last block, two unrelated patterns.
build() plants the sweep of every carrier into ONE text (seam_case.build(keep=)); the expected stream of EVERY pattern of
the list - carriers and decoys alike - is seam_case.sparse_expected over all plants on the quiet background and the oracle
(lev, subs) or the class model (cls) on the whole text on the noisy one.

tests/test_mp_seam_case.py checks the construction on the CPU; tests/test_gpu_mp_seams.py runs it on the device."""
import collections
import os
import random
import re

import numpy as np

import fuzzysearch_amd
from fuzzysearch_amd import _native, classes
from tests import seam_case as sc

FORM_KERNEL = sc.FORM_KERNEL                          # stats()["verify_form"] of a call whose groups rode a pass
FILTER_WG_PER_CU, VERIFY_WG_PER_CU = 8, 4             # mirrored from fzhip.hip: mp_launch_shard (launch_shape())
LISTS, VERIFY_BATCH, WAVES_PER_WG = 16, 64, 4         # FZ_MP_LISTS; candidates a wave takes at a time; FZ_WAVES_PER_BLOCK
MODES = {"lev": _native.MODE_LEV, "subs": _native.MODE_SUBS, "cls": _native.MODE_SUBS}
IUPAC = fuzzysearch_amd.IUPAC_DNA
LETTERS = b"RYSWKMBDHVN"

Route = collections.namedtuple("Route", "name mode k lengths alpha")
Case = collections.namedtuple("Case", "route patterns text plants own coverage plan n_cus k bg")


def launch_shape():
    """(filter workgroups per CU, verification workgroups per CU) as mp_launch_shard launches them, from its source lines."""
    path = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "fzhip.hip")
    with open(path) as f:
        src = f.read()
    src = src[src.index("static int mp_launch_shard("):src.index("static int mp_launch_group(")]
    grid = re.findall(r"const uint32_t grid = \(uint32_t\)std::min<uint64_t>\(ntiles, \(uint64_t\)d\.n_cus \* (\d+)\);", src)
    assert len(grid) == 1 and "hipLaunchKernelGGL(fk, dim3(grid), dim3(FZ_FILTER_THREADS)" in src, grid
    verify = re.findall(r"_kernel, dim3\(\(uint32_t\)d\.n_cus \* (\d+)\), dim3\(FZ_FILTER_THREADS\)", src)
    assert len(verify) == 3 and len(set(verify)) == 1, verify      # lev, subs, cls: each line launches its batch twin too
    return int(grid[0]), int(verify[0])


def mp_plan(n, n_cus):
    """The filter's tile walk over a buffer of n bytes as seam_case.build(plan=) takes it: (grid, form, overlapped, regions)."""
    ntiles = (n + sc.TILE - 1) // sc.TILE
    return (min(ntiles, FILTER_WG_PER_CU * n_cus), FORM_KERNEL, False, [])


def verify_sweep(n_cus):
    """Hits of ONE list that the verification launch takes per sweep: 64 per wave, 4 waves per workgroup."""
    return VERIFY_WG_PER_CU * n_cus * WAVES_PER_WG * VERIFY_BATCH


# -- routes ------------------------------------------------------------------------------------------------------------------
def _routes():
    out = []
    # (L, k, lengths): every filter instance DH = 1 .. 5, L > 8 (bytes beyond the hashed 8: the verification's n-gram test),
    # k = FZ_MP_MAX_K and m = FZ_MP_MAX_M, nine blocks per pattern
    shapes = [(4, 1, (8, 9)), (5, 2, (15, 16, 17)), (6, 2, (18, 19, 20)), (7, 3, (28, 29, 30, 31)), (8, 3, (32, 33, 34, 35)),
              (14, 8, (126, 127, 128)), (4, 8, (36, 37, 38, 39))]
    for mode in ("lev", "subs"):
        for (L, k, lengths) in shapes:
            assert all(m // (k + 1) == L for m in lengths)
            # (L <= 5: the wide alphabet keeps a noisy background sparse enough for the oracle; every route is run on a noisy
            #  background too: each has L >= 6 or that alphabet - the class lists' budgets are small for the model's sake)
            out.append(Route("%s-L%d-k%d" % (mode, L, k), mode, k, lengths, sc.WIDE if L <= 5 else sc.DNA))
    # symbol classes: L = 4, 6, 8, 14; the lengths hit every residue m % 4 (12, 13, 34, 35); budgets kept small - the class
    # model is numpy over every window of the text
    for (L, k, lengths) in ((4, 1, (8, 9)), (6, 1, (12, 13)), (8, 3, (34, 35)), (14, 1, (28, 29))):
        assert all(m // (k + 1) == L for m in lengths)
        out.append(Route("cls-L%d-k%d" % (L, k), "cls", k, lengths, sc.DNA))
    assert set(m % 4 for r in out if r.mode == "cls" for m in r.lengths) == {0, 1, 2, 3}
    return out


ROUTES = _routes()


def route(name):
    return next(r for r in ROUTES if r.name == name)


def dh(L):
    """fz_device.h: fz_mp_dh - the filter instance of an n-gram length."""
    return min(L, 8) - 3


def class_positions(m, k, i):
    """Where carrier i of a class route holds its IUPAC letters (tests/test_gpu_classes.py::_class_patterns): position 0, the
    last position, inside a block's hashed bytes, at block offset >= 8 (L > 8), the tail behind the last block."""
    L = m // (k + 1)
    tail = list(range((m // L) * L, m))
    wheres = [[0, L + 1, m - 1], [L + min(L, 8) - 1, 2 * L - 1] + tail[-2:]]
    if L > 8:
        wheres = [[0, L + 9, m - 1], [8, L + 1, 2 * L - 1] + tail[-2:]]
    return sorted(set(wheres[i % len(wheres)]))


def list_of(r):
    """-> (patterns, carriers): the route's list and the positions of its carriers in it."""
    rnd = random.Random(len(r.name) * 7919 + r.k * 131 + sum(r.lengths))
    alpha = bytes(r.alpha)

    def rand(n):
        return bytes(rnd.choice(alpha) for _ in range(n))

    def differing(src):
        return bytes(rnd.choice([c for c in alpha if c != x]) for x in src)

    L = r.lengths[0] // (r.k + 1)
    carriers = []
    for i, m in enumerate(r.lengths):
        p = bytearray(rand(m))
        if r.mode == "cls":
            for q in class_positions(m, r.k, i):
                p[q] = rnd.choice(LETTERS)
        carriers.append(bytes(p))
    pats = list(carriers)
    for i, c in enumerate(carriers):                          # block 0 of the carrier, another length, no other block of it
        m = r.lengths[(i + 1) % len(r.lengths)]
        pats.append(c[:L] + differing((c[L:] + c)[:m - L]))
    c = carriers[-1]                                          # the last carrier's last block, in its place, nothing else of it
    g = (len(c) // L - 1) * L
    pats.append(differing(c[:g]) + c[g:g + L] + differing(c[g + L:]))
    pats += [rand(r.lengths[0]), rand(r.lengths[-1])]
    return pats, list(range(len(carriers)))


def tables():
    return classes.class_tables(IUPAC)


def one_group(r, pats):
    """The whole list is one group of a pass (FZ_MP_FORCE_PASS set for lev and subs: gpu_cases.force_pass; class lists
    always ride)."""
    if r.mode == "cls":
        group_of, _per_pat, per_group = _native.multi_plan_classes(pats, r.k, tables())
        return group_of == [0] * len(pats) and len(per_group) == 1
    return _native.multi_plan(pats, r.k, MODES[r.mode]) == ([0] * len(pats), 1)


def spell(rnd, data):
    """A spelling of a copy of a class pattern: every IUPAC letter replaced by a member of its set."""
    return bytes(rnd.choice(IUPAC[c]) if c in IUPAC else c for c in data)


def text_bytes(r, copies=2, classes_=sc.MANY):
    """seam_case._r's rule summed over the carriers: about 4 MiB, odd; more where the sweeps need more tile seams.  Without
    the tile class (the CPU's check of the sparse stream): no floor, and a tile for every three plants of the row class."""
    plants = sum(copies * len(sc.sweep_offsets(m, r.k)) for m in r.lengths)
    if "tile" not in classes_:
        return (5 * plants // 12 + 16) * sc.TILE + 777
    need = sum(5 * copies * len(sc.sweep_offsets(m, r.k)) // 4 + 16 for m in r.lengths)
    return max(4 << 20, need * sc.TILE) + 777


def build(r, n, n_cus, background="quiet", classes_=sc.MANY, phase=0, seed=1, copies=2, text=None, bg=None, specs=None, plan=None):
    """-> Case: the sweep of every carrier of the route planted into one text.  `specs`: instead of `classes_` / `phase` for
    every carrier, a list of (carrier, classes, phase, first_seam) - seam_case.build's arguments of those names.  `plants`:
    all of them, sorted; `own[i]`: carrier i's; `coverage[i]`: carrier i's, under the multi-pattern plan."""
    pats, carriers = list_of(r)
    plan = plan or mp_plan(n, n_cus)
    plants, own, cover = [], {}, {}
    for j, (i, cl, ph, first_seam) in enumerate(specs if specs is not None else [(i, classes_, phase, None) for i in carriers]):
        # (the quiet background is digits for every pattern of every route: no pattern symbol, no member of an IUPAC set)
        case = sc.build(pats[i], r.k, n, n_cus, background, subs_only=r.mode != "lev", classes=cl, phase=ph, seed=seed * 31 + j,
                        copies=copies, text=text, bg=bg, pattern_alphabet=r.alpha, keep=plants, first_seam=first_seam, plan=plan,
                        spell=spell if r.mode == "cls" else None)
        own[i] = sorted(set(own.get(i, [])) | (set(case.plants) - set(plants)))
        cover[i] = sc.merge_coverage([cover[i], case.coverage]) if i in cover else case.coverage
        plants, text, bg = case.plants, case.text, case.bg
    return Case(r, pats, text, plants, own, cover, plan, n_cus, r.k, bg)


def _as_seam_case(case, p, plants=None):
    return sc.Case(p, case.text, case.plants if plants is None else plants, None, case.plan, case.n_cus, case.k, case.bg)


def sparse_expected(case):
    """The complete expected stream of every pattern of the list on the quiet background."""
    return [sc.sparse_expected(case.route.mode, _as_seam_case(case, p)) for p in case.patterns]


def expected(case):
    """The oracle / the class model on the whole text, for every pattern of the list."""
    t = case.text.tobytes()
    return [sc.oracle_fn(case.route.mode, p, case.k)(t) for p in case.patterns]


def check_exact_copies_found(case, want):
    for i, plants in case.own.items():
        if any(pl.exact and pl.whole for pl in plants):      # (an edge text may hold nothing but a cut copy of a carrier)
            sc.check_exact_copies_found(case.route.mode, _as_seam_case(case, case.patterns[i], plants), want[i])


def check_coverage(case, classes_, ntiles=None, cover=None):
    """seam_case.check_coverage for every carrier planted, under the multi-pattern plan."""
    for i in case.own:
        sc.check_coverage((cover or case.coverage)[i], len(case.patterns[i]), case.k, classes_, case.plan, ntiles)


def check_edge_coverage(cover, m, k):
    """The few-seam classes of one carrier over all the texts of edge_cases() / of a shard-cut sweep: every d as an exact copy
    (seam_case.check_coverage) AND as an edited one - `first`: every d of the sweep; `start`, `end`: every whole copy
    (d >= 0; a copy that lost characters to the edge is planted as it is, in both halves of the phases)."""
    sc.check_coverage(cover, m, k, [c for c in ("first", "start", "end") if c in cover])
    if k:
        if "first" in cover:
            assert cover["first"]["edited"] == set(sc.sweep_offsets(m, k)), ("first", "edited copies", sorted(cover["first"]["edited"])[:8])
        for cls in ("start", "end"):
            if cls in cover:
                assert cover[cls]["edited"] == set(d for d in sc.edge_items(m, k) if d >= 0), (cls, "edited copies", sorted(cover[cls]["edited"]))


def merge_coverage(cases):
    return {i: sc.merge_coverage(c.coverage[i] for c in cases if i in c.coverage) for i in set(i for c in cases for i in c.coverage)}


def coverage_line(case, cover=None):
    r = case.route
    L = r.lengths[0] // (r.k + 1)
    per = ["m %d: %s" % (len(case.patterns[i]), sc.coverage_line("", (cover or case.coverage)[i]).split("| ")[1]) for i in sorted(case.own)]
    return "mp seams %-12s L %d DH %d, %d patterns, grid %d | %s" % (r.name, L, dh(L), len(case.patterns), case.plan[0], " | ".join(per))


def edge_phases(r):
    """Texts that edge_cases() needs: every carrier's `first` sweep side by side, the `start` / `end` items carrier by carrier."""
    nc = len(r.lengths)
    return max(max(sc.phases("first", m, r.k) for m in r.lengths), nc * sc.phases("start", r.lengths[0], r.k))


def edge_cases(r, n_cus, background="quiet"):
    """The few-seam classes on small texts, one text per phase: carrier i's `first` sweep across the seam behind tile i (the
    carriers side by side), the `start` and `end` items of one carrier per text, in turn; a tile and a tail behind the last
    of those seams, the tail cycling through seam_case.EDGE_TAILS.  Together the texts hold every d of every class for every
    carrier."""
    nc = len(r.lengths)
    for ph in range(edge_phases(r)):
        n = (nc + 2) * sc.TILE + sc.EDGE_TAILS[ph % len(sc.EDGE_TAILS)]
        specs = [(i, ("first",), ph, (i + 1) * sc.TILE) for i, m in enumerate(r.lengths) if ph < sc.phases("first", m, r.k)]
        if ph // nc < sc.phases("start", r.lengths[0], r.k):
            specs.append((ph % nc, ("start", "end"), ph // nc, None))
        yield build(r, n, n_cus, background, specs=specs, seed=11 + ph)


# -- the second sweep of the verification kernels ----------------------------------------------------------------------------
def k_edits(rnd, p, k, subs_only):
    """p (no `A` behind its first block) with exactly k edits behind the first block's six bytes, each of which brings an `A`
    or takes a byte away: k substitutions at k positions, or a substitution, an insertion, a deletion in turn."""
    v = bytearray(p)
    if subs_only:
        for q in rnd.sample(range(6, len(v)), k):
            v[q] = ord("A")
        return bytes(v)
    for j in range(k):
        q = rnd.randrange(6, len(v))
        if j % 3 == 0:
            v[q] = ord("A")
        elif j % 3 == 1:
            v.insert(q, ord("A"))
        else:
            del v[q]
    return bytes(v)


def dense_case(mode, n_cus, seed=7):
    """A text of nothing but `A` in which every offset is a hit of every pattern of the list (block 0 = AAAAAA, then 14
    bases that are not A; the class list: one IUPAC letter among them that does not accept A), k = 2: long enough for more
    than 2.2 sweeps of the verification launch per hit list, one tile per filter workgroup (the lists balanced by
    blockIdx.x % 16).  An exact copy and one with k edits every 64 KiB, the patterns in turn.  No window of `A`s is within k of
    a pattern, so every row lies around a plant: seam_case.sparse_expected holds.  -> (patterns, sc.Case per pattern; a plant's
    `d` is the number of the pattern it is a copy of)."""
    k, m = 2, 20
    rnd = random.Random(seed)
    ntiles = LISTS * (int(2.3 * verify_sweep(n_cus) / sc.TILE) + 1)
    assert ntiles // LISTS * sc.TILE > 2.2 * verify_sweep(n_cus) and ntiles <= FILTER_WG_PER_CU * n_cus, ntiles
    n = ntiles * sc.TILE
    pats = []
    for _ in range(2):
        p = bytearray(b"AAAAAA" + bytes(rnd.choice(b"CGT") for _ in range(m - 6)))
        if mode == "cls":
            p[rnd.randrange(6, m)] = rnd.choice(b"YSKB")
        pats.append(bytes(p))
    text = np.full(n, ord("A"), dtype=np.uint8)
    plants = []
    for j, at in enumerate(range(1 << 15, n - (1 << 15), 1 << 16)):
        p = pats[(j // 2) % len(pats)]
        exact = j % 2 == 0
        v = p if exact else k_edits(rnd, p, k, mode != "lev")
        if mode == "cls":
            v = spell(rnd, v)
        start = at + j % 61                                     # (every residue mod 16 among them)
        text[start:start + len(v)] = np.frombuffer(v, dtype=np.uint8)
        plants.append(sc.Plant(start, v, "dense", (j // 2) % len(pats), at, exact, True))          # (d: the pattern it is a copy of)
    return pats, [sc.Case(p, text, plants, None, mp_plan(n, n_cus), n_cus, k, None) for p in pats]
