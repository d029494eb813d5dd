"""Seam-sweep inputs for the scan kernel (fz_kernels.h: fz_scan_kernel) and their expected streams.

The kernel's LAYOUT logic - the 16-byte lane row with its 8-byte halo, the 1 KiB wave, the 4 KiB row, the 16 KiB tile, the
queue code and its decoding through the workgroup's tile walk, the two window-prefetch paths, the pipelined tile loop, the
tapered regions, the partial last tile - cannot be compiled for the host.  This module builds texts that put an occurrence
of the pattern at EVERY offset across every kind of seam, and the expected raw stream to hold a search of them against:

    build(...)            -> Case(pattern, text, plants, coverage)
    sparse_expected(...)  -> the complete expected stream of a case on the QUIET background, from oracle runs on small
                             windows around the plants (cost proportional to the plants, not to the text)
    expected(...)         -> the oracle on the whole text (NOISY background)

tests/test_seam_case.py checks the construction on the CPU (sparse stream == full oracle stream, the coverage conditions,
the tile -> workgroup map); tests/test_gpu_scan_seams.py runs the cases on the device.

Sweep: for a pattern of m characters with budget k and a seam at byte S, one copy starts at S + d for every d in
[-(m + k) - 1, k + 1] (sweep_offsets): every n-gram block, every byte of the 8-byte hash window and both ends of the
verification window cross S for some d, and d runs over all residues mod 16 (lane seams).

Classes with many seams (wave, row, tile) take one plant per seam and hold the whole sweep, exact and edited copies, in ONE
text.  Classes with one or a few seams (first: S = 16 384; start; end; region: the first and last tile of every region of the
scan plan) cannot - copies at neighbouring d overlap - so a text holds one plant per such seam and the sweep is spread over
`phases(...)` texts; phase j and phase j + phases // 2 place the same d, exact and edited.
"""
import collections
import ctypes
import os
import random
import re

import numpy as np

import oracle
from fuzzysearch_amd import _native

LANE, WAVE, ROW, TILE = 16, 1024, 4096, 16384        # mirrored from fz_kernels.h (header_layout(); tests/test_seam_case.py)
GRAIN = 256                                           # occupancy granularity: plants keep at least this much apart
CLASSES = ("wave", "row", "tile", "first", "region", "start", "end")
MANY = ("wave", "row", "tile")                        # one text holds the whole sweep

DNA = b"ACGT"
DIGITS = b"0123456789"

Plant = collections.namedtuple("Plant", "start data cls d seam exact whole")
Case = collections.namedtuple("Case", "pattern text plants coverage plan n_cus k bg")


def header_layout():
    """(lane, wave, row, tile) bytes as fz_kernels.h defines them, from its #define lines."""
    path = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "fz_kernels.h")
    with open(path) as f:
        src = f.read()

    def define(name):
        m = re.search(r"^#define %s\s+(.+?)\s*(//.*)?$" % name, src, re.M)
        assert m, name
        return m.group(1).strip()
    threads, rows, bits = int(define("FZ_FILTER_THREADS")), int(define("FZ_FILTER_ROWS")), int(define("FZ_TILE_BITS"))
    assert define("FZ_ROW_BYTES") == "(FZ_FILTER_THREADS * 16)"
    assert define("FZ_TILE_BYTES") == "(FZ_ROW_BYTES * FZ_FILTER_ROWS)"
    assert define("FZ_WAVES_PER_BLOCK") == "(FZ_FILTER_THREADS / 64)"
    assert 1 << bits == threads * 16 * rows
    return 16, 64 * 16, threads * 16, threads * 16 * rows


# -- who scans which tile --------------------------------------------------------------------------------------------------
def scan_plan(p, k, buf_len, n_cus, shares_chip=0):
    """fz_debug_scan_plan -> (grid, form, overlapped, regions as (wg0, nwg, tile0, tile_end)).  The grid and the regions
    depend on the buffer's length, the CU count and `shares_chip` only; the form is that of a Levenshtein search."""
    L = _native.load_library()
    grid, form, n = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    ov = ctypes.c_int(0)
    tab = np.zeros(4 * 8, dtype=np.uint64)
    rc = L.fz_debug_scan_plan(bytes(p), len(p), k, buf_len, n_cus, shares_chip, ctypes.byref(grid), ctypes.byref(form),
                              ctypes.byref(ov), ctypes.byref(n), ctypes.c_void_p(tab.ctypes.data))
    assert rc == 0
    return grid.value, form.value, bool(ov.value), [tuple(int(x) for x in tab[4 * r:4 * r + 4]) for r in range(n.value)]


def tile_owner(T, ntiles, grid, regions):
    """-> (workgroup, iteration, region or -1, iteration is the workgroup's last) of tile T (fz_scan_kernel's walk)."""
    for r, (wg0, nwg, t0, t1) in enumerate(regions):
        if t0 <= T < t1:
            return wg0 + (T - t0) % nwg, (T - t0) // nwg, r, T + nwg >= t1
    return T % grid, T // grid, -1, T + grid >= ntiles


# -- the sweep ---------------------------------------------------------------------------------------------------------------
def sweep_offsets(m, k):
    return list(range(-(m + k) - 1, k + 2))


def edge_items(m, k):
    """start / end classes: whole copies 0 .. k + 1 bytes off the edge (d >= 0) and copies that lost j <= k characters to
    it (d = -j)."""
    return list(range(0, k + 2)) + [-j for j in range(1, k + 1)]


def phases(cls, m, k, n_seams=1):
    """Texts over which the sweep of a few-seam class is spread (exact phases, then as many edited ones)."""
    items = len(edge_items(m, k) if cls in ("start", "end") else sweep_offsets(m, k))
    return 2 * -(-items // max(1, n_seams))


def region_seams(ntiles, regions, n):
    """Both seams of the first and of the last tile of every region."""
    out = set()
    for (_wg0, _nwg, t0, t1) in regions:
        for T in (t0, t0 + 1, t1 - 1, t1):
            if TILE < T * TILE < n:                            # (byte 16 384 is the class `first`)
                out.add(T * TILE)
    return sorted(out)


def edited_copy(rnd, p, k, alphabet, subs_only, limits=None):
    """The pattern with 1 .. k edits (none for k = 0) over `alphabet`; `limits` = (substitutions, insertions, deletions)
    a generic search allows: no kind of edit is applied more often than its limit."""
    v = bytearray(p)
    left = list(limits) if limits else [k, 0 if subs_only else k, 0 if subs_only else k]
    for _ in range(rnd.randint(1, k) if k else 0):
        kinds = [i for i in range(3) if left[i] > 0 and (i != 2 or len(v) > 2)]
        if not kinds:
            break
        op = rnd.choice(kinds)
        left[op] -= 1
        q = rnd.randrange(len(v))
        if op == 0:
            v[q] = rnd.choice([c for c in alphabet if c != v[q]] or list(alphabet))
        elif op == 1:
            v.insert(q, rnd.choice(alphabet))
        else:
            del v[q]
    return bytes(v)


class Background(object):
    """quiet: a fixed block of random symbols the pattern does not contain, repeated; noisy: iid symbols of the pattern's
    own alphabet.  restore() puts the background back where plants were (large texts are built once and re-planted)."""

    def __init__(self, kind, alphabet, seed):
        self.kind, self.seed = kind, seed
        self.alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8)
        self.block = self.alpha[np.random.default_rng(seed).integers(0, len(self.alpha), 65521, dtype=np.uint8)]

    def fill(self, n):
        if self.kind == "quiet":
            return np.resize(self.block, n)
        return self.alpha[np.random.default_rng(self.seed).integers(0, len(self.alpha), n, dtype=np.uint8)]

    def restore(self, text, plants):
        assert self.kind == "quiet"
        for pl in plants:
            idx = np.arange(pl.start, pl.start + len(pl.data)) % len(self.block)
            text[pl.start:pl.start + len(pl.data)] = self.block[idx]


def quiet_alphabet(p):
    """Symbols for the quiet background: digits, or - for patterns that use digits - other bytes the pattern lacks."""
    out = bytes(c for c in DIGITS if c not in p)
    return out if len(out) >= 4 else bytes(c for c in range(0x61, 0x7b) if c not in p)


def build(p, k, n, n_cus, background="quiet", subs_only=False, classes=MANY, phase=0, seed=1, copies=2, shares_chip=0,
          text=None, bg=None, tile_base=0, pattern_alphabet=None, tile_pool=None, limits=None, keep=(), first_seam=None, dry=False,
          plan=None, spell=None):
    """-> Case.  `classes`: which seam classes are planted; `phase`: which slice of the few-seam classes' sweeps (see the
    module docstring); `copies`: 2 = an exact and an edited copy per d for the many-seam classes, 1 = exact only;
    `text` / `bg`: a text built earlier for the same (n, background) whose plants were restored; `tile_base`: byte of the
    text where the device buffer's tile 0 starts; `tile_pool`: the tiles whose seams the class `tile` may use (default:
    all, drawn so that iterations 0, 1 and last occur); `keep`: plants (of other patterns) that `text` holds already -
    they stay, and the case's plant list, which the sparse oracle works from, includes them; `first_seam`: the one seam of
    the class `first` (default: the end of tile 0); `dry`: no text is built, plants and coverage only; `plan`: (grid, form,
    overlapped, regions) of a launch that is not the single-pattern scan's (tests/mp_seam_case.py: the multi-pattern
    filter's) instead of the plan hook's answer; `spell`: (rnd, bytes) -> bytes, applied to every copy on its way into the
    text (a pattern with symbol classes is planted as one of its spellings).  The Case carries the Background, whose
    restore() takes the plants out of the text again."""
    p = bytes(p)
    m = len(p)
    rnd = random.Random(seed * 1000003 + phase)
    alpha = bytes(pattern_alphabet or sorted(set(p)))
    if bg is None:
        bg = Background(background, quiet_alphabet(p) if background == "quiet" else alpha, seed)
    if text is None and not dry:
        text = bg.fill(n)
    assert dry or len(text) == n
    ntiles = (n - tile_base + TILE - 1) // TILE
    grid, form, overlapped, regions = plan or scan_plan(p, k, n - tile_base, n_cus, shares_chip)
    occupied = np.zeros(n // GRAIN + 2, dtype=bool)
    plants = list(keep)
    for pl in keep:
        occupied[max(0, pl.start - GRAIN) // GRAIN:(pl.start + len(pl.data) + GRAIN) // GRAIN + 1] = True
    cover = {c: {"exact": set(), "edited": set(), "tiles": set(), "seams": set()} for c in classes}

    def put(start, data, cls, d, seam, exact, whole=True):
        lo, hi = start, start + len(data)
        if lo < 0 or hi > n or not data:
            return False
        a, b = max(0, lo - GRAIN) // GRAIN, (hi + GRAIN) // GRAIN + 1
        if occupied[a:b].any():
            return False
        occupied[a:b] = True
        if not dry:
            text[lo:hi] = np.frombuffer(data, dtype=np.uint8)
        plants.append(Plant(start, data, cls, d, seam, exact, whole))
        cover[cls]["exact" if exact else "edited"].add(d)
        cover[cls]["seams"].add(seam)
        if cls not in ("start", "end"):
            cover[cls]["tiles"].add(tile_owner((seam - tile_base) // TILE, ntiles, grid, regions))
        return True

    def spelled(data):
        return spell(rnd, data) if spell else data

    def variant(exact):
        return spelled(p if exact else edited_copy(rnd, p, k, alpha, subs_only, limits))

    offs = sweep_offsets(m, k)
    reach = m + 2 * k + 2
    # few-seam classes first: their seams are given
    for cls in classes:
        if cls in MANY:
            continue
        if cls in ("start", "end"):
            items = edge_items(m, k)
            half = phases(cls, m, k) // 2
            d = items[phase % half]
            exact = phase < half
            if d >= 0:
                data = variant(exact)
                ok = put(d if cls == "start" else n - d - len(data), data, cls, d, 0 if cls == "start" else n, exact)
            else:
                data = spelled(p[-d:] if cls == "start" else p[:m + d])
                ok = put(0 if cls == "start" else n - len(data), data, cls, d, 0 if cls == "start" else n, True, whole=False)
            assert ok, (cls, d)
            continue
        seams = [tile_base + TILE if first_seam is None else first_seam] if cls == "first" else [tile_base + s for s in region_seams(ntiles, regions, n - tile_base)]
        if not seams:
            continue
        half = phases(cls, m, k, len(seams)) // 2
        for i, S in enumerate(seams):
            idx = (i * half + phase % half) % len(offs)          # (seams beyond the sweep's need start it again)
            assert put(S + offs[idx], variant(phase < half), cls, offs[idx], S, phase < half), (cls, S, offs[idx])
    # many-seam classes: one plant per seam, the seams spread over the text (the class with the fewest seams first)
    for cls in ("tile", "row", "wave"):
        if cls not in classes:
            continue
        lo_t = (reach + GRAIN) // TILE + 2                      # (tile 1's seam belongs to the class `first`)
        if cls == "tile":
            tiles = np.arange(lo_t, ntiles) if tile_pool is None else np.asarray(tile_pool)
            own = [tile_owner(int(T), ntiles, grid, regions) for T in tiles]
            if tile_pool is None:
                pools = [[int(T) for T, o in zip(tiles, own) if o[1] == 0], [int(T) for T, o in zip(tiles, own) if o[1] == 1],
                         [int(T) for T, o in zip(tiles, own) if o[3] and o[1] > 1], [int(T) for T, o in zip(tiles, own) if o[1] > 1 and not o[3]]]
            else:
                pools = [[int(T) for T in tiles]]
            cand = [[tile_base + T * TILE for T in pool] for pool in pools if pool]
        else:
            unit, coarse = (WAVE, ROW) if cls == "wave" else (ROW, TILE)
            s = np.arange(unit, n - tile_base, unit)
            s = s[(s % coarse != 0) & (s > reach + GRAIN)]
            cand = [[tile_base + int(x) for x in s]]
        need = len(offs) * copies
        # walk every pool with a stride that spreads `need` plants over it
        cursors = [0] * len(cand)
        strides = [max(1, len(c) * len(cand) // (need + 1)) for c in cand]
        restart = [0] * len(cand)
        which = 0
        for c in range(copies):
            for d in offs:
                placed = False
                for _try in range(4 * sum(len(x) for x in cand)):
                    pool = which % len(cand)
                    which += 1
                    if cursors[pool] >= len(cand[pool]):          # the pool's stride is used up: its other seams, one by one
                        restart[pool] += 1
                        cursors[pool], strides[pool] = restart[pool], max(2, strides[pool])
                        if restart[pool] >= len(cand[pool]):
                            continue
                    S = cand[pool][cursors[pool]]
                    cursors[pool] += strides[pool]
                    if S + d < 0 or S + d + m + k > n:
                        continue
                    if put(S + d, variant(c == 0), cls, d, S, c == 0):
                        placed = True
                        break
                assert placed, "no room for %s d = %d: take a longer text" % (cls, d)
    plants.sort()
    return Case(p, text, plants, cover, (grid, form, overlapped, regions), n_cus, k, bg)


# -- expected streams --------------------------------------------------------------------------------------------------------
_iupac = []


def iupac_accept():
    """The acceptance table of fuzzysearch_amd.IUPAC_DNA (tests/classes_model.py), built once."""
    if not _iupac:
        import fuzzysearch_amd
        from tests import classes_model
        _iupac.append(classes_model.accept_table(fuzzysearch_amd.IUPAC_DNA))
    return _iupac[0]


def oracle_fn(kind, p, k):
    """kind: 'lev', 'subs', 'exact', 'cls' (substitutions under the IUPAC classes: the model of tests/classes_model.py) or
    ('generic', max_subs, max_ins, max_dels) -> text bytes -> rows."""
    if kind == "cls":
        from tests import classes_model
        return lambda t: classes_model.raw_rows(p, t, k, iupac_accept())
    if kind == "lev":
        return lambda t: oracle.lev_ngrams_raw(p, t, k)
    if kind == "subs":
        return lambda t: oracle.subs_ngrams_raw(p, t, k)
    if kind == "exact":
        return lambda t: oracle.search_exact(p, t)
    assert kind[0] == "generic"
    return lambda t: oracle.generic_ngrams_raw(p, t, kind[1], kind[2], kind[3], k)


def expected(kind, case):
    return oracle_fn(kind, case.pattern, case.k)(case.text.tobytes())


def sparse_expected(kind, case):
    """The complete expected stream of a case on the quiet background: no n-gram of the pattern occurs outside the plants,
    so every row of the stream depends on the m + 2k + 8 bytes either side of a plant only.  The oracle on every such
    window (overlapping ones merged), rows shifted, stably sorted by block: the reference walks the blocks in its outer
    loop and the text in its inner one."""
    m, k, n = len(case.pattern), case.k, len(case.text)
    W = m + 2 * k + 8
    fn = oracle_fn(kind, case.pattern, k)
    spans = []
    for pl in case.plants:                                     # (sorted by start)
        lo, hi = max(0, pl.start - W), min(n, pl.start + len(pl.data) + W)
        if spans and lo <= spans[-1][1]:
            spans[-1][1] = max(hi, spans[-1][1])
        else:
            spans.append([lo, hi])
    rows = []
    for lo, hi in spans:
        got = fn(case.text[lo:hi].tobytes())
        if kind == "exact":
            rows += [s + lo for s in got]
        else:
            rows += [(s + lo, e + lo, d, g) for (s, e, d, g) in got]
    if kind != "exact":
        rows.sort(key=lambda r: r[3])
    return rows


# -- conditions on the inputs ------------------------------------------------------------------------------------------------
def check_exact_copies_found(kind, case, rows):
    """Every exact, whole copy is in the expected stream."""
    m = len(case.pattern)
    if kind == "exact":
        have = set(rows)
        missing = [pl.start for pl in case.plants if pl.exact and pl.whole and pl.start not in have]
    elif kind in ("lev", "subs", "cls"):
        have = set(r[:3] for r in rows)
        missing = [pl.start for pl in case.plants if pl.exact and pl.whole and (pl.start, pl.start + m, 0) not in have]
    else:
        starts = np.array(sorted(r[0] for r in rows), dtype=np.int64)
        missing = []
        for pl in case.plants:
            if pl.exact and pl.whole:
                i = np.searchsorted(starts, pl.start - case.k)
                if i >= len(starts) or starts[i] > pl.start + m:
                    missing.append(pl.start)
    assert not missing, ("exact copies without a row", missing[:5])
    assert len(rows) > 0


def merge_coverage(covers):
    out = {}
    for cov in covers:
        for cls, c in cov.items():
            o = out.setdefault(cls, {"exact": set(), "edited": set(), "tiles": set(), "seams": set()})
            for key in o:
                o[key] |= c[key]
    return out


def check_coverage(cover, m, k, classes, plan=None, ntiles=None, edited=True):
    """Every class holds every d of its range as an exact copy (and, with k > 0 and `edited`, as an edited one); tile seams
    reach the iterations 0, 1 and last that the plan has; every region's first and last tile is planted."""
    for cls in classes:
        want = set(edge_items(m, k) if cls in ("start", "end") else sweep_offsets(m, k))
        c = cover[cls]
        if cls == "region" and not c["seams"] and plan is not None and not plan[3]:
            continue                                           # a plan without regions has no region edges
        assert c["exact"] == want, (cls, "exact copies missing at d =", sorted(want - c["exact"])[:8])
        if edited and k and cls in MANY:
            assert c["edited"] == set(sweep_offsets(m, k)), (cls, "edited copies missing at d =", sorted(want - c["edited"])[:8])
    if plan is not None and "tile" in classes:
        grid, _form, _ov, regions = plan
        iters = set(o[1] for o in cover["tile"]["tiles"])
        most = max(tile_owner(T, ntiles, grid, regions)[1] for T in range(0, ntiles, max(1, ntiles // 4096)))
        assert 0 in iters and (most < 1 or 1 in iters), sorted(iters)[:8]
        assert any(o[3] for o in cover["tile"]["tiles"]), "no plant in the last tile of a workgroup"
        assert most < 2 or any(o[3] and o[1] >= 2 for o in cover["tile"]["tiles"]), "no plant in a last tile beyond iteration 1"
    if plan is not None and "region" in classes and plan[3]:
        planted = cover["region"]["seams"]
        for (_wg0, _nwg, t0, t1) in plan[3]:
            for T in (t0, t1 - 1):
                if T == 0:
                    continue                                   # (tile 0: the classes `start` and `first`)
                assert T * TILE in planted or (T + 1) * TILE in planted, ("region tile without a plant", T)


def tiles_under(case, plan, classes=("tile",)):
    """The (workgroup, iteration, region, last) of the case's plants of `classes` under another plan of the same buffer
    (the plan of a scan launched behind another one)."""
    ntiles = (len(case.text) + TILE - 1) // TILE
    return set(tile_owner(pl.seam // TILE, ntiles, plan[0], plan[3]) for pl in case.plants if pl.cls in classes)


def size_with_iterations(n_cus, iterations, start):
    """The shortest text of start * 1.5^j bytes whose plan (fz_debug_scan_plan on `n_cus` CUs) gives some workgroup at
    least `iterations` tiles."""
    n = start
    while True:
        grid = scan_plan(b"ACGTACGT", 1, n, n_cus)[0]
        if ((n + TILE - 1) // TILE - 1) // grid >= iterations - 1:
            return n
        n += n // 2


def coverage_line(name, cover, form=None):
    parts = []
    for cls in CLASSES:
        if cls in cover and (cover[cls]["exact"] or cover[cls]["edited"]):
            c = cover[cls]
            its = sorted(set(o[1] for o in c["tiles"]))
            regs = sorted(set(o[2] for o in c["tiles"]) - {-1})
            parts.append("%s %d+%d d%s%s" % (cls, len(c["exact"]), len(c["edited"]),
                                             (" it %d..%d" % (its[0], its[-1])) if its else "", (" reg %s" % regs) if regs else ""))
    return "seams %-28s form %s | %s" % (name, form, "; ".join(parts))


# -- the instantiations of the scan kernel the sweep is run for --------------------------------------------------------------
FORM_NONE, FORM_BAND, FORM_CELLS, FORM_BITS1, FORM_BITS2, FORM_KERNEL, FORM_BITS32 = range(7)
WIDE = b"ACGTNRYK"                                    # 8 symbols: n-grams of 3 - 4 characters stay rare enough for the band forms

Route = collections.namedtuple("Route", "name kind m k alpha form env noisy n classes copies")


def _r(name, kind, m, k, form, alpha=DNA, env=None, noisy=True, classes=MANY, copies=2):
    """n: about 4 MiB, odd; more where the sweep (an exact and an edited copy per d, one plant per tile seam) needs it."""
    n = max(4 << 20, (5 * copies * len(sweep_offsets(m, k)) // 4 + 16) * TILE) + 777
    return Route(name, kind, m, k, alpha, form, env or {}, noisy, n, classes, copies)


ROUTES = (
    # exact search (the hit-emitting scan): one hash window up to 4 bytes, two windows DH = 2 .. 5 bytes apart beyond
    [_r("exact-%d" % m, "exact", m, 0, FORM_NONE, noisy=m >= 5) for m in (1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 300)] +
    # substitutions: Hamming count under the band form's queue discipline ...
    [_r("subs-L%d-k%d" % (m // (k + 1), k), "subs", m, k, FORM_BAND, alpha=WIDE)
     for (m, k) in ((6, 1), (13, 2), (24, 3), (40, 4), (21, 1))] +
    # ... and under the bit-vector forms' (dense candidates expected: WFG 3)
    [_r("subs-dense-%d-%d" % mk, "subs", mk[0], mk[1], FORM_BAND) for mk in ((12, 3), (20, 4))] +
    # Levenshtein, register band
    [_r("band-L%d-k%d" % (m // (k + 1), k), "lev", m, k, FORM_BAND, alpha=WIDE if m // (k + 1) < 6 else DNA)
     for (m, k) in ((8, 1), (12, 1), (20, 1), (12, 2), (20, 2), (30, 2))] +
    [_r("band-nobits-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BAND, env={"FZ_NO_BITS": "1"}, alpha=WIDE) for mk in ((24, 3), (40, 4))] +
    # Levenshtein, bit-vector columns of 32 / 64 / 128 bits
    [_r("bits32-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BITS32) for mk in ((12, 3), (20, 4), (32, 7))] +
    [_r("bits64-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BITS1) for mk in ((33, 5), (54, 8), (64, 15))] +
    [_r("bits128-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BITS2, noisy=mk[1] < 20) for mk in ((65, 10), (128, 31))] +
    # more than 16 blocks: the second launch starts at block 16
    [_r("blocks21-100-20", "lev", 100, 20, FORM_BITS2, noisy=False),
     _r("blocks20-60-19", "lev", 60, 19, FORM_BITS1, noisy=False)] +
    # lane per cell inside the scan, 16 and 32 lanes per candidate
    [_r("cells16-150-5", "lev", 150, 5, FORM_CELLS), _r("cells16-200-7", "lev", 200, 7, FORM_CELLS),
     _r("cells32-260-10", "lev", 260, 10, FORM_CELLS, env={"FZ_WF32": "1"})] +
    # verification in a kernel of its own behind a hit list
    [_r("kernel-140-34", "lev", 140, 34, FORM_KERNEL, noisy=False),
     # (the pattern in HBM.  The oracle's verification is quadratic in m: exact copies on tile seams only - a copy longer than a
     #  wave crosses wave seams wherever it lies)
     _r("kernel-hbm-1030-2", "lev", 1030, 2, FORM_KERNEL, noisy=False, classes=("tile",), copies=1),
     _r("kernel-forced-20-2", "lev", 20, 2, FORM_KERNEL, env={"FZ_FORCE_BIG_VERIFY": "1"}),
     _r("kernel-forced-54-8", "lev", 54, 8, FORM_KERNEL, env={"FZ_FORCE_BIG_VERIFY": "1"})] +
    # generic n-grams: scan + window table + per-hit automaton
    [_r("generic-20", ("generic", 2, 1, 1), 20, 2, FORM_NONE), _r("generic-64", ("generic", 5, 2, 2), 64, 5, FORM_NONE, alpha=WIDE)] +
    # the general slot form of the filter
    [_r("slots-lev-20-2", "lev", 20, 2, FORM_BAND, env={"FZ_NO_SLOT_AND": "1"}),
     _r("slots-exact-8", "exact", 8, 0, FORM_NONE, env={"FZ_NO_SLOT_AND": "1"})]
)


def route_args(route):
    """build()'s arguments that follow from the route's kind."""
    return {"subs_only": route.kind == "subs", "limits": route.kind[1:] if route.kind[0] == "generic" else None,
            "classes": route.classes, "copies": route.copies}


def route_pattern(route, nul=None):
    """The route's pattern: random over its alphabet; `nul` = 'head' / 'tail': two NUL bytes at that end (the zero padding
    around the device buffer must not complete an occurrence)."""
    rnd = random.Random(len(route.name) * 7919 + route.m * 31 + route.k)
    p = bytes(rnd.choice(route.alpha) for _ in range(route.m))
    if nul == "head":
        p = b"\0\0" + p[2:]
    elif nul == "tail":
        p = p[:-2] + b"\0\0"
    return p


EDGE_TAILS = (777, 1, 15, 16, 17)                     # n % 16 384 of the small texts: < one lane row, one row, one byte more


def edge_cases(route, n_cus, p=None, background="quiet", classes=("first", "start", "end"), tail=None, tiles=3):
    """The few-seam classes on small texts (three tiles and a tail): every phase, the tail cycling through EDGE_TAILS (or
    fixed).  Yields the cases; together they hold every d of every class."""
    p = p or route_pattern(route)
    total = max(phases(c, route.m, route.k) for c in classes)
    for ph in range(total):
        n = tiles * TILE + (EDGE_TAILS[ph % len(EDGE_TAILS)] if tail is None else tail)
        yield build(p, route.k, n, n_cus, background, pattern_alphabet=route.alpha, **dict(route_args(route),
                    classes=[c for c in classes if ph < phases(c, route.m, route.k)], phase=ph, seed=11 + ph))
