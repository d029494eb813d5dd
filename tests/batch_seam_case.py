"""Seam-sweep inputs for the RAGGED kernel instances (fz_kernel_bodies.inc compiled with RAG = true: batch_scan_kernel and
the fz_batch_verify_* kernels behind fz_batch_search) and their expected streams.

tests/seam_case.py puts a copy of the pattern at every offset across the seams of the scan kernel's LAYOUT; here the seams
are those BETWEEN THE SEQUENCES of a batch, where every verification form clamps its window to [sa, se) in code of its own:

    build(route, cls, ...)    -> (sequences, plants, coverage)     one batch that holds a whole sweep of one seam class
    batches(route)            -> every batch of a route: (cls, sequences, plants, coverage)
    expected(mode, p, seqs, k, cache) -> (raw rows, reduced rows): the oracle PER SEQUENCE, the only reference
    seam_blind / clamped_one_side     -> what a kernel that ignores the seams, or one of the two clamps, would return:
                                         the construction test holds the inputs against them (tests/test_batch_seam_case.py)

For a seam at packed offset S between the sequences A and B an exact and an edited copy (seam_case.edited_copy) start at S + d,
d over seam_case.sweep_offsets(m, k) = [-(m + k) - 1, k + 1]; for -len < d < 0 the copy is cut: its head is A's tail and its
rest B's head.  Every d has a pair (A, B) of its own, the background is quiet (seam_case.quiet_alphabet: no symbol of the
pattern), so a row of the expected stream can only come from a plant.

Classes: `mid` (S mod 16 takes all 16 values over the sweep), `tile` (a filler sequence in front of the pair puts S on a
multiple of 16 384 - fz_ragged_first's `ends[j] <= t << 14` - and, for the straddling subset, one byte to either side:
`tile-1`, `tile+1`), `empty1` / `empty3` (one and three empty sequences between A and B: equal ends[]), `short` (triples
A|M|B with |M| in short_lengths(): both clamps bind in one window), `first` / `last` (a copy flush at byte 0 of sequence 0
and at the end of the last sequence, the packed length mod 16 384 over seam_case.EDGE_TAILS).

Routes with m + k <= 200 run the full sweep in `mid` and `tile` and the straddling subset elsewhere; longer ones the subset
everywhere.  The two routes with k >= 256 (fz_batch_verify_big_kernel<16> beyond 512 band cells and <32>: no smaller budget
selects them, and the reference's verification is (k + 1) m (m + k) cells per copy - 10^8 and more) run
trimmed (TIER2 in the functions below), between sequences that end 8 bytes around the copy (both clamps bind in every
window, and the oracle's windows stay short): k = 256 every class, each a test of its own - `mid` d = -m, -(m / 2), 0; `tile`
(on the tile only), `empty` (one empty sequence): d = -(m / 2); `short`: |M| = m; `first` / `last`: the tail of 777 bytes -;
k = 512 (2.7 s of oracle per whole copy): `mid` with d = -(m / 2) and 0."""
import collections
import random

import numpy as np

import oracle
from tests import seam_case as sc

TILE = sc.TILE
EXACT, LEV, SUBS = 0, 1, 2
MODE = {"exact": EXACT, "lev": LEV, "subs": SUBS}
HEAVY = 10 ** 7

Plant = collections.namedtuple("Plant", "start data cls d seam exact")

# -- routes ----------------------------------------------------------------------------------------------------------------
WIDE128 = bytes(range(128, 256))                      # patterns whose n-grams are one or two characters: every n-gram occurs once
NOT_DIGITS = bytes(c for c in range(1, 256) if c not in sc.DIGITS)[:200]


def _from_scan_sweep():
    keep = ("exact-", "subs-", "band-", "bits32-", "bits64-", "bits128-", "blocks2", "cells16-", "kernel-140-34", "kernel-forced-")
    return [r for r in sc.ROUTES if r.name.startswith(keep)]


ROUTES = _from_scan_sweep() + [
    # the pattern in HBM for the exact route's confirmation (fz_confirm: a.pat_g)
    sc._r("exact-1030", "exact", 1030, 0, sc.FORM_NONE, noisy=False),
    # the fused 32-lane form: taken without a switch for dense patterns (two symbols)
    sc._r("cells32-dense-150-8", "lev", 150, 8, sc.FORM_CELLS, alpha=b"AC"),
    # the stand-alone ragged kernels
    sc._r("ring-band-300-2", "lev", 300, 2, sc.FORM_KERNEL, noisy=False),           # fz_batch_verify_kernel, register band
    sc._r("ring-subs-300-10", "subs", 300, 10, sc.FORM_KERNEL, noisy=False),        # fz_batch_verify_kernel, substitutions
    sc._r("wf32-150-8", "lev", 150, 8, sc.FORM_KERNEL, alpha=NOT_DIGITS),            # fz_batch_verify_wf_kernel<32>: rare candidates
    sc._r("wf64-140-20", "lev", 140, 20, sc.FORM_KERNEL),                            # fz_batch_verify_wf_kernel<64>
    sc._r("wf16-150-5", "lev", 150, 5, sc.FORM_KERNEL, env={"FZ_NO_WF_FUSE": "1"}),  # fz_batch_verify_wf_kernel<16>: under the switch only
    sc._r("big1-1030-2", "lev", 1030, 2, sc.FORM_KERNEL, noisy=False),              # fz_batch_verify_big_kernel<1>
    sc._r("big1-subs-1030-2", "subs", 1030, 2, sc.FORM_KERNEL, noisy=False),
    # ... with more than one band cell per lane, on short patterns under FZ_FORCE_BIG_VERIFY=1 (m + k just beyond 200: the subset)
    sc._r("big2-forced-170-32", "lev", 170, 32, sc.FORM_KERNEL, env={"FZ_FORCE_BIG_VERIFY": "1"}),                  # 2k + 1 = 65 cells
    sc._r("big4-forced-136-65", "lev", 136, 65, sc.FORM_KERNEL, alpha=WIDE128, env={"FZ_FORCE_BIG_VERIFY": "1"}),   # 131 cells
    sc._r("big16-forced-129-128", "lev", 129, 128, sc.FORM_KERNEL, alpha=WIDE128, env={"FZ_FORCE_BIG_VERIFY": "1"}),  # 257 cells: <16> in a batch, <8> in memory
    # ... and budgets beyond FZ_MAX_K, which need no switch
    sc._r("big16-257-256", "lev", 257, 256, sc.FORM_KERNEL, alpha=WIDE128, noisy=False),    # 513 cells
    sc._r("big32-513-512", "lev", 513, 512, sc.FORM_KERNEL, alpha=NOT_DIGITS, noisy=False), # 1025 cells
]

# noisy batches (noisy() below): every fused form, and fz_batch_verify_wf_kernel<64> on either side of FZ_WF_COMPACT_MIN
WF_COMPACT_MIN = 8192                                 # fz_kernels.h: FZ_WF_COMPACT_MIN
NOISY_ROUTES = [(name, 3, None) for name in ("subs-L6-k3", "subs-dense-20-4", "band-L6-k2", "bits32-20-4", "bits64-54-8",
                                             "bits128-65-10", "cells16-150-5", "cells32-dense-150-8")] + [
    ("wf64-140-20", 3, "slotted"),                    # few n-gram hits: a record slot per hit
    ("wf64-dense-140-20", 4, "compact"),              # two symbols: more than WF_COMPACT_MIN hits, records appended
]
EXTRA_ROUTES = [sc._r("wf64-dense-140-20", "lev", 140, 20, sc.FORM_KERNEL, alpha=b"AC")]   # noisy batches only


def route(name):
    return next(r for r in ROUTES + EXTRA_ROUTES if r.name == name)


def oracle_cells(r):
    """DP cells the oracle runs for one whole copy of the route's pattern: a block per n-gram, both sides of each."""
    if r.kind != "lev":
        return r.m
    L = r.m // (r.k + 1)
    return (r.m // L) * r.m * (r.m + r.k)


def tier(r):
    """0: the full sweep in `mid` and `tile`; 1: the straddling subset everywhere; 2 (k >= 256 only): TIER2."""
    return 2 if oracle_cells(r) > HEAVY else 0 if r.m + r.k <= 200 else 1


def straddling(m, k):
    """The offsets at which a part of the copy, of an n-gram block or of a verification window meets the seam."""
    L = m // (k + 1)
    G = m // L
    ds = [-(m + k) - 1, -(m + k), -m - 1, -m, -m + 1, -m + L - 1, -m + L, -(m // 2), -L - 1, -L, -L + 1, -1, 0, 1, k, k + 1]
    ds += [-g * L for g in (0, G // 2, G - 1)]
    lo, hi = -(m + k) - 1, k + 1
    return sorted(set(d for d in ds if lo <= d <= hi))


def core(m, k):
    """TIER2, `mid`: a copy flush against the end of A (k = 256 only), one cut in half, one flush against the start of B."""
    return [-m, -(m // 2), 0] if k < 512 else [-(m // 2), 0]


def short_lengths(m, k, heavy=False):
    """|M| of the `short` class (TIER2: the pattern's length)."""
    L = m // (k + 1)
    return sorted(set(q for q in ((m,) if heavy else (1, L - 1, L, m - k - 1, m - k, m, m + k)) if q > 0))


def class_offsets(r, c):
    """The offsets a route runs in the sub-class c."""
    t = tier(r)
    if t == 2:
        return core(r.m, r.k) if c == "mid" else [-(r.m // 2)]
    if t == 0 and c in ("mid", "tile"):
        return sc.sweep_offsets(r.m, r.k)
    return straddling(r.m, r.k)


CLASSES = ("mid", "tile", "empty", "short", "edge")


def classes_of(r):
    """(m = 513, k = 512, single-character n-grams: 3 x 10^8 oracle cells per copy, 2.7 s - `mid` alone)"""
    return ("mid",) if tier(r) == 2 and r.k >= 512 else CLASSES


def edge_tails(r):
    return sc.EDGE_TAILS[:1] if tier(r) == 2 else sc.EDGE_TAILS


def sub_classes(cls, heavy=False):
    """The coverage entries of a class's batch (TIER2: the seam on the tile, one empty sequence)."""
    if heavy and cls in ("tile", "empty"):
        return {"tile": ("tile",), "empty": ("empty1",)}[cls]
    return {"mid": ("mid",), "tile": ("tile", "tile-1", "tile+1"), "empty": ("empty1", "empty3"), "short": ("short",),
            "edge": ("first", "last")}[cls]


# -- the construction ------------------------------------------------------------------------------------------------------
class _Packed(object):
    def __init__(self, p, seed):
        quiet = np.frombuffer(sc.quiet_alphabet(p), dtype=np.uint8)
        self.block = quiet[np.random.default_rng(seed).integers(0, len(quiet), 65521)].tobytes() * 2
        self.buf = bytearray()
        self.ends = []

    def seq(self, n):
        """A quiet sequence of n bytes -> its packed start."""
        at = len(self.buf)
        o = at % 65521
        while n > 0:
            piece = self.block[o:o + min(n, 65521)]
            self.buf += piece
            n -= len(piece)
            o = 0
        self.ends.append(len(self.buf))
        return at

    def sequences(self):
        out, lo = [], 0
        for e in self.ends:
            out.append(bytes(self.buf[lo:e]))
            lo = e
        return out


def build(r, cls, p=None, seed=1, tail=777):
    """One batch of the route `r` for the seam class `cls` ('mid', 'tile', 'empty', 'short', 'edge') -> (sequences, plants,
    coverage): plants in packed coordinates, coverage[sub-class] = {"exact": set of d, "edited": set of d, "seams": set of S
    (`short`: "M": the lengths of the middle sequence as well)}.  `tail`: the packed length mod 16 384 of the `edge` batch."""
    p = bytes(p or sc.route_pattern(r))
    m, k = r.m, r.k
    rnd = random.Random(seed * 1000003 + len(cls))
    pk = _Packed(p, seed)
    plants = []
    cover = {c: {"exact": set(), "edited": set(), "seams": set(), "M": set()} for c in sub_classes(cls, tier(r) == 2)}
    heavy = tier(r) == 2
    reach = 8 if heavy else m + 2 * k + 8
    subs_only = r.kind == "subs"

    def variants():
        out = [(True, p)]
        if k:
            out.append((False, sc.edited_copy(rnd, p, k, bytes(r.alpha), subs_only)))
        return out

    def put(at, v, c, d, S, exact):
        assert 0 <= at and at + len(v) <= len(pk.buf), (c, d)
        pk.buf[at:at + len(v)] = v
        plants.append(Plant(at, v, c, d, S, exact))
        cover[c]["exact" if exact else "edited"].add(d)
        cover[c]["seams"].add(S)

    def pair(c, d, v, exact, residue=None, on_tile=None, empties=0):
        """A | (empty sequences) | B with the copy v at S + d; `residue`: S mod 16; `on_tile`: S = a multiple of 16 384 + on_tile
        (a quiet filler sequence in front of A)."""
        len_a = max(0, -d) + reach + rnd.randint(0, 7)
        len_b = max(0, d + len(v)) + reach + rnd.randint(0, 7)
        at = len(pk.buf)
        if on_tile is not None:
            fill = (on_tile - (at + len_a)) % TILE
            if fill:
                pk.seq(fill)
        elif residue is not None:
            len_a += (residue - (at + len_a)) % 16
        pk.seq(len_a)
        S = len(pk.buf)
        for _ in range(empties):
            pk.seq(0)
        pk.seq(len_b)
        put(S + d, v, c, d, S, exact)

    if cls == "mid":
        i = 0
        for d in class_offsets(r, cls):
            for exact, v in variants():
                pair("mid", d, v, exact, residue=i % 16)
                i += 1
        if i < 16 and not heavy:                                  # (a sweep of fewer than 16 copies: exact copies at d = 0 fill the residues)
            for res in range(16):
                pair("mid", 0, p, True, residue=res)
    elif cls == "tile":
        for d in class_offsets(r, "tile"):
            for exact, v in variants():
                pair("tile", d, v, exact, on_tile=0)
        for shift, c in ((-1, "tile-1"), (1, "tile+1")) if not heavy else ():
            for d in class_offsets(r, c):
                for exact, v in variants():
                    pair(c, d, v, exact, on_tile=shift)
    elif cls == "empty":
        for n_empty, c in ((1, "empty1"), (3, "empty3"))[:1 if heavy else 2]:
            for d in class_offsets(r, c):
                for exact, v in variants():
                    pair(c, d, v, exact, empties=n_empty)
    elif cls == "short":
        for q in short_lengths(m, k, heavy):
            for exact, v in variants():
                # the copy starts in A, covers M and ends in B - centred on M, all but one byte of its rest in B, all but one in
                # A (a whole n-gram block on either side of M) -; where it fits, M starts with it (|M| = len: M is the copy)
                over = len(v) - q
                for d in sorted(set([-(over // 2), -1, -(over - 1)])) if over > 0 else [0]:
                    pk.seq(-d + reach + rnd.randint(0, 7))
                    S = pk.seq(q)
                    pk.seq(max(0, d + len(v) - q) + reach + rnd.randint(0, 7))
                    put(S + d, v, "short", d, S, exact)
                cover["short"]["M"].add(q)
    else:
        assert cls == "edge"
        # sequence 0 starts with the pattern, sequence 1 with an edited copy; the last two end with them; one tile and `tail` bytes
        total = TILE + tail
        head = variants()
        for exact, v in head:
            at = pk.seq(len(v) + reach + rnd.randint(0, 7))
            put(at, v, "first", 0, at, exact)
        room = total - len(pk.buf) - sum(len(v) + reach for _e, v in head)
        assert room > 0
        while room > 0:
            n = min(room, rnd.randint(1, 3000))
            pk.seq(n)
            room -= n
        for exact, v in reversed(head):
            pk.seq(len(v) + reach)
            put(len(pk.buf) - len(v), v, "last", -len(v), len(pk.buf), exact)
        assert len(pk.buf) == total
    return pk.sequences(), plants, cover


def batches(r, p=None, classes=None):
    """Every batch of the route (of `classes`): (cls or 'edge-<tail>', sequences, plants, coverage)."""
    for cls in classes or classes_of(r):
        if cls == "edge":
            for tail in edge_tails(r):
                yield ("edge-%d" % tail,) + build(r, "edge", p, seed=3 + tail, tail=tail)
        else:
            yield (cls,) + build(r, cls, p)


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, seqs), dtype=np.uint64, count=len(seqs)), out=offs[1:])
    return b"".join(seqs), offs


def check_coverage(r, cls, cover, seqs):
    """Every d of the class's sweep or subset is planted exact and (k > 0) edited in every sub-class; the 16 residues in `mid`;
    the tile seams where they are meant to be; equal ends in `empty`."""
    name = cls.split("-")[0]
    heavy = tier(r) == 2
    for c in sub_classes(name, heavy):
        if name == "edge":
            want = {0} if c == "first" else None
        elif name == "short":
            want = None
            assert cover[c]["M"] == set(short_lengths(r.m, r.k, tier(r) == 2)), (r.name, c, cover[c]["M"])
        else:
            want = set(class_offsets(r, c))
        if want is not None:
            assert cover[c]["exact"] >= want, (r.name, c, "exact copies missing at d =", sorted(want - cover[c]["exact"])[:8])
            if r.k:
                assert cover[c]["edited"] >= want, (r.name, c, "edited copies missing at d =", sorted(want - cover[c]["edited"])[:8])
        assert cover[c]["exact"] and (not r.k or cover[c]["edited"]), (r.name, c)
    if name == "mid" and tier(r) < 2:                             # (TIER2: six copies)
        assert set(S % 16 for S in cover["mid"]["seams"]) == set(range(16)), (r.name, "seam residues mod 16")
    if name == "tile":
        for c, shift in (("tile", 0), ("tile-1", TILE - 1), ("tile+1", 1))[:1 if heavy else 3]:
            assert all(S % TILE == shift for S in cover[c]["seams"]), (r.name, c)
    if name == "empty":
        ends = np.cumsum([len(s) for s in seqs])
        runs = collections.Counter()
        for c in sub_classes("empty", heavy):
            for S in cover[c]["seams"]:
                runs[int((ends == S).sum())] += 1
        assert set(runs) == ({2} if heavy else {2, 4}), (r.name, runs)                 # A's end and one / three empty sequences' ends coincide
    if name == "edge":
        assert sum(len(s) for s in seqs) % TILE in sc.EDGE_TAILS


# -- expected streams --------------------------------------------------------------------------------------------------------
def raw_oracle(mode, p, s, k):
    if mode == EXACT:
        return [(i, i + len(p), 0, -1) for i in oracle.search_exact(p, s)]
    return oracle.lev_ngrams_raw(p, s, k) if mode == LEV else oracle.subs_ngrams_raw(p, s, k)


def _cached(mode, p, s, k, cache):
    key = (mode, bytes(s))
    rows = cache.get(key)
    if rows is None:
        rows = cache[key] = [tuple(x) for x in raw_oracle(mode, p, s, k)]
    return rows


def expected(mode, p, seqs, k, cache):
    """The oracle per sequence -> (raw rows, reduced rows) of the batch as (sequence, start, end, dist, block) in the sequence's
    own coordinates; the reduced rows (oracle.consolidate / oracle.group_best) without the block.  `cache`: by sequence bytes."""
    raw, red = [], []
    for j, s in enumerate(seqs):
        if len(s) == 0:
            continue
        rows = _cached(mode, p, s, k, cache)
        if not rows:
            continue
        raw += [(j,) + r for r in rows]
        if mode == EXACT:
            best = [r[:3] for r in rows]
        elif mode == LEV:
            best = oracle.consolidate(rows)
        else:
            best = [b[:3] for b in oracle.group_best(rows)[0]]
        red += [(j,) + tuple(b) for b in best]
    return raw, red


def _ngram_at(mode, row, L):
    """Where the row's n-gram lies (exactly for exact and substitution rows, within k of it for Levenshtein rows)."""
    return row[0] if mode == EXACT else row[0] + row[3] * L


def seam_blind(mode, p, seqs, k, plants, cache):
    """A kernel without any clamp at the seams: the oracle on the packed bytes (on the quiet background: on the bytes around
    every plant), every row given to the sequence of its n-gram, in that sequence's coordinates, ordered as a batch search
    orders its rows (by sequence; within a sequence by block, then position)."""
    blob, offs = pack(seqs)
    offs = offs.astype(np.int64)
    m = len(p)
    L = m // (k + 1)
    W = m + 2 * k + 8
    rows = []
    for pl in sorted(plants):
        lo, hi = max(0, pl.start - W), min(len(blob), pl.start + len(pl.data) + W)
        for r in _cached(mode, p, blob[lo:hi], k, cache):
            at = min(max(_ngram_at(mode, r, L) + lo, 0), len(blob) - 1)
            j = int(np.searchsorted(offs, at, side="right")) - 1
            sa = int(offs[j])
            rows.append((j, r[0] + lo - sa, r[1] + lo - sa, r[2], r[3]))
    rows.sort(key=lambda x: (x[0], x[4]))
    return rows


def clamped_one_side(mode, p, seqs, k, side, cache):
    """A kernel that clamps a window at one end of its sequence only: `side` = 'sa': the oracle on packed[sa:] (here: up to the
    window's reach past se), 'se': on packed[:se] (from the reach before sa); rows whose n-gram lies in the sequence."""
    blob, offs = pack(seqs)
    offs = offs.astype(np.int64)
    m = len(p)
    L = m // (k + 1)
    W = m + 2 * k + 8
    rows = []
    for j in range(len(seqs)):
        sa, se = int(offs[j]), int(offs[j + 1])
        if sa == se:
            continue
        lo, hi = (sa, min(len(blob), se + W)) if side == "sa" else (max(0, sa - W), se)
        for r in _cached(mode, p, blob[lo:hi], k, cache):
            at = _ngram_at(mode, r, L) + lo
            if sa <= at < se:
                rows.append((j, r[0] + lo - sa, r[1] + lo - sa, r[2], r[3]))
    return rows


def flush_missing(mode, p, seqs, plants, raw):
    """The exact copies flush against a seam (d = 0: a sequence starts with it; d = -len: one ends with it) that the stream
    does not hold at distance 0 in that sequence."""
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    have = set(r[:4] for r in raw)
    missing = []
    for pl in plants:
        if pl.exact and pl.d in (0, -len(pl.data)):
            j = int(np.searchsorted(offs, pl.start, side="right")) - 1
            local = pl.start - int(offs[j])
            if local + len(p) > len(seqs[j]):
                continue                                        # (`short`: the copy starts with M and ends in B)
            assert local == 0 or local + len(p) == len(seqs[j]), (pl.cls, pl.d, "the copy is not flush")
            if (j, local, local + len(p), 0) not in have:
                missing.append((pl.cls, pl.d, j))
    return missing


def near(plants, seqs, j):
    """The plants in or next to sequence j, for a failure's report."""
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    lo, hi = int(offs[max(0, j - 1)]), int(offs[min(len(seqs), j + 2)])
    return [(pl.cls, pl.d, "exact" if pl.exact else "edited") for pl in plants if pl.start < hi and pl.start + len(pl.data) > lo][:4]


# -- noisy batches -----------------------------------------------------------------------------------------------------------
def noisy(r, p, tiles=3, seed=5):
    """`tiles` tiles and a tail of reads of 30 .. 300 bytes over the pattern's own alphabet, every third one with a copy of the
    pattern (exact or edited; at its start, at its end or inside), every seventh seam with a copy cut by it -> (sequences,
    plants).  The expected stream is the oracle per read."""
    rnd = random.Random(seed * 7919 + r.m)
    alpha = bytes(r.alpha)
    total = tiles * TILE + 777
    seqs, plants, at = [], [], 0
    while at < total:
        n = min(total - at, rnd.randint(30, 300))
        t = bytearray(rnd.choices(alpha, k=n))
        if len(seqs) % 3 == 0:
            exact = rnd.random() < 0.4
            v = p if exact else sc.edited_copy(rnd, p, r.k, alpha, r.kind == "subs")
            if len(v) <= n:
                o = rnd.choice([0, n - len(v), rnd.randint(0, n - len(v))])
                t[o:o + len(v)] = v
                plants.append(Plant(at + o, v, "noisy", o, at, exact))
        seqs.append(t)
        at += n
    for j in range(0, len(seqs) - 1, 7):
        a, b = seqs[j], seqs[j + 1]
        cut = rnd.randint(1, max(1, r.m - 1))
        if len(a) >= cut and len(b) >= r.m - cut:
            a[len(a) - cut:] = p[:cut]
            b[:r.m - cut] = p[cut:]
    return [bytes(s) for s in seqs], plants


def ngram_hits(p, seqs, k):
    """The n-gram occurrences the reference verifies over the batch (levenshtein_ngram.py:171-176, per sequence)."""
    m = len(p)
    L = m // (k + 1)
    hits = 0
    for s in seqs:
        n = len(s)
        for st in range(0, m - L + 1, L):
            lo = min(n, max(0, st - k))
            hits += len(oracle.search_exact(p[st:st + L], s, lo, max(lo, min(n, n - m + st + L + k))))
    return hits
