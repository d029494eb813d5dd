"""-m gpu: many patterns over many sequences (fz_batch_search_multi / find_near_matches_multi_batch) — every (pattern,
sequence) slice bit-exact and ordered against the oracle run on that sequence alone and against the engine's own
fz_batch_search of that pattern, raw and reduced, as a pass and as the loop inside the call."""
import os
import random

import numpy as np
import pytest

import oracle
from fuzzysearch_amd import _native
from tests import gpu_cases

pytestmark = pytest.mark.gpu

TILE = 16384
EXACT, LEV, SUBS = 0, 1, 2
FORM_KERNEL = 5


force_pass = pytest.fixture(gpu_cases.force_pass)


def _rand(rnd, alpha, n):
    return bytes(rnd.choices(alpha, k=n))


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, seqs), dtype=np.uint64, count=len(seqs)), out=offs[1:])
    return b"".join(seqs), offs


def _edit(rnd, mode, p, n, alpha):
    """p with n edits (Levenshtein) or n substituted characters (substitutions only)."""
    if mode == LEV:
        return gpu_cases.edited(rnd, p, n, alpha)
    v = bytearray(p)
    for q in rnd.sample(range(len(v)), min(n, len(v))):
        v[q] = rnd.choice(alpha)
    return bytes(v)


def _oracle_raw(mode, p, s, k, cache):
    key = (mode, p, s, k)
    rows = cache.get(key)
    if rows is None:
        rows = cache[key] = oracle.lev_ngrams_raw(p, s, k) if mode == LEV else oracle.subs_ngrams_raw(p, s, k)
    return rows


def _expected(mode, p, seqs, k, cache):
    """-> (raw rows, reduced rows) of one pattern over the batch as (sequence, start, end, dist[, block]), per sequence."""
    raw, red = [], []
    for j, s in enumerate(seqs):
        rows = _oracle_raw(mode, p, s, k, cache)
        if not rows:
            continue
        raw += [(j,) + tuple(r) for r in rows]
        best = oracle.consolidate(rows) if mode == LEV else [b[:3] for b in oracle.group_best(rows)[0]]
        red += [(j,) + tuple(b) for b in best]
    return raw, red


def _flat(rows, seq_of):
    assert len(rows) == len(seq_of)
    assert np.all(np.diff(seq_of.astype(np.int64)) >= 0), "seq_of is non-decreasing within a pattern's slice"
    return [(int(j),) + tuple(int(x) for x in r) for j, r in zip(seq_of.tolist(), rows.tolist())]


def _check(engine, h, seqs, mode, pats, k, cache, vs_single=True, what=None):
    """fz_batch_search_multi over resident batch `h` (= seqs), raw and reduced, against the oracle per (pattern, sequence)
    and against fz_batch_search of every pattern.  -> (raw rows, (pattern, sequence) cells with rows, stats of the raw call)."""
    raw = engine.batch_search_multi(h, mode, pats, k, reduced=False)
    st = engine.stats()
    red = engine.batch_search_multi(h, mode, pats, k, reduced=True)
    assert len(raw) == len(red) == len(pats)
    n_rows = cells = 0
    for i, p in enumerate(pats):
        want_raw, want_red = _expected(mode, p, seqs, k, cache)
        got = _flat(*raw[i])
        assert got == want_raw, ("raw vs oracle", what, mode, k, i, len(p))
        assert [g[:4] for g in _flat(*red[i])] == want_red, ("reduced vs oracle", what, mode, k, i, len(p))
        if vs_single:
            assert got == _flat(*engine.batch_search(h, mode, p, k, reduced=False)), ("raw vs single", what, i)
            assert _flat(*red[i]) == _flat(*engine.batch_search(h, mode, p, k, reduced=True)), ("reduced vs single", what, i)
        n_rows += len(want_raw)
        cells += len(set(r[0] for r in want_raw))
    assert st["raw_matches"] == n_rows
    return n_rows, cells, st


def _random_batch(rnd, mode, pats, k, alpha, n_seqs):
    """The batches of test_gpu_batch, for a list of patterns: sequences of lengths 0 .. ~3 tiles — many short ones per tile,
    at most two long ones that span tile seams — with planted edited copies (both ends included) and copies cut in two by a
    seam between sequences."""
    seqs, big = [], 0
    for _ in range(n_seqs):
        m = len(rnd.choice(pats))
        kind = rnd.random()
        if kind < 0.15:
            n = 0
        elif kind < 0.4:
            n = rnd.randint(1, 40)
        elif kind < 0.6:
            n = rnd.randint(max(0, m - k - 2), m + 2 * k + 2)
        elif kind < 0.93 or big >= 2:
            n = rnd.randint(100, 400)
        else:
            n = rnd.choice([rnd.randint(TILE - 50, TILE + 50), rnd.randint(TILE, 3 * TILE)])
            big += 1
        t = bytearray(_rand(rnd, alpha, n))
        for _rep in range(2):
            p = rnd.choice(pats)
            if n >= len(p) - k and rnd.random() < 0.6:
                v = _edit(rnd, mode, p, rnd.randint(0, k), alpha)
                if len(v) <= n:
                    st = rnd.choice([0, 1, n - len(v) - 1, n - len(v), rnd.randint(0, n - len(v))])
                    st = max(0, min(st, n - len(v)))
                    t[st:st + len(v)] = v
        seqs.append(t)
    for j in range(len(seqs) - 1):                       # a copy cut in two by the seam between j and j + 1
        if rnd.random() < 0.3:
            p = rnd.choice(pats)
            cut = rnd.randint(1, len(p) - 1)
            a, b = seqs[j], seqs[j + 1]
            if len(a) >= cut and len(b) >= len(p) - cut:
                a[len(a) - cut:] = p[:cut]
                b[:len(p) - cut] = p[cut:]
    return [bytes(s) for s in seqs]


def random_draw(rnd, it):
    """Draw `it` of the random test: (mode, k, patterns, sequences).  2 .. 40 patterns of one to three lengths, inside the
    batched domain (n-grams of 4 and more, up to 128 characters) and outside it (n-grams of 3; 129 and 150 characters)."""
    mode = LEV if it % 2 == 0 else SUBS
    k = [1, 2, 3, 4, 8][(it // 2) % 5]
    sigma = rnd.choice([2, 4, 4, 4, 20, 200])
    alpha = bytes(rnd.sample(range(1, 256), sigma))
    pool = [3 * (k + 1), 4 * (k + 1), 4 * (k + 1) + 1, 5 * (k + 1) + 2, 20, 23, 32, 64, 128, 129, 150]
    lengths = [rnd.choice([m for m in pool if m >= 3 * (k + 1)]) for _ in range(rnd.randint(1, 3))]
    # (two symbols: nearly every offset is a candidate and most windows match — few patterns, few sequences)
    npat = rnd.randint(2, 5) if sigma == 2 else rnd.randint(2, 40)
    pats = [_rand(rnd, alpha, rnd.choice(lengths)) for _ in range(npat)]
    n_seqs = rnd.choice([1, 2, rnd.randint(3, 12)]) if sigma == 2 else rnd.choice([1, 2, rnd.randint(3, 40), rnd.randint(100, 300)])
    return mode, k, pats, _random_batch(rnd, mode, pats, k, alpha, n_seqs)


RANDOM_SEED, RANDOM_LISTS, RANDOM_CHUNKS = 191, 40, 4
# Per chunk of ten draws, computed on the CPU from the oracle and the planner (tests/test_gpu_multi_batch.py run as a
# program prints them): raw rows; lists in which a group rides a pass by the cost rule / with FZ_MP_FORCE_PASS; (pattern,
# sequence) cells with rows.  The floors are those figures: a run that finds less found too little.
RANDOM_FLOORS = {
    0: (269, 3, 6, 80),
    1: (308, 3, 6, 97),
    2: (1249, 6, 7, 432),
    3: (1389, 3, 7, 439),
}


def _chunk_draws(chunk):
    rnd = random.Random(RANDOM_SEED + chunk)
    per = RANDOM_LISTS // RANDOM_CHUNKS
    return [(it,) + random_draw(rnd, it) for it in range(chunk * per, (chunk + 1) * per)]


def _plan_groups(pats, k, mode):
    return _native.multi_plan(pats, k, mode)[1]


@pytest.mark.parametrize("chunk", range(RANDOM_CHUNKS))
def test_random(engine, force_pass, chunk):
    rows = cells = 0
    passes = {False: 0, True: 0}
    for it, mode, k, pats, seqs in _chunk_draws(chunk):
        blob, offs = _pack(seqs)
        h = engine.upload_batch(blob, offs)
        cache = {}
        try:
            for forced in (False, True):
                force_pass(forced)
                n, c, st = _check(engine, h, seqs, mode, pats, k, cache, vs_single=not forced, what=(it, forced))
                rides = _plan_groups(pats, k, mode) > 0 and len(blob) > 0
                assert (st["verify_form"] == FORM_KERNEL) == rides, ("a planned group rides a pass", it, forced)
                passes[forced] += rides
            rows += n
            cells += c
        finally:
            h.release()
    print("random chunk %d: %d rows, %d / %d lists with a pass (cost rule / forced), %d cells with rows"
          % (chunk, rows, passes[False], passes[True], cells))
    want_rows, want_rule, want_forced, want_cells = RANDOM_FLOORS[chunk]
    assert want_rows > 0 and want_forced > 0 and want_cells > 0, "floors are computed, not left empty"
    assert rows >= want_rows and passes[False] >= want_rule and passes[True] >= want_forced and cells >= want_cells


def _seam_patterns(rnd, m, alpha=b"ACGT"):
    return [_rand(rnd, alpha, m) for _ in range(8)]


@pytest.mark.parametrize("mode", [LEV, SUBS])
@pytest.mark.parametrize("m", [20, 33])
def test_seams_every_split(engine, force_pass, mode, m):
    """Two- and three-sequence batches, a copy with 0 .. k edits across the seam(s) at every split 1 .. m - 1: found for no
    neighbour (beyond what a neighbour holds on its own: the oracle says); a copy ending exactly at a seam and one starting
    exactly at it: found, in the right sequence."""
    force_pass(True)
    rnd = random.Random(192 + m + mode)
    k, alpha, bg = 2, b"ACGT", b"xyz"                       # a background free of the patterns' symbols
    pats = _seam_patterns(rnd, m)
    assert _plan_groups(pats, k, mode) == 1
    cache = {}
    nothing = found = 0
    for cut in range(1, m):
        i = cut % len(pats)
        v = _edit(rnd, mode, pats[i], cut % (k + 1), alpha)
        c = min(cut, len(v) - 1)
        c2 = c + max(1, (len(v) - c) // 2)
        two = [_rand(rnd, bg, 40) + v[:c], v[c:] + _rand(rnd, bg, 40)]
        three = [_rand(rnd, bg, 40) + v[:c], v[c:c2], v[c2:] + _rand(rnd, bg, 40)]
        for seqs in (two, three):
            blob, offs = _pack(seqs)
            h = engine.upload_batch(blob, offs)
            n, _, st = _check(engine, h, seqs, mode, pats, k, cache, vs_single=False, what=(m, cut, len(seqs)))
            h.release()
            assert st["verify_form"] == FORM_KERNEL and st["filter_launches"] == 1
            nothing += n == 0
            found += n
    # (k < cut < m - k: no part of an exact or edited copy is within the budget on its own)
    assert nothing >= m - 1 - 2 * (k + 1), nothing
    p = pats[0]
    seqs = [_rand(rnd, bg, 30) + p, p + _rand(rnd, bg, 30), _rand(rnd, bg, 10) + p]
    blob, offs = _pack(seqs)
    h = engine.upload_batch(blob, offs)
    _check(engine, h, seqs, mode, pats, k, cache)
    got = _flat(*engine.batch_search_multi(h, mode, pats, k, reduced=True)[0])
    h.release()
    assert [g[:4] for g in got] == [(0, 30, 30 + m, 0), (1, 0, m, 0), (2, 10, 10 + m, 0)], "flush against a seam, in the right sequence"


def test_seams_window_clamps(engine, force_pass):
    """Levenshtein: a copy that lost its first characters at the start of its sequence and one that lost its last ones at
    the end of its sequence — the window is clamped to [sa, se), with the neighbours' bytes right behind the clamps."""
    force_pass(True)
    rnd = random.Random(193)
    alpha, k = b"ACGT", 2
    for m in (20, 33):
        pats = _seam_patterns(rnd, m)
        cache = {}
        for d in range(0, k + 1):
            seqs = []
            for i, p in enumerate(pats):
                seqs += [p[d:] + _rand(rnd, alpha, 12), _rand(rnd, alpha, 12) + p[:m - d], p[d:m - (k - d)]]
            blob, offs = _pack(seqs)
            h = engine.upload_batch(blob, offs)
            n, _, st = _check(engine, h, seqs, LEV, pats, k, cache, what=(m, d))
            got = engine.batch_search_multi(h, LEV, pats, k)
            h.release()
            assert st["verify_form"] == FORM_KERNEL
            for i, p in enumerate(pats):
                rows = _flat(*got[i])
                assert any(r[0] == 3 * i and r[1] == 0 and r[3] <= d for r in rows), (m, d, i, "leading deletions at sa")
                assert any(r[0] == 3 * i + 1 and r[2] == 12 + m - d and r[3] <= d for r in rows), (m, d, i, "trailing deletions at se")
                assert any(r[0] == 3 * i + 2 and r[3] <= k for r in rows), (m, d, i, "both")


@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_seams_tile_boundary_and_degenerate(engine, force_pass, mode):
    """A seam at a tile boundary and at +-1 and +-(L - 1) around it; sequences of length 0, 1, L - 1, L, m - k - 1, m - k and m
    between two long ones; the first sequence at offset 0, the last one ending with the buffer; all-empty and one-sequence
    batches."""
    force_pass(True)
    rnd = random.Random(194 + mode)
    alpha, k = b"ACGT", 2
    rows = 0
    for m in (20, 33):
        L = m // (k + 1)
        pats = _seam_patterns(rnd, m)
        p = pats[0]
        cache = {}
        for seam in (TILE - (L - 1), TILE - 1, TILE, TILE + 1, TILE + (L - 1)):
            a = bytearray(_rand(rnd, alpha, seam))
            b = bytearray(_rand(rnd, alpha, 500))
            a[:m] = pats[2]                                # the first sequence starts the buffer
            a[seam - m:] = _edit(rnd, mode, p, 1, alpha)[:m].ljust(m, b"A")    # ends exactly at the seam
            b[:m] = pats[1]                                # starts exactly at it
            b[500 - m:] = pats[3]                          # the last sequence ends with the buffer
            for seqs in ([bytes(a), bytes(b)],
                         [bytes(a)] + [p[:n] for n in (0, 1, L - 1, L, m - k - 1, m - k, m)] + [bytes(b)]):
                blob, offs = _pack(seqs)
                h = engine.upload_batch(blob, offs)
                n, _, st = _check(engine, h, seqs, mode, pats, k, cache, vs_single=(seam == TILE), what=(m, seam, len(seqs)))
                h.release()
                assert st["verify_form"] == FORM_KERNEL
                rows += n
        # all sequences empty: nothing is launched, every slice is empty
        for n_seqs in (1, 7):
            blob, offs = _pack([b""] * n_seqs)
            h = engine.upload_batch(blob, offs)
            assert _check(engine, h, [b""] * n_seqs, mode, pats, k, cache)[0] == 0
            h.release()
        # one sequence: the multi-pattern search of the same bytes uploaded plainly
        one = bytearray(_rand(rnd, alpha, 2 * TILE + 123))
        for j, at in enumerate((0, 700, TILE - 9, 2 * TILE + 123 - m)):
            one[at:at + m] = _edit(rnd, mode, pats[j], j % (k + 1), alpha)[:m].ljust(m, b"C")
        one = bytes(one)
        hb = engine.upload_batch(*_pack([one]))
        hs = engine.upload(one)
        got = engine.batch_search_multi(hb, mode, pats, k)
        plain = (engine.lev_ngrams_multi if mode == LEV else engine.subs_ngrams_multi)(hs, pats, k)
        assert [[tuple(int(x) for x in r) for r in g[0].tolist()] for g in got] == plain
        assert sum(len(r) for r in plain) >= 4 and not any(g[1].any() for g in got)
        hb.release()
        hs.release()
    assert rows > 100


def _periodic_patterns(rnd, m=20, L=6):
    """8 patterns of m over four letters that share their n-grams: rotations of one string of period L, so that a text made
    of them matches several blocks of several patterns at nearly every offset."""
    unit = _rand(rnd, b"ACGT", L)
    while len(set(unit)) < 3:
        unit = _rand(rnd, b"ACGT", L)
    return [((unit[r % L:] + unit[:r % L]) * (m // L + 2))[:m] for r in range(8)]


@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_overflow(force_pass, mode):
    """Far more hits and records than the sizing from the arguments expects (8 patterns of 20 over four letters: 24 n / 4^6
    hits; the reads are the patterns themselves over and over, and the patterns share their n-grams): the launches are run
    again with what their counters ask for, and the result stays exact.  On an engine of its own: the hit lists and the
    record buffer of a context keep the size an earlier search grew them to."""
    force_pass(True)
    rnd = random.Random(195 + mode)
    k = 2
    pats = _periodic_patterns(rnd)
    assert _plan_groups(pats, k, mode) == 1
    seqs, total = [], 0
    while total < (64 << 10):
        s = b"".join(rnd.choice(pats) for _ in range(8))[:rnd.randint(100, 160)]
        seqs.append(s)
        total += len(s)
    eng = _native.Engine([0])
    try:
        h = eng.upload_batch(*_pack(seqs))
        n, cells, st = _check(eng, h, seqs, mode, pats, k, {}, vs_single=False)
        h.release()
        assert st["verify_form"] == FORM_KERNEL and st["filter_launches"] >= 2, "the first sizing should not have held this"
        assert n > (1 << 16) and cells >= len(seqs)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_several_passes(engine, force_pass, mode):
    force_pass(True)
    rnd = random.Random(196 + mode)
    alpha, k = b"ACGT", 2
    pats = [_rand(rnd, alpha, 20) for _ in range(150)]
    group_of, ng = _native.multi_plan(pats, k, mode)
    assert ng == 3 and None not in group_of
    seqs = []
    for j in range(200):
        t = bytearray(_rand(rnd, alpha, rnd.randint(100, 200)))
        v = _edit(rnd, mode, pats[(7 * j) % len(pats)], j % (k + 1), alpha)
        at = rnd.choice([0, len(t) - len(v), rnd.randint(0, len(t) - len(v))])
        t[at:at + len(v)] = v
        seqs.append(bytes(t))
    blob, offs = _pack(seqs)
    h = engine.upload_batch(blob, offs)
    n, cells, st = _check(engine, h, seqs, mode, pats, k, {}, vs_single=False)
    h.release()
    assert st["filter_launches"] == ng and st["bytes_scanned"] == ng * len(blob) and st["verify_form"] == FORM_KERNEL
    assert n >= 200 and cells >= 200                       # (a planted copy keeps a block intact: a row at least in every read)


def test_refusals_and_state(engine, force_pass):
    force_pass(True)
    rnd = random.Random(197)
    alpha, k = b"ACGT", 2
    seqs = [_rand(rnd, alpha, 200) for _ in range(20)]
    pats = [seqs[4][50:70], seqs[9][100:120], seqs[0][:20], seqs[19][180:]]
    blob, offs = _pack(seqs)
    hb = engine.upload_batch(blob, offs)
    hs = engine.upload(blob)
    before_batch = _flat(*engine.batch_search(hb, LEV, pats[0], k))
    before_multi = engine.subs_ngrams_multi(hs, pats, k)
    # a plain handle; modes the call does not serve
    with pytest.raises(ValueError):
        engine.batch_search_multi(hs, LEV, pats, k)
    for mode in (EXACT, 3):
        with pytest.raises(ValueError):
            engine.batch_search_multi(hb, mode, pats, k)
    # the multi-pattern calls of a plain sequence keep refusing a batch handle
    with pytest.raises(ValueError):
        engine.lev_ngrams_multi(hb, pats, k)
    with pytest.raises(ValueError):
        engine.subs_ngrams_multi(hb, pats, k)
    # a search still in flight: refused, and the pipeline stays usable
    engine.lev_ngrams_begin(hs, pats[0], k)
    try:
        with pytest.raises(ValueError):
            engine.batch_search_multi(hb, LEV, pats, k)
    finally:
        assert engine.lev_ngrams_end() == oracle.lev_ngrams_raw(pats[0], blob, k)
    # a pattern the single call refuses fails the whole call with that call's error, before anything runs
    for mode in (LEV, SUBS):
        for bad in (b"", b"AC", b"G"):
            with pytest.raises(Exception) as single:
                engine.batch_search(hb, mode, bad, k)
            with pytest.raises(Exception) as multi:
                engine.batch_search_multi(hb, mode, [pats[0], bad, pats[1]], k)
            assert type(multi.value) is type(single.value) and str(multi.value) == str(single.value)
    assert engine.batch_search_multi(hb, LEV, [], k) == []
    # an engine of two device states
    two = _native.Engine([0, 0])
    try:
        h2 = two.upload(blob)
        with pytest.raises(_native.UnsupportedSearch):
            two.batch_search_multi(h2, LEV, pats, k)
        h2.release()
    finally:
        two.close()
    # ... and everything works as before: the call itself, and the calls that share its buffers
    cache = {}
    n, _, st = _check(engine, hb, seqs, LEV, pats, k, cache)
    assert n >= 4 and st["verify_form"] == FORM_KERNEL
    _check(engine, hb, seqs, SUBS, pats, k, cache)
    assert _flat(*engine.batch_search(hb, LEV, pats[0], k)) == before_batch
    assert engine.subs_ngrams_multi(hs, pats, k) == before_multi
    assert sum(len(r) for r in before_multi) >= 4
    hb.release()
    hs.release()


def test_timing_totals(engine, force_pass):
    """The device times of the three list-of-patterns calls — the plain sequence's, the batch's and the assignment — with four
    patterns that ride one pass and one (n-grams of 2: below the batched domain) that is searched on its own: with timing on
    both spans are measured and device_ms is their sum; with timing off all three are exactly 0 and the results the same."""
    force_pass(True)
    rnd = random.Random(200)
    k = 2
    seqs = [_rand(rnd, b"ACGT", 200) for _ in range(20)]
    pats = [seqs[4][50:70], seqs[9][100:120], seqs[0][:20], seqs[19][180:], seqs[12][30:37]]
    blob, offs = _pack(seqs)
    hb = engine.upload_batch(blob, offs)
    hs = engine.upload(blob)

    def plain(mode):
        rows, bounds = engine.multi_rows_call(hs, pats, k, mode=mode)
        return rows.to_array().tolist(), list(bounds)

    def batch(mode):
        return [_flat(*g) for g in engine.batch_search_multi(hb, mode, pats, k)]

    def assign(mode):
        return engine.batch_assign(hb, mode, pats, k).tolist()

    try:
        for mode in (LEV, SUBS):
            group_of, ng = _native.multi_plan(pats, k, mode)
            assert ng == 1 and group_of[:4] == [0] * 4 and group_of[4] is None, "four patterns in a pass, one on its own"
            for call in (plain, batch, assign):
                engine.set_timing(1)
                timed = call(mode)
                st = engine.stats()
                print(call.__name__, mode, st["filter_ms"], st["verify_ms"], st["device_ms"], st["n_devices"])
                assert st["filter_ms"] > 0 and st["verify_ms"] > 0
                assert st["device_ms"] == pytest.approx(st["filter_ms"] + st["verify_ms"], rel=1e-9, abs=0)
                assert st["n_devices"] == 1
                engine.set_timing(0)
                untimed = call(mode)
                st = engine.stats()
                assert st["filter_ms"] == 0 and st["verify_ms"] == 0 and st["device_ms"] == 0
                assert st["n_devices"] == 1
                assert untimed == timed and len(timed) > 0
    finally:
        engine.set_timing(1)
        hb.release()
        hs.release()


# ---- the public call ------------------------------------------------------------------------------------------------

def _reads(rnd, pats, alpha="ACGT"):
    seqs = []
    for _ in range(150):
        n = rnd.choice([0, 5, 23, 24, 30, 150, 151, 400])
        s = [rnd.choice(alpha) for _ in range(n)]
        if n >= 30 and rnd.random() < 0.6:
            p = rnd.choice(pats)
            v = gpu_cases.edited(rnd, p.encode(), rnd.randint(0, 2), alpha.encode()).decode()
            at = rnd.randint(0, n - len(v)) if n > len(v) else 0
            s[at:at + len(v)] = v
        seqs.append("".join(s))
    return seqs


def _nested(pats, seqs, **limits):
    import fuzzysearch_amd as fa
    return [fa.find_near_matches_batch(p, seqs, **limits) for p in pats]


def _same(got, want):
    assert got == want
    assert [[[x.matched for x in s] for s in g] for g in got] == [[[x.matched for x in s] for s in w] for w in want]
    return sum(len(s) for g in got for s in g)


L2 = dict(max_l_dist=2)
S2 = dict(max_substitutions=2, max_insertions=0, max_deletions=0)


def test_public_api_bytes_and_str(engine):
    import fuzzysearch_amd as fa
    rnd = random.Random(198)
    spats = ["".join(rnd.choice("ACGT") for _ in range(m)) for m in (24, 24, 24, 20, 20, 32, 24, 24, 24, 24, 33, 64)]
    sseqs = _reads(rnd, spats)
    bpats, bseqs = [p.encode() for p in spats], [s.encode() for s in sseqs]
    assert _native.multi_plan(bpats, 2, LEV)[1] >= 1 and _native.multi_plan(bpats, 2, SUBS)[1] >= 1, "the lists are meant to ride a pass"
    found = 0
    for limits in (L2, S2):
        got = fa.find_near_matches_multi_batch(bpats, bseqs, **limits)
        assert engine.stats()["verify_form"] == FORM_KERNEL, "the default engine ran a pass last"
        found += _same(got, _nested(bpats, bseqs, **limits))
        # (latin-1 str: Levenshtein rides the pass, substitutions-only loops read by read — fewer of them)
        ps, ss = (spats, sseqs) if limits is L2 else (spats[:4], sseqs[:60])
        found += _same(fa.find_near_matches_multi_batch(ps, ss, **limits), _nested(ps, ss, **limits))
    # (a floor from the inputs alone: 3 / 8 of the 150 reads are 150 bytes or longer, 60 % of those carry a copy, a third of
    # the copies are exact and found under either limit: some 11 per call, four calls, the substitution-only ones on fewer reads)
    assert found >= 30
    got = fa.find_near_matches_multi_batch(bpats[:2], bseqs, **L2)
    hit = [(j, x) for j, per in enumerate(got[0]) for x in per]
    assert hit and all(x.matched == bseqs[j][x.start:x.end] for j, x in hit), "matched comes from the read itself"


def test_public_api_resident_mixed_kinds_and_routes(engine):
    import fuzzysearch_amd as fa
    rnd = random.Random(199)
    spats = ["".join(rnd.choice("ACGT") for _ in range(24)) for _ in range(6)]
    bpats = [p.encode() for p in spats]
    bseqs = [s.encode() for s in _reads(rnd, spats)]
    # a resident batch reused across two pattern lists
    held = fa.resident_batch(bseqs)
    found = _same(fa.find_near_matches_multi_batch(bpats, held, **L2), _nested(bpats, bseqs, **L2))
    second = [p[2:] for p in bpats[:3]] + [bytearray(bpats[4]), memoryview(bpats[5])]
    found += _same(fa.find_near_matches_multi_batch(second, held, **S2), _nested(second, bseqs, **S2))
    # exact, n-gram, linear-programming and generic-limit routes in one list / through the keyword limits
    routes = [bpats[0], bpats[1][:5], bpats[2], b"ACG", bpats[3][:8], next(s for s in bseqs if len(s) >= 150)[3:27]]
    for limits in (L2, S2, dict(max_l_dist=0), dict(max_substitutions=1, max_insertions=1, max_deletions=1, max_l_dist=2),
                   dict(max_substitutions=2, max_insertions=2, max_deletions=2, max_l_dist=2)):
        found += _same(fa.find_near_matches_multi_batch(routes, held, **limits), _nested(routes, bseqs, **limits))
    held.release()
    assert found >= 30                                     # (as above: the exact copies of the first two lists alone)
    # a list with mixed kinds: the loop, and its errors
    mixed = [bseqs[5], bytearray(bseqs[6]), bseqs[7]]
    _same(fa.find_near_matches_multi_batch(bpats, mixed, **L2), _nested(bpats, mixed, **L2))
    ints = [[rnd.randint(0, 3) for _ in range(rnd.randint(0, 60))] for _ in range(20)]
    pi = [[0, 1, 2, 3] * 3, [3, 2, 1, 0] * 3]
    assert fa.find_near_matches_multi_batch(pi, ints, max_l_dist=1) == _nested(pi, ints, max_l_dist=1)
    with pytest.raises(TypeError):
        fa.find_near_matches_multi_batch(bpats, [bseqs[5], bseqs[6].decode()], **L2)
    with pytest.raises(TypeError):
        fa.find_near_matches_multi_batch([bpats[0], spats[1]], bseqs, **L2)       # what the loop raises at the str
    with pytest.raises(ValueError) as e1:
        fa.find_near_matches_batch(b"", bseqs, **L2)
    with pytest.raises(ValueError) as e2:
        fa.find_near_matches_multi_batch([bpats[0], b"", bpats[1]], bseqs, **L2)
    assert str(e1.value) == str(e2.value)


if __name__ == "__main__":
    # The floors of test_random, from the oracle and the planner alone (no device).
    lib = _native.load_library()
    for chunk in range(RANDOM_CHUNKS):
        rows = cells = rule = forced = 0
        for it, mode, k, pats, seqs in _chunk_draws(chunk):
            cache = {}
            for p in pats:
                raw, _ = _expected(mode, p, seqs, k, cache)
                rows += len(raw)
                cells += len(set(r[0] for r in raw))
            has_bytes = any(len(s) for s in seqs)
            os.environ.pop("FZ_MP_FORCE_PASS", None)
            lib.fz_debug_reload_switches()
            rule += _plan_groups(pats, k, mode) > 0 and has_bytes
            os.environ["FZ_MP_FORCE_PASS"] = "1"
            lib.fz_debug_reload_switches()
            forced += _plan_groups(pats, k, mode) > 0 and has_bytes
        print("    %d: (%d, %d, %d, %d)," % (chunk, rows, rule, forced, cells))
