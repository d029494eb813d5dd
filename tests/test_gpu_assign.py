"""-m gpu: the best pattern per sequence on the device (fz_batch_assign / Engine.batch_assign / find_best_matches_batch) —
every row against the ten-line model of the definition (tests/test_assign_host.py) over the oracle's raw rows per (pattern,
sequence), as a pass and as the loop inside the call."""
import random

import numpy as np
import pytest

from fuzzysearch_amd import _native
from tests import gpu_cases
from tests.test_assign_host import as_tuples, check_floors, draws, oracle_model, pack, raw_rows, tally
from tests.test_gpu_multi_batch import (force_pass, _edit, _flat, _periodic_patterns, _plan_groups, _rand, _reads,  # noqa: F401
                                        EXACT, FORM_KERNEL, LEV, SUBS, TILE)

pytestmark = pytest.mark.gpu

NONE = (-1, 0, 0, 0, 0)
BG = b"xyz"                                                 # a background free of the patterns' symbols


def _assign(engine, seqs, mode, pats, k, cache, what=None, want=None):
    """batch_assign over a fresh upload of `seqs` against the model; -> (the expected rows, stats of the call)."""
    blob, offs = pack(seqs)
    h = engine.upload_batch(blob, offs)
    try:
        got = engine.batch_assign(h, mode, pats, k)
        st = engine.stats()
    finally:
        h.release()
    assert got.dtype == _native.assign_dtype() and len(got) == len(seqs)
    if want is None:
        want = oracle_model(mode, pats, seqs, k, cache)
    assert as_tuples(got) == want, (what, mode, k)
    assert st["raw_matches"] == sum(len(raw_rows(mode, p, s, k, cache)) for p in pats for s in seqs), ("records folded", what)
    return want, st


def _assign_and_multi(engine, h, mode, pats, k):
    """-> (rows of batch_assign, its stats, the stats of batch_search_multi for the same arguments).  A call whose first
    sizing overflows runs a launch again and the context keeps the grown buffers: the assignment is run (and checked) once
    before the two calls whose launches are compared."""
    first = engine.batch_assign(h, mode, pats, k)
    engine.batch_search_multi(h, mode, pats, k, reduced=False)
    multi = engine.stats()
    got = engine.batch_assign(h, mode, pats, k)
    assert np.array_equal(first, got), "the same answer whatever the buffers' sizes"
    return got, engine.stats(), multi


def test_random(engine, force_pass):
    total = [0, 0, 0]
    passes = {False: 0, True: 0}
    for it, mode, k, pats, seqs in draws():
        blob, offs = pack(seqs)
        cache = {}
        want = oracle_model(mode, pats, seqs, k, cache)
        h = engine.upload_batch(blob, offs)
        try:
            for forced in (False, True):
                force_pass(forced)
                got, st, multi = _assign_and_multi(engine, h, mode, pats, k)
                assert as_tuples(got) == want, (it, mode, k, forced)
                rides = _plan_groups(pats, k, mode) > 0 and len(blob) > 0
                assert (st["verify_form"] == FORM_KERNEL) == rides, ("a planned group rides a pass", it, forced)
                assert st["filter_launches"] == multi["filter_launches"] and st["bytes_scanned"] == multi["bytes_scanned"], (it, forced)
                assert st["raw_matches"] == multi["raw_matches"] and st["ngram_hits"] == multi["ngram_hits"], (it, forced)
                passes[forced] += rides
        finally:
            h.release()
        total = [a + b for a, b in zip(total, tally(want))]
    print("random: %d assigned, %d tied, %d winners other than pattern 0; %d / %d lists with a pass (cost rule / forced)"
          % (tuple(total) + (passes[False], passes[True])))
    check_floors(total)
    assert passes[True] > 0


@pytest.mark.parametrize("m", [20, 11])
@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_ties_and_order(engine, force_pass, mode, m):
    """Hand-built reads.  m = 20: the list rides a pass; m = 11: n-grams of 3, every pattern is searched on its own and its
    records take the same fold."""
    force_pass(True)
    rnd = random.Random(1210 + mode + m)
    k = 2
    a, b, c = (_rand(rnd, b"ACGT", m) for _ in range(3))

    def bg(n):
        return _rand(rnd, BG, n)

    def one(p):                                             # one substitution behind the last n-gram block: distance 1 in both modes
        return p[:-1] + bytes([next(x for x in b"ACGT" if x != p[-1])])

    pats = [a, b, a, c]
    rides = m == 20
    assert _plan_groups(pats, k, mode) == (1 if rides else 0)
    seqs = [
        bg(7) + a + bg(5),                                  # a pattern listed twice: the lowest index, tied
        bg(3) + one(b) + bg(9) + c + bg(4),                 # c exact, b at 1: c, not tied
        bg(5) + one(c) + bg(6) + one(b) + bg(2),            # b and c both at 1: the lower index, tied
        bg(4) + b + bg(11) + b + bg(3),                     # two exact copies of the winner: the smaller start
        bg(30),                                             # nothing
        c + one(c),                                         # flush against both ends; the exact copy wins, not tied
    ]
    want = [(0, 0, 1, 7, 7 + m), (3, 0, 0, 12 + m, 12 + 2 * m), (1, 1, 1, 11 + m, 11 + 2 * m), (1, 0, 0, 4, 4 + m), NONE, (3, 0, 0, 0, m)]
    cache = {}
    assert oracle_model(mode, pats, seqs, k, cache) == want, "the model agrees with the hand-built answers"
    _, st = _assign(engine, seqs, mode, pats, k, cache, want=want)
    assert (st["verify_form"] == FORM_KERNEL) == rides


@pytest.mark.parametrize("forced", [False, True])
def test_equal_start_two_lengths(engine, force_pass, forced):
    """Levenshtein: rows of the winner with equal distance and equal start and two lengths — the longer one.  The cases
    are searched for with the oracle (small alphabets make them): patterns whose best rows in their own read differ only
    in their ends."""
    force_pass(forced)
    rnd = random.Random(1211)
    k = 3
    pats, seqs = [], []
    while len(pats) < 8:
        sig = rnd.choice([b"AC", b"ACG"])
        p = _rand(rnd, sig, rnd.choice([16, 17, 20]))
        read = _rand(rnd, sig, 6) + gpu_cases.edited(rnd, p, rnd.randint(1, k), sig) + _rand(rnd, sig, 6)
        rows = raw_rows(LEV, p, read, k, {})
        if not rows:
            continue
        d = min(r[2] for r in rows)
        st = min(r[0] for r in rows if r[2] == d)
        if len(set(r[1] for r in rows if r[2] == d and r[0] == st)) > 1:
            pats.append(p)
            seqs.append(read)
    cache = {}
    want, _ = _assign(engine, seqs, LEV, pats, k, cache)
    two = 0
    for j, (i, d, _tied, st, en) in enumerate(want):
        ends = set(r[1] for r in raw_rows(LEV, pats[i], seqs[j], k, cache) if r[2] == d and r[0] == st)
        assert en == max(ends)
        two += len(ends) > 1
    assert two >= 4, two


@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_seams(engine, force_pass, mode):
    force_pass(True)
    rnd = random.Random(1212 + mode)
    k, m, alpha = 2, 20, b"ACGT"
    L = m // (k + 1)
    pats = [_rand(rnd, alpha, m) for _ in range(8)]
    assert _plan_groups(pats, k, mode) == 1
    cache = {}
    # a copy cut by the seam between two reads, at every split: neither read is assigned beyond what the oracle says
    seqs = []
    for cut in range(1, m):
        v = _edit(rnd, mode, pats[cut % len(pats)], cut % (k + 1), alpha)
        c = min(cut, len(v) - 1)
        seqs += [_rand(rnd, BG, 40) + v[:c], v[c:] + _rand(rnd, BG, 40)]
    want, st = _assign(engine, seqs, mode, pats, k, cache, what="every split")
    assert st["verify_form"] == FORM_KERNEL and st["filter_launches"] == 1
    # (k < cut < m - k: no part of the copy is within the budget on its own)
    assert sum(w == NONE for w in want) >= 2 * (m - 1 - 2 * (k + 1)), want
    # a copy flush against a seam on either side: assigned to the right read
    p, q = pats[0], pats[5]
    seqs = [_rand(rnd, BG, 30) + p, q + _rand(rnd, BG, 30), _rand(rnd, BG, 10) + p]
    want, _ = _assign(engine, seqs, mode, pats, k, cache, what="flush")
    assert want == [(0, 0, 0, 30, 50), (5, 0, 0, 0, 20), (0, 0, 0, 10, 30)]
    # seams at a tile boundary and around it; degenerate reads give -1 rows in place
    short = [p[:n] for n in (0, 1, L - 1, L, m - k - 1)]
    for seam in (TILE - (L - 1), TILE - 1, TILE, TILE + 1, TILE + (L - 1)):
        a = bytearray(_rand(rnd, BG, seam))
        b = bytearray(_rand(rnd, BG, 300))
        a[:m] = pats[2]                                     # the first read starts the buffer
        a[seam - m:] = pats[3]                              # ends exactly at the seam
        b[:m] = pats[1]                                     # starts exactly at it
        b[300 - m:] = pats[4]                               # the last read ends with the buffer
        for seqs in ([bytes(a), bytes(b)], [bytes(a)] + short + [bytes(b)] + short):
            want, st = _assign(engine, seqs, mode, pats, k, cache, what=("tile seam", seam, len(seqs)))
            assert st["verify_form"] == FORM_KERNEL
            assert want[0] == (2, 0, 1, 0, m) and want[len(seqs) - 1 - (len(seqs) > 2) * len(short)] == (1, 0, 1, 0, m)
            if len(seqs) > 2:
                assert want[1:1 + len(short)] == [NONE] * len(short) and want[-len(short):] == [NONE] * len(short)
    # all reads empty, no reads, no patterns: rows of -1, nothing launched
    for seqs in ([b""] * 5, []):
        want, st = _assign(engine, seqs, mode, pats, k, cache)
        assert want == [NONE] * len(seqs) and st["filter_launches"] == 0 and st["bytes_scanned"] == 0
    want, st = _assign(engine, [p + q, b"", q], mode, [], k, cache)
    assert want == [NONE] * 3 and st["filter_launches"] == 0


@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_several_passes_and_the_loop(engine, force_pass, mode):
    force_pass(True)
    rnd = random.Random(1213 + mode)
    alpha, k = b"ACGT", 2
    pats = [_rand(rnd, alpha, 20) for _ in range(150)]
    pats.insert(40, _rand(rnd, alpha, 129))                 # outside the batched domain: longer than 128
    pats.insert(100, _rand(rnd, alpha, 3 * (k + 1)))        # ... and n-grams of 3
    group_of, ng = _native.multi_plan(pats, k, mode)
    assert ng == 3 and [i for i, g in enumerate(group_of) if g is None] == [40, 100]
    seqs = []
    for j in range(200):
        t = bytearray(_rand(rnd, BG, rnd.randint(100, 200)))
        i = (7 * j) % len(pats)
        v = _edit(rnd, mode, pats[i], j % (k + 1), alpha)
        if len(v) > len(t):
            t = bytearray(_rand(rnd, BG, 200))
        at = rnd.choice([0, len(t) - len(v), rnd.randint(0, len(t) - len(v))])
        t[at:at + len(v)] = v
        seqs.append(bytes(t))
    cache = {}
    blob, offs = pack(seqs)
    h = engine.upload_batch(blob, offs)
    try:
        got, st, multi = _assign_and_multi(engine, h, mode, pats, k)
    finally:
        h.release()
    want = oracle_model(mode, pats, seqs, k, cache)
    assert as_tuples(got) == want
    assert st["verify_form"] == FORM_KERNEL and st["filter_launches"] == multi["filter_launches"] >= ng + 2
    assert st["bytes_scanned"] == multi["bytes_scanned"] >= (ng + 2) * len(blob) and st["raw_matches"] == multi["raw_matches"]
    winners = set(w[0] for w in want)
    assert {40, 100} <= winners and set(group_of[i] for i in winners if i >= 0) == {None, 0, 1, 2}, "winners in every group and both looped patterns"
    assert sum(w[0] >= 0 for w in want) == 200


@pytest.mark.parametrize("one_sequence", [False, True])
@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_overflow_and_contention(force_pass, mode, one_sequence):
    """More than 2^16 records (periodic patterns over reads made of them): the group's launches are run again and only the
    attempt that held is folded.  The same bytes as ONE sequence: every record lands in one table entry — the case the
    load in front of the atomic exists for."""
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
    if one_sequence:
        seqs = [b"".join(seqs)]
    eng = _native.Engine([0])
    try:
        want, st = _assign(eng, seqs, mode, pats, k, {})
        assert st["verify_form"] == FORM_KERNEL and st["filter_launches"] >= 2, "the first sizing should not have held this"
        assert st["raw_matches"] > (1 << 16) and all(w[0] >= 0 for w in want)
    finally:
        eng.close()


def test_refusals_and_state(engine, force_pass):
    force_pass(True)
    rnd = random.Random(1214)
    alpha, k = b"ACGT", 2
    seqs = [_rand(rnd, alpha, 200) for _ in range(20)]
    pats = [seqs[4][50:70], seqs[9][100:120], seqs[0][:20], seqs[19][180:]]
    blob, offs = pack(seqs)
    hb = engine.upload_batch(blob, offs)
    hs = engine.upload(blob)
    before_batch = _flat(*engine.batch_search(hb, LEV, pats[0], k))
    before_multi = [_flat(*x) for x in engine.batch_search_multi(hb, LEV, pats, k)]
    before_subs = engine.subs_ngrams_multi(hs, pats, k)

    def same_refusal(handle, mode, patterns, budget, eng=engine):
        with pytest.raises(Exception) as multi:
            eng.batch_search_multi(handle, mode, patterns, budget)
        with pytest.raises(Exception) as best:
            eng.batch_assign(handle, mode, patterns, budget)
        assert type(best.value) is type(multi.value), (best.value, multi.value)
        assert str(best.value) == str(multi.value).replace("fz_batch_search_multi", "fz_batch_assign")
        return best.value

    assert isinstance(same_refusal(hs, LEV, pats, k), ValueError)                        # a plain handle
    for mode in (EXACT, 3):
        assert isinstance(same_refusal(hb, mode, pats, k), ValueError)
    engine.lev_ngrams_begin(hs, pats[0], k)                                               # a search still in flight
    try:
        assert isinstance(same_refusal(hb, LEV, pats, k), ValueError)
    finally:
        engine.lev_ngrams_end()
    for mode in (LEV, SUBS):                                                              # a bad pattern inside the list
        for bad in (b"", b"AC", b"G"):
            same_refusal(hb, mode, [pats[0], bad, pats[1]], k)
    two = _native.Engine([0, 0])
    try:
        h2 = two.upload(blob)
        assert isinstance(same_refusal(h2, LEV, pats, k, eng=two), _native.UnsupportedSearch)
        h2.release()
    finally:
        two.close()
    # the tables' domain: a budget of 128 (that batch_search_multi takes: patterns of 600 are searched one by one)
    long = [_rand(rnd, alpha, 600), _rand(rnd, alpha, 600)]
    with pytest.raises(_native.UnsupportedSearch):
        engine.batch_assign(hb, LEV, long, 128)
    with pytest.raises(_native.UnsupportedSearch):
        engine.batch_assign(hb, SUBS, long, 128)
    # ... and everything works as before: the call itself, and the calls that share its buffers
    cache = {}
    for mode in (LEV, SUBS):
        got = engine.batch_assign(hb, mode, pats, k)
        assert engine.stats()["verify_form"] == FORM_KERNEL
        want = oracle_model(mode, pats, seqs, k, cache)
        assert as_tuples(got) == want and sum(w[0] >= 0 for w in want) >= 4
    assert _flat(*engine.batch_search(hb, LEV, pats[0], k)) == before_batch
    assert [_flat(*x) for x in engine.batch_search_multi(hb, LEV, pats, k)] == before_multi
    assert engine.subs_ngrams_multi(hs, pats, k) == before_subs and sum(len(r) for r in before_subs) >= 4
    hb.release()
    hs.release()


# ---- the public call ------------------------------------------------------------------------------------------------

L2 = dict(max_l_dist=2)
S2 = dict(max_substitutions=2, max_insertions=0, max_deletions=0)


def _edit_distance(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1]


def _from_multi(nested):
    """(pattern, dist, tied) per sequence from find_near_matches_multi_batch's output."""
    out = []
    for j in range(len(nested[0])):
        best = [min(x.dist for x in per[j]) if per[j] else None for per in nested]
        have = [d for d in best if d is not None]
        if not have:
            out.append((-1, -1, False))
            continue
        d = min(have)
        out.append((best.index(d), d, best.count(d) > 1))
    return out


def _check_public(engine, pats, seqs, limits, held=None):
    import fuzzysearch_amd as fa
    from fuzzysearch_amd import batch, multi_batch
    from fuzzysearch_amd.common import LevenshteinSearchParams
    got = fa.find_best_matches_batch(pats, held if held is not None else seqs, **limits)
    nested = fa.find_near_matches_multi_batch(pats, held if held is not None else seqs, **limits)
    assert len(got) == len(seqs)
    assert list(zip(got.pattern.tolist(), got.dist.tolist(), got.tied.tolist())) == _from_multi(nested)
    kind = batch.batch_kind(list(seqs))
    params = LevenshteinSearchParams(limits.get("max_substitutions"), limits.get("max_insertions"), limits.get("max_deletions"),
                                     limits.get("max_l_dist"))
    riding, mode, k = multi_batch.multi_batch_routes(pats, kind, params)
    generic = all(limits.get(x) is not None for x in ("max_substitutions", "max_insertions", "max_deletions")) and \
        (limits["max_insertions"] or limits["max_deletions"])
    assigned = 0
    raw = {}
    hb = engine.upload_batch(*pack([s.encode("latin-1") if kind == "str" else bytes(s) for s in seqs])) if riding else None
    for j, (i, d, st, en) in enumerate(zip(got.pattern.tolist(), got.dist.tolist(), got.start.tolist(), got.end.tolist())):
        if i < 0:
            assert (d, st, en) == (-1, -1, -1)
            continue
        assigned += 1
        if i in riding:                                     # a row of the winner at dist in the engine's raw stream
            if i not in raw:
                p = pats[i].encode("latin-1") if kind == "str" else bytes(pats[i])
                raw[i] = set(_flat(*engine.batch_search(hb, {"lev": LEV, "subs": SUBS}[mode], p, k, reduced=False)))
            assert any(r[:4] == (j, st, en, d) for r in raw[i]), (j, i, st, en, d)
        else:                                               # ... or one of the public matches
            assert any((x.start, x.end, x.dist) == (st, en, d) for x in nested[i][j]), (j, i, st, en, d)
        piece, p = seqs[j][st:en], pats[i]
        if isinstance(piece, str):
            piece, p = piece.encode("latin-1"), p.encode("latin-1")
        # the matched text is within dist of the pattern.  (Not asked of separate limits: there the reference's own Match can
        # carry a dist below the edit distance of its matched text — b"AGCCTGGC" in a read holding b"AGTCTG", one of each
        # edit and max_l_dist = 2, is (start, start + 6, dist 2) at edit distance 3; b"ACG" in b"AGTAT" is (0, 1, dist 1) —
        # and this package returns what the reference returns.  Such a position is one of the public matches, checked above.)
        if not generic:
            assert _edit_distance(bytes(p), bytes(piece)) <= d, (j, i, st, en, d)
    if hb is not None:
        hb.release()
    return assigned, len(riding)


def test_public_api(engine):
    import fuzzysearch_amd as fa
    rnd = random.Random(1215)
    spats = ["".join(rnd.choice("ACGT") for _ in range(m)) for m in (24, 24, 24, 20, 20, 32, 24, 24, 24, 24, 33, 64)]
    sseqs = _reads(rnd, spats)
    bpats, bseqs = [p.encode() for p in spats], [s.encode() for s in sseqs]
    assigned = 0
    for limits in (L2, S2):
        a, r = _check_public(engine, bpats, bseqs, limits)
        assert r == len(bpats)
        assigned += a
        # (latin-1 str: Levenshtein rides the pass, substitutions-only loops read by read — fewer of them)
        ps, ss = (spats, sseqs) if limits is L2 else (spats[:4], sseqs[:60])
        assigned += _check_public(engine, ps, ss, limits)[0]
    # (a floor from the inputs alone, as in test_gpu_multi_batch: 3 / 8 of the 150 reads are 150 bytes or longer, 60 % of
    # those carry a copy, a third of the copies are exact and found under either limit)
    assert assigned >= 30
    # a resident batch reused across two lists; exact, n-gram, linear-programming and generic-limit routes in one list
    held = fa.resident_batch(bseqs)
    try:
        assigned = _check_public(engine, bpats[:6], bseqs, L2, held=held)[0]
        second = [p[2:] for p in bpats[:3]] + [bytearray(bpats[4]), memoryview(bpats[5])]
        assigned += _check_public(engine, second, bseqs, S2, held=held)[0]
        # (8 characters at k = 2: linear programming under max_l_dist, the generic n-gram search under separate limits)
        routes = [bpats[0], bpats[2], bpats[3][:8], next(s for s in bseqs if len(s) >= 150)[3:27], bpats[0], bpats[1][:8]]
        for limits in (L2, S2, dict(max_l_dist=0), dict(max_substitutions=1, max_insertions=1, max_deletions=1, max_l_dist=2)):
            a, r = _check_public(engine, routes, bseqs, limits, held=held)
            assert a >= 1 and (r > 0) == (limits in (L2, S2))
            assigned += a
    finally:
        held.release()
    assert assigned >= 30
    with pytest.raises(ValueError) as e1:
        fa.find_near_matches_batch(b"", bseqs, **L2)
    with pytest.raises(ValueError) as e2:
        fa.find_best_matches_batch([bpats[0], b"", bpats[1]], bseqs, **L2)
    assert str(e1.value) == str(e2.value)
