"""-m gpu: the substitutions-only multi-pattern search (fz_subs_ngrams_multi / find_near_matches_multi with
max_insertions = max_deletions = 0) — every pattern's slice bit-exact and ordered against the oracle and against the
engine's own single call."""
import random

import numpy as np
import pytest

import oracle
from fuzzysearch_amd import _native
from tests import workloads

pytestmark = pytest.mark.gpu

TILE = 16384
SUBS = _native.MODE_SUBS


def _mutated(rnd, p, nsub, alpha):
    """p with exactly nsub substituted characters."""
    v = bytearray(p)
    for q in rnd.sample(range(len(v)), nsub):
        v[q] = rnd.choice([c for c in alpha if c != v[q]])
    return bytes(v)


def _check(engine, h, text, pats, k, vs_oracle=True, vs_single=True):
    """The multi calls on resident `h` (= text) against the oracle and the single calls, raw and best-of-group."""
    raw = engine.subs_ngrams_multi(h, pats, k)
    assert len(raw) == len(pats)
    st = engine.stats()
    assert st["raw_matches"] == sum(len(r) for r in raw)
    best = engine.subs_ngrams_multi_best(h, pats, k)
    n_rows = 0
    for i, p in enumerate(pats):
        if vs_oracle:
            exp = oracle.subs_ngrams_raw(p, text, k)
            assert raw[i] == exp, ("raw vs oracle", i, p, k, len(text))
            assert [r[:3] for r in best[i]] == [r[:3] for r in oracle.group_best(exp)[0]], ("best vs oracle", i, p, k)
        if vs_single:
            assert raw[i] == engine.subs_ngrams(h, p, k), ("raw vs single", i, p, k)
            assert best[i] == engine.subs_ngrams_best(h, p, k), ("best vs single", i, p, k)
        n_rows += len(raw[i])
    return n_rows, st


def _random_list(rnd, k):
    """1 .. 40 patterns of mixed lengths over one alphabet — inside the batched domain and outside it (beyond 128
    characters, n-grams of 3, 2 and 1) — and a text with planted substituted copies, from empty to a few tiles."""
    alpha = bytes(rnd.sample(range(1, 256), rnd.choice([2, 4, 4, 20, 20, 200])))
    lengths = [rnd.choice([k + 1, 2 * (k + 1) + 1, 3 * (k + 1), 4 * (k + 1), 4 * (k + 1) + 1, 5 * (k + 1) + 2, 20, 23, 32, 64, 128, 129, 150])
               for _ in range(rnd.randint(1, 3))]
    pats = []
    for _ in range(rnd.randint(1, 40)):
        m = max(k + 1, rnd.choice(lengths))
        pats.append(bytes(rnd.choice(alpha) for _ in range(m)))
    n = rnd.choice([0, 1, rnd.randint(2, 40), rnd.randint(100, TILE), rnd.randint(TILE, 3 * TILE + 100), 2 * TILE])
    t = bytearray(rnd.choice(alpha) for _ in range(n))
    for p in pats:
        for _rep in range(2):
            if n > len(p) + 10 and rnd.random() < 0.8:
                v = _mutated(rnd, p, rnd.randint(0, min(k + 1, len(p))), alpha)
                st = rnd.choice([0, 1, n - len(v) - 1, n - len(v), rnd.randint(0, n - len(v))])
                t[st:st + len(v)] = v
    return pats, bytes(t)


RANDOM_SEED, RANDOM_LISTS = 92, 40        # (on the CPU, oracle and planner: 134 402 rows, 19 lists with a group)


def test_random_lists(engine):
    rnd = random.Random(RANDOM_SEED)
    rows = batched = 0
    for it in range(RANDOM_LISTS):
        k = [1, 2, 3, 4, 8][it % 5]
        pats, text = _random_list(rnd, k)
        h = engine.upload(text)
        n, st = _check(engine, h, text, pats, k)
        h.release()
        rows += n
        assert (st["verify_form"] == 5) == (_native.multi_plan(pats, k, SUBS)[1] > 0), "a planned group runs batched"
        batched += st["verify_form"] == 5
    print("random lists: %d rows, %d lists with a batched group" % (rows, batched))
    assert rows > 500 and batched >= 5


def test_seams(engine):
    """Copies with 0 .. k substitutions straddling every tile boundary of a five-tile text at every split 0 .. m, at offset
    0 and at n - m; a text shorter than the pattern and one of exactly m bytes."""
    rnd = random.Random(92)
    k, m = 2, 20
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(m)) for _ in range(8)]
    n = 5 * TILE
    total = 0
    for delta in range(0, m + 1):
        t = bytearray(workloads.dna(n, 100 + delta).tobytes())
        for b in range(TILE, n, TILE):
            p = pats[(delta + b // TILE) % len(pats)]
            t[b - delta:b - delta + m] = _mutated(rnd, p, (delta + b // TILE) % (k + 1), b"ACGT")
        t[0:m] = _mutated(rnd, pats[delta % len(pats)], delta % (k + 1), b"ACGT")
        t[n - m:n] = _mutated(rnd, pats[(delta + 3) % len(pats)], (delta + 1) % (k + 1), b"ACGT")
        text = bytes(t)
        h = engine.upload(text)
        raw = engine.subs_ngrams_multi(h, pats, k)
        assert engine.stats()["verify_form"] == 5
        for i, p in enumerate(pats):
            assert raw[i] == oracle.subs_ngrams_raw(p, text, k), (delta, i)
            total += len(raw[i])
        h.release()
    assert total >= (m + 1) * 6
    for text in (pats[0][:m - 1], pats[0], _mutated(rnd, pats[1], k, b"ACGT"), _mutated(rnd, pats[1], k + 1, b"ACGT"), b"A"):
        h = engine.upload(text)
        _check(engine, h, text, pats, k)
        h.release()


def test_adversarial_lists(engine):
    rnd = random.Random(93)
    base = bytes(rnd.choice(b"ACGT") for _ in range(26))
    text = bytearray(rnd.choice(b"ACGT") for _ in range(3 * TILE + 77))
    for j, at in enumerate((0, 5000, TILE - 7, 2 * TILE - 13, len(text) - 26)):
        text[at:at + 26] = _mutated(rnd, base, j % 3, b"ACGT")
    text[9000:9300] = b"A" * 300                                       # a run of one symbol
    text[TILE - 40:TILE + 40] = b"C" * 80                             # ... and one across a tile seam
    rep = b"ACGTAC" + b"GATTAC" + b"ACGTAC" + b"TT"                     # a pattern with a repeated n-gram (blocks 0 and 2)
    text[20000:20020] = rep
    text[21000:21020] = rep[:6] + b"GATTAG" + b"ACGTAC" + b"TT"
    # a window within the budget whose substitutions all lie in block 0 of base[:20]: blocks 1 and 2 find it, block 0 must not
    only_others = bytearray(base[:20])
    only_others[1] = ord("A") if base[1] != ord("A") else ord("C")
    only_others[4] = ord("G") if base[4] != ord("G") else ord("T")
    text[30001:30021] = only_others
    text = bytes(text)
    pats = [base[:20], base[:20], base[1:21], base[2:22], base[3:23], base[6:26],      # duplicates, shifts of one another
            rep, b"A" * 20, b"C" * 20, b"A" * 20, base[4:24]]
    h = engine.upload(text)
    n, st = _check(engine, h, text, pats, 2)
    assert n > 300 and st["verify_form"] == 5 and st["filter_launches"] == 1
    raw = engine.subs_ngrams_multi(h, pats, 2)
    at30001 = [r for r in raw[0] if r[0] == 30001]
    assert [(r[2], r[3]) for r in at30001] == [(2, 1), (2, 2)], "no row under the block that does not match"
    # the single-symbol pattern over a text that is nothing but that symbol
    run = b"G" * 5000
    h2 = engine.upload(run)
    _check(engine, h2, run, [b"G" * 12, b"G" * 14, b"GGGGGGGGGGGA", b"G" * 13, b"AGGGGGGGGGGG"], 2)
    h.release()
    h2.release()


def test_overflow():
    """Far more hits and records than the sizing from the arguments expects (8 patterns of 20 over four letters: 24 n / 4^6
    hits; the text is the patterns themselves over and over): the launch is run again with what its counters ask for.
    On an engine of its own: the hit lists and the record buffer of a context keep the size an earlier search grew them to."""
    rnd = random.Random(94)
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(8)]
    assert _native.multi_plan(pats, 2, SUBS) == ([0] * 8, 1)
    unit = b"".join(pats)
    text = unit * ((1 << 20) // len(unit))
    eng = _native.Engine([0])
    try:
        h = eng.upload(text)
        raw = eng.subs_ngrams_multi(h, pats, 2)
        st = eng.stats()
        assert st["verify_form"] == 5 and st["filter_launches"] >= 2, "the first sizing should not have held this"
        for i in range(8):
            assert raw[i] == oracle.subs_ngrams_raw(pats[i], text, 2)
            assert len(raw[i]) >= 3 * (len(text) // len(unit))
        h.release()
    finally:
        eng.close()


def test_several_passes(engine):
    rnd = random.Random(95)
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(300)]
    t = bytearray(workloads.dna(4 * TILE + 123, 6).tobytes())
    for j in range(0, 300, 7):
        at = rnd.randint(0, len(t) - 20)
        t[at:at + 20] = _mutated(rnd, pats[j], rnd.randint(0, 2), b"ACGT")
    text = bytes(t)
    group_of, ng = _native.multi_plan(pats, 2, SUBS)
    single = sum(1 for g in group_of if g is None)
    assert ng >= 1
    h = engine.upload(text)
    raw = engine.subs_ngrams_multi(h, pats, 2)
    st = engine.stats()
    # one filter launch per group, one per pattern outside the groups (m = 20, k = 2: three blocks, one scan launch)
    assert st["filter_launches"] == ng + single and st["bytes_scanned"] == (ng + single) * len(text)
    for i, p in enumerate(pats):
        assert raw[i] == oracle.subs_ngrams_raw(p, text, 2), i
    assert sum(len(r) for r in raw) >= 40
    h.release()


def test_pipeline_outstanding_is_refused(engine):
    text = workloads.dna(1 << 16, 8).tobytes()
    p = text[100:120]
    h = engine.upload(text)
    engine.lev_ngrams_begin(h, p, 2)
    try:
        with pytest.raises(ValueError):
            engine.subs_ngrams_multi(h, [p, p], 2)
    finally:
        engine.lev_ngrams_end()
    for bad in (b"", b"AC", b"G"):                               # empty; m <= k: what the single call raises
        with pytest.raises(Exception) as single:
            engine.subs_ngrams(h, bad, 2)
        with pytest.raises(Exception) as multi:
            engine.subs_ngrams_multi(h, [p, bad, p], 2)
        assert type(multi.value) is type(single.value) and str(multi.value) == str(single.value)
        with pytest.raises(type(single.value)):
            engine.subs_ngrams_multi_best(h, [bad], 2)
    assert engine.subs_ngrams_multi(h, [], 2) == []
    h.release()


def test_sharded_sequence():
    """Three device states on one GPU, small shards placed far apart in a global sequence of 8 GiB (indices beyond 2^32):
    every slice equals the single call on the same sequence."""
    rnd = random.Random(97)
    world, blen, halo, n = 3, 100000, 200, 1 << 33
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(m)) for m in (20, 20, 20, 20, 20, 20, 21, 32, 32, 32, 32, 64, 128, 150, 9)]
    offs = [0, (5 << 30) + 12345, n - blen]
    eng = _native.Engine([0] * world)
    try:
        h = eng.new_sequence(n)
        for r in range(world):
            buf = bytearray(workloads.dna(blen, 300 + r).tobytes())
            for j, p in enumerate(pats):
                for at in (halo - 5 + 7 * j, 3000 + 400 * j, TILE - 10 + j, blen - halo - len(p) + 3 * j - 20):
                    if 0 <= at <= blen - len(p):
                        buf[at:at + len(p)] = _mutated(rnd, p, rnd.randint(0, 2), b"ACGT")
            lo = offs[r] + (halo if r else 0)
            hi = offs[r] + blen - (halo if r < world - 1 else 0)
            eng.add_shard(h, r, bytes(buf), offs[r], lo, hi)
        for k in (2, 1):
            assert _native.multi_plan(pats, k, SUBS)[1] >= 1
            raw = eng.subs_ngrams_multi(h, pats, k, as_array=True)
            st = eng.stats()
            assert st["verify_form"] == 5
            total = 0
            for i, p in enumerate(pats):
                single = eng.subs_ngrams(h, p, k, as_array=True)
                assert np.array_equal(raw[i], single), (k, i)
                total += len(single)
            assert total > 40 and any(int(r["start"].max()) > (1 << 32) for r in raw if len(r))
            best = eng.subs_ngrams_multi_best(h, pats, k)
            assert best == [eng.subs_ngrams_best(h, p, k) for p in pats]
        h.release()
    finally:
        eng.close()


def _triples(matches):
    return [(x.start, x.end, x.dist, x.matched) for x in matches]


def test_public_api(engine):
    import fuzzysearch_amd as fa
    rnd = random.Random(98)
    alpha = b"ACGT"
    pats = [bytes(rnd.choice(alpha) for _ in range(m)) for m in (20, 20, 24, 32, 20, 64, 20, 20, 20, 20, 23, 23)]
    t = bytearray(workloads.dna(200000, 9).tobytes())
    for j, p in enumerate(pats):
        for at in (0, 777 + 1000 * j, TILE - 9 + j, len(t) - len(p)):
            t[at:at + len(p)] = _mutated(rnd, p, rnd.randint(0, 2), alpha)
    data = bytes(t)
    text = data.decode("latin-1")
    spats = [p.decode("latin-1") for p in pats]
    wide = text[:5000] + "Ж中" + text[5000:30000]
    assert _native.multi_plan(pats, 2, SUBS)[1] >= 1, "the list is meant to ride a pass"
    for kw in ({"max_substitutions": 2, "max_insertions": 0, "max_deletions": 0},
               {"max_substitutions": 3, "max_insertions": 0, "max_deletions": 0, "max_l_dist": 2}):
        sequences = [
            (pats, data), (pats, bytearray(data)), (spats, text), (spats, wide), (spats + ["Ж" + spats[0][1:]], text),
            ([list(p) for p in pats], list(data[:30000])),
        ]
        for ps, seq in sequences:
            got = fa.find_near_matches_multi(ps, seq, **kw)
            exp = [fa.find_near_matches(p, seq, **kw) for p in ps]
            assert [_triples(g) for g in got] == [_triples(e) for e in exp], (type(seq), kw)
            assert sum(len(g) for g in got) >= len(ps)
        # after the bytes case the engine's stats show a batched pass over the whole list (not the last single search)
        fa.find_near_matches_multi(pats, data, **kw)
        st = engine.stats()
        assert st["verify_form"] == 5 and st["raw_matches"] == sum(len(oracle.subs_ngrams_raw(p, data, 2)) for p in pats)
        r = fa.resident(data)
        assert [_triples(g) for g in fa.find_near_matches_multi(pats, r, **kw)] == \
            [_triples(fa.find_near_matches(p, data, **kw)) for p in pats]
        r.release()
        rs = fa.resident(text)
        assert [_triples(g) for g in fa.find_near_matches_multi(spats, rs, **kw)] == \
            [_triples(fa.find_near_matches(p, text, **kw)) for p in spats]
        rs.release()
        # a list mixing routes: a linear-programming pattern, one beyond 128 characters, n-grams of 3
        mixed = [pats[0], pats[0][:5], data[1000:1140], pats[1], data[50000:50200], pats[2][:8], pats[3][:9]]
        got = fa.find_near_matches_multi(mixed, data, **kw)
        assert [_triples(g) for g in got] == [_triples(fa.find_near_matches(p, data, **kw)) for p in mixed], kw
    kw = {"max_substitutions": 2, "max_insertions": 0, "max_deletions": 0}
    with pytest.raises(ValueError) as e1:
        fa.find_near_matches(b"", data, **kw)
    with pytest.raises(ValueError) as e2:
        fa.find_near_matches_multi([pats[0], b"", pats[1]], data, **kw)
    assert str(e1.value) == str(e2.value)
    with pytest.raises(TypeError):
        fa.find_near_matches_multi([pats[0], spats[1]], data, **kw)
    fa.cache_clear()
