"""-m gpu: the multi-pattern search (fz_lev_ngrams_multi / find_near_matches_multi) — every pattern's slice bit-exact and
ordered against the oracle and against the engine's own single call."""
import random

import numpy as np
import pytest

import oracle
from tests import gpu_cases, workloads

pytestmark = pytest.mark.gpu

TILE = 16384


def _rows(arr):
    return [tuple(int(x) for x in r) for r in arr.tolist()]


def _check(engine, h, text, pats, k, vs_oracle=True, vs_single=True):
    """The multi call on resident `h` (= text) against the oracle and the single calls, raw and consolidated."""
    raw = engine.lev_ngrams_multi(h, pats, k)
    assert len(raw) == len(pats)
    st = engine.stats()
    assert st["raw_matches"] == sum(len(r) for r in raw)
    cons = engine.lev_ngrams_multi_consolidated(h, pats, k)
    n_rows = 0
    for i, p in enumerate(pats):
        if vs_oracle:
            exp = oracle.lev_ngrams_raw(p, text, k)
            assert raw[i] == exp, ("raw vs oracle", i, p, k, len(text))
            assert [r[:3] for r in cons[i]] == oracle.consolidate(exp), ("consolidated vs oracle", i, p, k)
        if vs_single:
            assert raw[i] == engine.lev_ngrams(h, p, k), ("raw vs single", i, p, k)
            assert cons[i] == engine.lev_ngrams_consolidated(h, p, k), ("consolidated vs single", i, p, k)
        n_rows += len(raw[i])
    return n_rows, st


def _random_list(rnd, k):
    """1 .. 40 patterns of mixed lengths over one alphabet, and a text with planted edited copies (gpu_cases.random_cases's
    alphabets and planting), from empty to a few tiles."""
    alpha = bytes(rnd.sample(range(1, 256), rnd.choice([2, 3, 4, 4, 20, 200])))
    lengths = [rnd.choice([k + 1, 3 * (k + 1), 4 * (k + 1), 5 * (k + 1) + 2, 20, 32, 64, 128, 150]) for _ in range(rnd.randint(1, 3))]
    pats = []
    for _ in range(rnd.randint(1, 40)):
        m = max(k + 1, rnd.choice(lengths))
        pats.append(bytes(rnd.choice(alpha) for _ in range(m)))
    n = rnd.choice([0, 1, rnd.randint(2, 40), rnd.randint(100, TILE), rnd.randint(TILE, 3 * TILE + 100), 2 * TILE])
    t = bytearray(rnd.choice(alpha) for _ in range(n))
    for p in pats:
        for _rep in range(2):
            if n > len(p) + 10 and rnd.random() < 0.8:
                v = gpu_cases.edited(rnd, p, rnd.randint(0, k), alpha)
                st = rnd.choice([0, 1, n - len(v) - 1, n - len(v), rnd.randint(0, max(0, n - len(v)))])
                st = max(0, min(st, n - len(v)))
                t[st:st + len(v)] = v
    return pats, bytes(t)


def test_random_lists(engine):
    rnd = random.Random(81)
    from fuzzysearch_amd import _native
    rows = batched = 0
    for it in range(40):
        k = [1, 2, 3, 4, 8][it % 5]
        pats, text = _random_list(rnd, k)
        h = engine.upload(text)
        n, st = _check(engine, h, text, pats, k)
        h.release()
        rows += n
        assert (st["verify_form"] == 5) == (_native.multi_plan(pats, k)[1] > 0), "a planned group runs batched"
        batched += st["verify_form"] == 5
    assert rows > 500 and batched >= 1


def test_adversarial_lists(engine):
    rnd = random.Random(82)
    base = bytes(rnd.choice(b"ACGT") for _ in range(26))
    text = bytearray(rnd.choice(b"ACGT") for _ in range(3 * TILE + 77))
    for at in (0, 5000, TILE - 7, 2 * TILE - 13, len(text) - 26):
        text[at:at + 26] = base
    text[9000:9300] = b"A" * 300                                       # a run of one symbol
    text[TILE - 40:TILE + 40] = b"C" * 80                             # ... and one across a tile seam
    rep = b"ACGTAC" + b"GATTAC" + b"ACGTAC" + b"TT"                     # a pattern with a repeated n-gram (blocks 0 and 2)
    text[20000:20020] = rep
    text = bytes(text)
    pats = [base[:20], base[:20], base[1:21], base[2:22], base[3:23], base[6:26],      # duplicates, shifts of one another
            rep, b"A" * 20, b"C" * 20, b"A" * 20, base[4:24]]
    h = engine.upload(text)
    n, st = _check(engine, h, text, pats, 2)
    assert n > 300 and st["verify_form"] == 5 and st["filter_launches"] == 1
    # the single-symbol pattern over a text that is nothing but that symbol
    run = b"G" * 5000
    h2 = engine.upload(run)
    _check(engine, h2, run, [b"G" * 12, b"G" * 14, b"GGGGGGGGGGGA"], 2)
    h.release()
    h2.release()


def test_dense_case_and_overflow(engine):
    """64 DNA patterns, m = 12, k = 2: 192 of the 256 possible 4-mers are blocks — three quarters of all offsets are hits."""
    rnd = random.Random(83)
    kmers = [bytes(b"ACGT"[(q >> (2 * j)) & 3] for j in range(4)) for q in range(256)]
    rnd.shuffle(kmers)
    pats = [kmers[3 * i] + kmers[3 * i + 1] + kmers[3 * i + 2] for i in range(64)]
    text = workloads.dna(256 << 10, 5).tobytes()
    h = engine.upload(text)
    n, st = _check(engine, h, text, pats, 2, vs_single=False)
    assert n > 0                  # (the planner's cost rule gives a list this dense to the loop: the slices are what counts)
    assert engine.lev_ngrams_multi(h, pats[:5], 2) == [engine.lev_ngrams(h, p, 2) for p in pats[:5]]
    h.release()
    # far more hits and records than the sizing from the arguments expects (8 patterns of 20 over four letters: 24 n / 4^6
    # hits; the text is the patterns themselves over and over: 3 n / 20 hits and as many records): the lists overflow, the
    # launch is run again with what its counters ask for, nothing is lost
    from fuzzysearch_amd import _native
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(8)]
    assert _native.multi_plan(pats, 2) == ([0] * 8, 1)
    unit = b"".join(pats)
    text = unit * ((1 << 20) // len(unit))
    h = engine.upload(text)
    raw = engine.lev_ngrams_multi(h, pats, 2)
    st = engine.stats()
    assert st["verify_form"] == 5 and st["filter_launches"] >= 2, "the first sizing should not have held this"
    for i in range(8):
        assert raw[i] == oracle.lev_ngrams_raw(pats[i], text, 2)
        assert len(raw[i]) >= 3 * (len(text) // len(unit))
    h.release()


def test_seams(engine):
    """Copies straddling every tile boundary of a five-tile text, at every split, and at both ends of the buffer."""
    rnd = random.Random(84)
    k, m = 2, 20
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(m)) for _ in range(8)]
    n = 5 * TILE
    total = 0
    for delta in range(0, m + k + 2):
        t = bytearray(workloads.dna(n, 100 + delta).tobytes())
        for b in range(TILE, n, TILE):
            p = pats[(delta + b // TILE) % len(pats)]
            t[b - delta:b - delta + m] = p                              # `delta` bytes before the boundary, the rest behind it
        t[0:m] = pats[delta % len(pats)]
        t[n - m:n] = pats[(delta + 3) % len(pats)]
        text = bytes(t)
        h = engine.upload(text)
        raw = engine.lev_ngrams_multi(h, pats, k)
        for i, p in enumerate(pats):
            assert raw[i] == oracle.lev_ngrams_raw(p, text, k), (delta, i)
            total += len(raw[i])
        h.release()
    assert total >= (m + k + 2) * 6


def test_several_passes(engine):
    rnd = random.Random(85)
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(300)]
    t = bytearray(workloads.dna(4 * TILE + 123, 6).tobytes())
    for j in range(0, 300, 7):
        at = rnd.randint(0, len(t) - 20)
        t[at:at + 20] = gpu_cases.edited(rnd, pats[j], rnd.randint(0, 2), b"ACGT")[:20].ljust(20, b"A")
    text = bytes(t)
    h = engine.upload(text)
    raw = engine.lev_ngrams_multi(h, pats, 2)
    st = engine.stats()
    assert st["filter_launches"] == 5 and st["bytes_scanned"] == 5 * len(text)
    for i, p in enumerate(pats):
        assert raw[i] == oracle.lev_ngrams_raw(p, text, 2), i
    assert sum(len(r) for r in raw) >= 40
    h.release()


def test_shared_pass(engine):
    """32 patterns of one length: the filter launches and the bytes streamed are those of ONE single search."""
    rnd = random.Random(86)
    text = workloads.dna(1 << 20, 7).tobytes()
    for (m, k) in ((20, 2), (32, 2), (24, 1), (40, 4)):
        pats = [bytes(rnd.choice(b"ACGT") for _ in range(m)) for _ in range(32)]
        h = engine.upload(text)
        single = engine.lev_ngrams(h, pats[0], k)
        one = engine.stats()
        multi = engine.lev_ngrams_multi(h, pats, k)
        st = engine.stats()
        assert one["filter_launches"] == 1 and one["bytes_scanned"] == len(text)
        assert st["filter_launches"] == one["filter_launches"] and st["bytes_scanned"] == one["bytes_scanned"]
        assert st["verify_form"] == 5 and st["raw_matches"] == sum(len(r) for r in multi)
        assert multi[0] == single
        h.release()


def test_pipeline_outstanding_is_refused(engine):
    text = workloads.dna(1 << 16, 8).tobytes()
    p = text[100:120]
    h = engine.upload(text)
    engine.lev_ngrams_begin(h, p, 2)
    try:
        with pytest.raises(ValueError):
            engine.lev_ngrams_multi(h, [p, p], 2)
    finally:
        engine.lev_ngrams_end()
    with pytest.raises(ValueError):
        engine.lev_ngrams_multi(h, [p, b""], 2)
    with pytest.raises(ValueError):
        engine.lev_ngrams_multi(h, [p, b"AC"], 2)
    assert engine.lev_ngrams_multi(h, [], 2) == []
    h.release()


def test_sharded_sequence():
    """Three device states on one GPU, small shards placed far apart in a global sequence of 8 GiB (indices beyond 2^32
    through buf_global_off): every slice equals the single call on the same sequence."""
    from fuzzysearch_amd import _native
    rnd = random.Random(87)
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
                        buf[at:at + len(p)] = gpu_cases.edited(rnd, p, rnd.randint(0, 2), b"ACGT")[:len(p)].ljust(len(p), b"C")
            lo = offs[r] + (halo if r else 0)
            hi = offs[r] + blen - (halo if r < world - 1 else 0)
            eng.add_shard(h, r, bytes(buf), offs[r], lo, hi)
        for k in (2, 1):
            raw = eng.lev_ngrams_multi(h, pats, k, as_array=True)
            st = eng.stats()
            assert st["verify_form"] == 5
            total = 0
            for i, p in enumerate(pats):
                single = eng.lev_ngrams(h, p, k, as_array=True)
                assert np.array_equal(raw[i], single), (k, i)
                total += len(single)
            assert total > 40 and any(int(r["start"].max()) > (1 << 32) for r in raw if len(r))
            cons = eng.lev_ngrams_multi_consolidated(h, pats, k)
            assert cons == [eng.lev_ngrams_consolidated(h, p, k) for p in pats]
        h.release()
    finally:
        eng.close()


def _triples(matches):
    return [(x.start, x.end, x.dist, x.matched) for x in matches]


def test_public_api():
    import fuzzysearch_amd as fa
    rnd = random.Random(88)
    alpha = b"ACGT"
    pats = [bytes(rnd.choice(alpha) for _ in range(m)) for m in (20, 20, 24, 32, 20, 64, 20, 20, 20, 20)]
    t = bytearray(workloads.dna(200000, 9).tobytes())
    for j, p in enumerate(pats):
        for at in (0, 777 + 1000 * j, TILE - 9 + j, len(t) - len(p)):
            v = gpu_cases.edited(rnd, p, rnd.randint(0, 2), alpha)
            t[at:at + len(v)] = v
    data = bytes(t)
    text = data.decode("latin-1")
    spats = [p.decode("latin-1") for p in pats]
    wide = text[:5000] + "Ж中" + text[5000:30000]
    sequences = [
        (pats, data), (pats, bytearray(data)), (spats, text), (spats, wide), (spats + ["Ж" + spats[0][1:]], text),
        ([list(p) for p in pats], list(data[:30000])),
    ]
    for ps, seq in sequences:
        got = fa.find_near_matches_multi(ps, seq, max_l_dist=2)
        exp = [fa.find_near_matches(p, seq, max_l_dist=2) for p in ps]
        assert [_triples(g) for g in got] == [_triples(e) for e in exp], type(seq)
        assert sum(len(g) for g in got) >= len(ps)
    from fuzzysearch_amd import _native
    assert _native.multi_plan(pats, 2)[1] == 1, "the list is meant to ride a pass"
    r = fa.resident(data)
    assert [_triples(g) for g in fa.find_near_matches_multi(pats, r, max_l_dist=2)] == \
        [_triples(fa.find_near_matches(p, data, max_l_dist=2)) for p in pats]
    r.release()
    # a list mixing routes: the exact route (k = 0 is a different call), a linear-programming pattern, one beyond 128 characters
    mixed = [pats[0], pats[0][:5], data[1000:1140], pats[1], data[50000:50200], pats[2][:8]]
    for kw in ({"max_l_dist": 2}, {"max_l_dist": 0}, {"max_substitutions": 2, "max_insertions": 0, "max_deletions": 0},
               {"max_substitutions": 1, "max_insertions": 1, "max_deletions": 1, "max_l_dist": 2}, {"max_l_dist": 1}):
        got = fa.find_near_matches_multi(mixed, data, **kw)
        exp = [fa.find_near_matches(p, data, **kw) for p in mixed]
        assert [_triples(g) for g in got] == [_triples(e) for e in exp], kw
    # the first offending pattern raises what find_near_matches raises
    with pytest.raises(ValueError) as e1:
        fa.find_near_matches(b"", data, max_l_dist=2)
    with pytest.raises(ValueError) as e2:
        fa.find_near_matches_multi([pats[0], b"", pats[1]], data, max_l_dist=2)
    assert str(e1.value) == str(e2.value)
    with pytest.raises(TypeError):
        fa.find_near_matches_multi([pats[0], spats[1]], data, max_l_dist=2)
    # one preparation per call: one acquire of the residency cache for 6 patterns on 3 routes
    fa.cache_clear()
    before = fa.cache_info()
    fa.find_near_matches_multi(mixed, data, max_l_dist=2)
    mid = fa.cache_info()
    fa.find_near_matches_multi(mixed, data, max_l_dist=2)
    after = fa.cache_info()
    assert (mid["hits"] - before["hits"], mid["misses"] - before["misses"]) == (0, 1)
    assert (after["hits"] - mid["hits"], after["misses"] - mid["misses"]) == (1, 0)
    fa.cache_clear()


def test_size_256_mib(engine):
    """256 MiB of DNA, 64 patterns of m = 20, k = 2, planted variants of several of them."""
    seq = workloads.dna(256 << 20, 20250925)
    pats = [workloads.dna(20, 1000 + i) for i in range(64)]
    for i in range(0, 64, 5):
        workloads.plant_variants(seq, pats[i], 40, 7 + i)
    text = seq.tobytes()
    pats = [p.tobytes() for p in pats]
    h = engine.upload(seq)
    raw = engine.lev_ngrams_multi(h, pats, 2, as_array=True)
    st = engine.stats()
    assert st["filter_launches"] == 1 and st["bytes_scanned"] == len(text) and st["verify_form"] == 5
    total = 0
    for i, p in enumerate(pats):
        single = engine.lev_ngrams(h, p, 2, as_array=True)
        assert np.array_equal(raw[i], single), i
        total += len(single)
    assert total >= 13 * 40                                     # every planted variant (at most one edit) is a row at least
    for i in (0, 37):
        assert _rows(raw[i]) == oracle.lev_ngrams_raw(pats[i], text, 2)
    h.release()
