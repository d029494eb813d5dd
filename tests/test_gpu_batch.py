"""-m gpu: one pattern, many sequences, one pass (fz_batch_upload / fz_batch_search / find_near_matches_batch) — every
sequence's rows bit-exact and ordered against the oracle run on that sequence alone."""
import random

import numpy as np
import pytest

import oracle
from tests import gpu_cases

pytestmark = pytest.mark.gpu

TILE = 16384
EXACT, LEV, SUBS = 0, 1, 2


def _rand(rnd, alpha, n):
    return bytes(rnd.choices(alpha, k=n))


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, seqs), dtype=np.uint64, count=len(seqs)), out=offs[1:])
    return b"".join(seqs), offs


def _got(engine, h, mode, p, k, reduced):
    rows, seq_of = engine.batch_search(h, mode, p, k, reduced=reduced)
    assert len(rows) == len(seq_of)
    assert np.all(np.diff(seq_of.astype(np.int64)) >= 0), "seq_of is non-decreasing"
    return [(int(j),) + tuple(int(x) for x in r) for j, r in zip(seq_of.tolist(), rows.tolist())]


def _raw_oracle(mode, p, s, k):
    if mode == EXACT:
        return [(i, i + len(p), 0, -1) for i in oracle.search_exact(p, s)]
    return oracle.lev_ngrams_raw(p, s, k) if mode == LEV else oracle.subs_ngrams_raw(p, s, k)


def _expected(mode, p, seqs, k, cache=None):
    """-> (raw rows, reduced rows) of the whole batch as (sequence, start, end, dist, block); the reduced rows without block."""
    raw, red = [], []
    for j, s in enumerate(seqs):
        key = (mode, bytes(s))
        rows = cache.get(key) if cache is not None else None
        if rows is None:
            rows = _raw_oracle(mode, p, s, k)
            if cache is not None:
                cache[key] = rows
        raw += [(j,) + tuple(r) for r in rows]
        if mode == EXACT:
            best = [r[:3] for r in rows]
        elif mode == LEV:
            best = oracle.consolidate(rows)
        else:
            best = [b[:3] for b in oracle.group_best(rows)[0]]
        red += [(j,) + tuple(b) for b in best]
    return raw, red


def _check(engine, seqs, p, k, modes=(EXACT, LEV, SUBS), what=None):
    """The batch search over `seqs`, raw and reduced, in every mode, against the oracle per sequence.  -> (rows, forms)."""
    blob, offs = _pack(seqs)
    h = engine.upload_batch(blob, offs)
    n_rows, forms = 0, set()
    try:
        for mode in modes:
            kk = 0 if mode == EXACT else k
            raw, red = _expected(mode, p, seqs, kk)
            got = _got(engine, h, mode, p, kk, False)
            st = engine.stats()
            assert got == raw, ("raw", mode, what, p, kk, [len(s) for s in seqs][:20])
            assert st["raw_matches"] == len(raw)
            if mode != EXACT and blob:                             # (a batch without bytes launches nothing: no form)
                forms.add(st["verify_form"])
            got = _got(engine, h, mode, p, kk, True)
            assert [g[:4] for g in got] == red, ("reduced", mode, what, p, kk)
            n_rows += len(raw)
    finally:
        h.release()
    return n_rows, forms


def _random_batch(rnd, p, k, alpha, n_seqs):
    """Sequences of lengths 0 .. ~3 tiles — many short ones per tile, at most two long ones that span tile seams — with
    planted edited copies (gpu_cases' planting: both ends included) and copies cut in two by a seam between sequences."""
    m = len(p)
    seqs, big = [], 0
    for _ in range(n_seqs):
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
            if n >= m - k and rnd.random() < 0.6:
                v = gpu_cases.edited(rnd, p, rnd.randint(0, k), alpha)
                if len(v) <= n:
                    st = rnd.choice([0, 1, n - len(v) - 1, n - len(v), rnd.randint(0, n - len(v))])
                    st = max(0, min(st, n - len(v)))
                    t[st:st + len(v)] = v
        seqs.append(t)
    for j in range(len(seqs) - 1):                       # a copy cut in two by the seam between j and j + 1
        if rnd.random() < 0.3:
            cut = rnd.randint(1, m - 1)
            a, b = seqs[j], seqs[j + 1]
            if len(a) >= cut and len(b) >= m - cut:
                a[len(a) - cut:] = p[:cut]
                b[:m - cut] = p[cut:]
    return [bytes(s) for s in seqs]


def test_random_batches(engine):
    rnd = random.Random(91)
    ks = [1, 2, 3, 4, 8]
    ms = lambda k: [3 * (k + 1), 20, 32, 54, 64, 100, 150]
    # every (k, m) once, then k = 8, m = 150 — the pattern beyond the bit-vector forms — over two symbols (lane-per-cell
    # inside the scan) and over many (the hit-list kernel)
    plan = [(k, m, None) for m_i in range(7) for k in ks for m in [ms(k)[m_i]]]
    plan += [(8, 150, 2), (8, 150, 20), (8, 150, 2), (8, 150, 200), (2, 150, 4)]
    assert len(plan) == 40
    rows, forms = 0, set()
    for it, (k, m, sigma) in enumerate(plan):
        alpha = bytes(rnd.sample(range(1, 256), sigma or rnd.choice([2, 3, 4, 4, 20, 200])))
        p = _rand(rnd, alpha, m)
        n_seqs = rnd.choice([1, 2, rnd.randint(3, 40), rnd.randint(100, 300)])
        seqs = _random_batch(rnd, p, k, alpha, n_seqs)
        n, f = _check(engine, seqs, p, k, what=it)
        rows += n
        forms |= f
    assert rows > 500
    # register band / Hamming count, lane-per-cell, bit-vector columns on 64, 128 and 32 bits, the hit-list kernels
    assert forms == {1, 2, 3, 4, 5, 6}, forms


@pytest.mark.parametrize("mode", [EXACT, LEV, SUBS])
def test_seam_sweep(engine, mode):
    """Two sequences A|B, the seam at tile_edge - 2 .. + 2 and mid-tile, a copy of the pattern — exact, and with k edits —
    at every offset from -(m + k) to +(m + k) around the seam: nothing that needs bytes of both sides, everything flush
    against either side."""
    rnd = random.Random(92 + mode)
    alpha = b"ACGT"
    m, k = 12, (0 if mode == EXACT else 2)
    p = _rand(rnd, alpha, m)
    variants = [p, gpu_cases.edited(random.Random(5), p, 2, alpha)]
    total = TILE + 4000
    bg = _rand(rnd, b"xyz", total)            # background free of the pattern's symbols
    cache = {}
    rows = flush = 0
    for seam in [TILE - 2, TILE - 1, TILE, TILE + 1, TILE + 2, TILE // 2 + 3]:
        for v in variants:
            for off in range(-(m + 2), m + 2 + 1):
                t = bytearray(bg)
                at = seam + off
                t[at:at + len(v)] = v
                seqs = [bytes(t[:seam]), bytes(t[seam:])]
                blob, offs = _pack(seqs)
                h = engine.upload_batch(blob, offs)
                raw, red = _expected(mode, p, seqs, k, cache)
                assert _got(engine, h, mode, p, k, False) == raw, (mode, seam, off, v)
                assert [g[:4] for g in _got(engine, h, mode, p, k, True)] == red, (mode, seam, off, v)
                h.release()
                rows += len(raw)
                if v == p and off in (-m, 0):
                    flush += 1
                    assert any(r[0] == (0 if off < 0 else 1) and r[3] == 0 for r in raw), "a copy flush against the seam is found"
                if v == p and -m < off < 0 and mode == EXACT:
                    assert not raw, "a copy across the seam belongs to neither sequence"
    assert rows > 100 and flush == 12


def test_degenerate_shapes(engine):
    rnd = random.Random(93)
    alpha = b"ACGT"
    m, k = 20, 2
    L = m // (k + 1)
    p = _rand(rnd, alpha, m)
    # all sequences empty
    for n_seqs in (1, 5, 1000):
        assert _check(engine, [b""] * n_seqs, p, k)[0] == 0
    # sequences shorter than the n-gram, the pattern, the window; the pattern itself; below the file stream's minimum chunk
    shorts = []
    for n in (L - 1, m - 1, m, m + k, m + 2 * k + 1):
        shorts.append(p[:n] if n <= m else p + _rand(rnd, alpha, n - m))
        shorts.append(_rand(rnd, alpha, n))
        shorts.append(p[1:n + 1] if n < m else _rand(rnd, alpha, n - m) + p)
    shorts += [p, p[:-1], p[1:], p[:5] + p[6:], p, b""]
    n, _ = _check(engine, shorts, p, k)
    assert n > 10
    # a pattern equal to a whole sequence, many times over
    n, _ = _check(engine, [p] * 50, p, k)
    assert n >= 150
    # one sequence only: the in-memory search of the same bytes
    one = bytearray(_rand(rnd, alpha, 2 * TILE + 123))
    for at in (0, 700, TILE - 9, 2 * TILE + 123 - m):
        one[at:at + m] = p
    one = bytes(one)
    blob, offs = _pack([one])
    hb = engine.upload_batch(blob, offs)
    hs = engine.upload(one)
    rows, seq_of = engine.batch_search(hb, LEV, p, k)
    assert [tuple(int(x) for x in r) for r in rows.tolist()] == engine.lev_ngrams(hs, p, k) and len(rows) >= 4
    assert not seq_of.any()
    hb.release()
    hs.release()


def test_one_long_sequence_between_many_short(engine):
    rnd = random.Random(94)
    alpha = b"ACGT"
    m, k = 20, 2
    p = _rand(rnd, alpha, m)
    short = lambda: _rand(rnd, alpha, rnd.randint(0, 40))
    seqs = [short() for _ in range(10000)]
    long_one = bytearray(_rand(rnd, alpha, 3 * TILE))
    for at in (0, TILE - 10, 2 * TILE - 5, 3 * TILE - m):
        long_one[at:at + m] = p
    seqs.append(bytes(long_one))
    seqs += [short() for _ in range(10000)]
    for j in (0, 17, 9999, 10001, 20000):
        seqs[j] = p + seqs[j][:10]
    n, _ = _check(engine, seqs, p, k)
    assert n >= 3 * 9


def test_one_pass(engine):
    """The filter launches of a batch search = those of the unsegmented search of the pattern over the same packed bytes."""
    rnd = random.Random(95)
    alpha = b"ACGT"
    seqs = [_rand(rnd, alpha, rnd.randint(100, 200)) for _ in range(1000)]
    blob, offs = _pack(seqs)
    hb = engine.upload_batch(blob, offs)
    hs = engine.upload(blob)
    for m, k in ((20, 2), (54, 8), (100, 4)):                    # one launch, and patterns of more blocks than one launch tests
        p = _rand(rnd, alpha, m)
        engine.lev_ngrams(hs, p, k)
        single = engine.stats()
        engine.batch_search(hb, LEV, p, k)
        st = engine.stats()
        assert st["filter_launches"] == single["filter_launches"] >= 1
        assert st["verify_form"] == single["verify_form"]
        assert st["bytes_scanned"] == single["bytes_scanned"]
    hb.release()
    hs.release()


def _reads(rnd, kind):
    alpha = "ACGT"
    p = "".join(rnd.choice(alpha) for _ in range(24))
    seqs = []
    for _ in range(120):
        n = rnd.choice([0, 5, 23, 24, 30, 150, 151, 400])
        s = [rnd.choice(alpha) for _ in range(n)]
        if n >= 30 and rnd.random() < 0.5:
            v = gpu_cases.edited(rnd, p.encode(), rnd.randint(0, 2), alpha.encode()).decode()
            at = rnd.randint(0, n - len(v)) if n > len(v) else 0
            s[at:at + len(v)] = v
        seqs.append("".join(s))
    if kind == "str":
        return p, seqs
    if kind == "bytes":
        return p.encode(), [s.encode() for s in seqs]
    return bytearray(p.encode()), [bytearray(s.encode()) if i % 2 else memoryview(s.encode()) for i, s in enumerate(seqs)]


LIMITS = [dict(max_l_dist=2), dict(max_l_dist=0), dict(max_substitutions=2, max_insertions=0, max_deletions=0),
          dict(max_l_dist=7),                                                      # 24 // 8 = 3: still the n-gram route, dense candidates
          dict(max_substitutions=1, max_insertions=1, max_deletions=1, max_l_dist=2)]  # generic limits: the loop


@pytest.mark.parametrize("kind", ["bytes", "bytearray", "str"])
def test_public_api(kind):
    import fuzzysearch_amd as fa
    rnd = random.Random(96)
    p, seqs = _reads(rnd, kind)
    found = 0
    for limits in LIMITS:
        got = fa.find_near_matches_batch(p, seqs, **limits)
        want = [fa.find_near_matches(p, s, **limits) for s in seqs]
        assert got == want, (kind, limits)
        assert [[x.matched for x in g] for g in got] == [[x.matched for x in w] for w in want], (kind, limits)
        found += sum(len(g) for g in got)
    assert found > 100
    short = p[:5]                                                    # 5 // 3 = 1: the linear-programming route
    assert fa.find_near_matches_batch(short, seqs[:40], max_l_dist=2) == [fa.find_near_matches(short, s, max_l_dist=2) for s in seqs[:40]]


def test_public_api_resident_batch_and_loop_routes():
    import fuzzysearch_amd as fa
    rnd = random.Random(97)
    p, seqs = _reads(rnd, "bytes")
    held = fa.resident_batch(seqs)
    assert len(held) == len(seqs) and held[3] == seqs[3]
    for pat, limits in ((p, dict(max_l_dist=2)), (p[2:], dict(max_l_dist=1)), (p[:12], dict(max_substitutions=1, max_insertions=0, max_deletions=0))):
        got = fa.find_near_matches_batch(pat, held, **limits)
        want = [fa.find_near_matches(pat, s, **limits) for s in seqs]
        assert got == want and [[x.matched for x in g] for g in got] == [[x.matched for x in w] for w in want]
    # the loop inside the same handle: generic limits
    g = dict(max_substitutions=1, max_insertions=1, max_deletions=0, max_l_dist=2)
    assert fa.find_near_matches_batch(p, held, **g) == [fa.find_near_matches(p, s, **g) for s in seqs]
    held.release()
    # lists of ints, mixed kinds
    ints = [[rnd.randint(0, 3) for _ in range(rnd.randint(0, 60))] for _ in range(30)]
    pi = ints[3][:12] if len(ints[3]) >= 12 else [0, 1, 2, 3] * 3
    assert fa.find_near_matches_batch(pi, ints, max_l_dist=1) == [fa.find_near_matches(pi, s, max_l_dist=1) for s in ints]
    held = fa.resident_batch(ints)
    assert fa.find_near_matches_batch(pi, held, max_l_dist=1) == [fa.find_near_matches(pi, s, max_l_dist=1) for s in ints]
    held.release()
    mixed = [seqs[0], bytearray(seqs[1]), seqs[2]]
    assert fa.find_near_matches_batch(p, mixed, max_l_dist=2) == [fa.find_near_matches(p, s, max_l_dist=2) for s in mixed]
    with pytest.raises(TypeError):
        fa.find_near_matches_batch(p, [seqs[0], seqs[1].decode()], max_l_dist=2)      # what the loop raises at the str
    # an empty subsequence and a refused budget raise what the loop raises
    long_p = b"ACGT" * 1100                                      # 4400 // 1101 = 3: the n-gram route, with a budget beyond the kernels'
    def outcome(fn):
        try:
            return ("value", fn())
        except Exception as exc:
            return (type(exc), str(exc))

    raised = 0
    for bad_p, limits in ((b"", dict(max_l_dist=1)), (p, dict(max_l_dist=2000)), (p, dict()), (long_p, dict(max_l_dist=1100)),
                          (p, dict(max_l_dist=-1)), (p, dict(max_substitutions=30, max_insertions=0, max_deletions=0))):
        loop = outcome(lambda: [fa.find_near_matches(bad_p, s, **limits) for s in seqs])
        assert outcome(lambda: fa.find_near_matches_batch(bad_p, seqs, **limits)) == loop, (bad_p[:30], limits)
        raised += loop[0] != "value"
    assert raised >= 3
    assert fa.find_near_matches_batch(p, [], max_l_dist=2) == []


def test_handle_misuse(engine):
    rnd = random.Random(98)
    seqs = [_rand(rnd, b"ACGT", 200) for _ in range(20)]
    p = seqs[4][50:70]
    blob, offs = _pack(seqs)
    hb = engine.upload_batch(blob, offs)
    hs = engine.upload(blob)
    with pytest.raises(ValueError):
        engine.lev_ngrams(hb, p, 2)
    with pytest.raises(ValueError):
        engine.subs_ngrams(hb, p, 2)
    with pytest.raises(ValueError):
        engine.search_exact(hb, p)
    with pytest.raises(ValueError):
        engine.lev_ngrams_multi(hb, [p, p[1:]], 2)
    with pytest.raises(ValueError):
        engine.batch_search(hs, LEV, p, 2)
    with pytest.raises(ValueError):
        engine.batch_search(hb, 3, p, 2)                          # no batched generic search
    with pytest.raises(ValueError):
        engine.batch_search(hb, LEV, b"", 2)
    with pytest.raises(ValueError):
        engine.batch_search(hb, LEV, b"AC", 2)                    # n-gram length 0, as fz_lev_ngrams refuses it
    # ... and the engine is as usable as before
    assert engine.lev_ngrams(hs, p, 2) == oracle.lev_ngrams_raw(p, blob, 2)
    got = _got(engine, hb, LEV, p, 2, False)
    assert got == _expected(LEV, p, seqs, 2)[0] and any(g[0] == 4 and g[3] == 0 for g in got)
    hb.release()
    hs.release()
