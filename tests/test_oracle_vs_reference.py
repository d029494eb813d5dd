"""Random differentials: the oracle (oracle/fz_oracle.c) against the REFERENCE's own compiled
C/Cython path.  The reference's answers for these seeded inputs were recorded with all four of its
native extensions bound (tests/golden/gen_reference_results.py -> tests/golden/reference_results.json.gz);
the inputs are regenerated here from the same seeds and checked against the digest stored with them.
This is what pins the oracle beyond the reference's unit tests — in particular the last-arg-min tie
rule of `expand` (SURVEY.md trap 2), which the reference's own KATs do not distinguish."""
import random

import oracle
from tests import golden_io


def _case(rnd, max_n=60, max_m=14, max_k=3):
    sigma = rnd.choice([2, 2, 3, 4])
    alpha = bytes(rnd.sample(range(65, 91), sigma))
    n = rnd.randint(0, max_n)
    t = bytes(rnd.choice(alpha) for _ in range(n))
    k = rnd.randint(1, max_k)
    m = rnd.randint(k + 1, max_m)
    if rnd.random() < 0.5 and n >= m:
        st = rnd.randint(0, n - m)
        p = bytearray(t[st:st + m])
        for _ in range(rnd.randint(0, k)):
            q = rnd.randrange(len(p))
            op = rnd.random()
            if op < 0.4:
                p[q] = rnd.choice(alpha)
            elif op < 0.7 and len(p) > k + 1:
                del p[q]
            else:
                p.insert(q, rnd.choice(alpha))
        p = bytes(p)
    else:
        p = bytes(rnd.choice(alpha) for _ in range(m))
    return p, t, k


def lev_ngrams_cases():
    rnd = random.Random(1)
    out = []
    for _ in range(6000):
        p, t, k = _case(rnd)
        if len(p) // (k + 1) == 0:
            continue
        out.append((p, t, k))
    return out


def expand_cases():
    rnd = random.Random(2)
    out = []
    for _ in range(20000):
        alpha = bytes(rnd.sample(range(65, 91), rnd.choice([2, 3])))
        sub = bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 16)))
        win = bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 20)))
        k = rnd.randint(0, 5)
        out.append((sub, win, k))
    return out


def subs_ngrams_cases():
    rnd = random.Random(3)
    return [_case(rnd, max_k=4) for _ in range(6000)]


def generic_cases():
    """-> (p, t, (max_substitutions, max_insertions, max_deletions, max_l_dist)) as handed to LevenshteinSearchParams."""
    rnd = random.Random(4)
    out = []
    for _ in range(2500):
        alpha = bytes(rnd.sample(range(65, 91), rnd.choice([2, 3, 4])))
        t = bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 40)))
        p = bytes(rnd.choice(alpha) for _ in range(rnd.randint(1, 12)))
        ms, mi, md = rnd.randint(0, 3), rnd.randint(0, 3), rnd.randint(0, 3)
        out.append((p, t, (ms, mi, md, rnd.randint(0, ms + mi + md))))
    return out


def lp_fallback_cases():
    rnd = random.Random(9)
    out = []
    for _ in range(4000):
        alpha = bytes(rnd.sample(range(65, 91), rnd.choice([2, 2, 3, 4])))
        t = bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 50)))
        m = rnd.randint(1, 10)
        if rnd.random() < 0.5 and len(t) >= m:
            st = rnd.randint(0, len(t) - m)
            p = bytearray(t[st:st + m])
            if rnd.random() < 0.5:
                p[rnd.randrange(m)] = rnd.choice(alpha)
            p = bytes(p)
        else:
            p = bytes(rnd.choice(alpha) for _ in range(m))
        k = rnd.randint(0, 4)
        out.append((p, t, k))
    return out


def api_cases():
    rnd = random.Random(5)
    out = []
    for _ in range(3000):
        p, t, k = _case(rnd, max_m=16)
        if len(p) // (k + 1) < 3:
            continue
        out.append((p, t, k))
    return out


def test_lev_ngrams_raw():
    """find_near_matches_levenshtein_ngrams (ordered raw list) == the oracle's raw stream."""
    cases = lev_ngrams_cases()
    exp = golden_io.recorded("lev_ngrams_raw", cases)
    for (p, t, k), e in zip(cases, exp):
        assert golden_io.as_triples(e) == [r[:3] for r in oracle.lev_ngrams_raw(p, t, k)], (p, t, k)
    assert len(cases) > 4000


def test_expand_tie_rule():
    """levenshtein_ngram._expand == oracle.expand, (dist, length) including the tie rule."""
    cases = expand_cases()
    exp = golden_io.recorded("expand", cases)
    for (sub, win, k), e in zip(cases, exp):
        assert tuple(e) == oracle.expand(sub, win, k), (sub, win, k)


def test_subs_ngrams_raw():
    """substitutions_only._subs_only_fnm_ngram_byteslike (ordered start list) == the oracle's raw stream."""
    cases = subs_ngrams_cases()
    exp = golden_io.recorded("subs_ngrams_raw", cases)
    for (p, t, k), e in zip(cases, exp):
        assert e == [r[0] for r in oracle.subs_ngrams_raw(p, t, k)], (p, t, k)


def test_generic_raw():
    """find_near_matches_generic_linear_programming / _ngrams (ordered raw lists) == the oracle's; the limits as the
    reference's LevenshteinSearchParams normalises them (recorded as `unpacked`).  The lists are long here (every
    start / end pair within the limits on a text of at most 40 bytes): recorded as count + sha256 (golden_io.rows_digest)."""
    cases = generic_cases()
    exp = golden_io.recorded("generic_raw", cases)
    for (p, t, _limits), (a, lp, ng) in zip(cases, exp):
        assert golden_io.rows_digest(oracle.generic_lp_raw(p, t, *a)) == lp, (p, t, a)
        if len(p) // (a[3] + 1) >= 1:
            assert golden_io.rows_digest(oracle.generic_ngrams_raw(p, t, *a)) == ng, (p, t, a)
        else:
            assert ng is None


def test_linear_programming_fallbacks_raw():
    """(f)3: the oracle's restatement of the linear-programming fallbacks against the reference's own functions
    (levenshtein.py:52-148, substitutions_only.py:82-136) — ordered emission lists, short and long patterns,
    budgets up to and beyond the pattern length."""
    cases = lp_fallback_cases()
    exp = golden_io.recorded("lp_fallbacks_raw", cases)
    n_lev = n_subs = 0
    for (p, t, k), (lev, subs) in zip(cases, exp):
        assert [r[:3] for r in oracle.lev_lp_raw(p, t, k)] == golden_io.as_triples(lev), (p, t, k)
        n_lev += bool(lev)
        assert [r[:3] for r in oracle.subs_lp_raw(p, t, k)] == golden_io.as_triples(subs), (p, t, k)
        n_subs += bool(subs)
    assert n_lev > 1500 and n_subs > 1000


def test_api_consolidated_tie_aware():
    """find_near_matches(max_l_dist=k) == consolidate(raw) up to hash-seed dependent ties (recorded with
    PYTHONHASHSEED=0)."""
    cases = api_cases()
    exp = golden_io.recorded("api_consolidated", cases)
    strict = 0
    for (p, t, k), e in zip(cases, exp):
        e = golden_io.as_triples(e)
        raw = oracle.lev_ngrams_raw(p, t, k)
        got = oracle.consolidate(raw)
        assert golden_io.equal_modulo_ties(got, e, raw), (p, t, k, got, e)
        strict += got == e
    assert len(cases) > 500 and strict >= 0.8 * len(cases)
