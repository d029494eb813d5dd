"""The oracle — the expected side of every GPU assertion — pinned against the REFERENCE's compiled path where the GPU
is actually judged: 16 MiB of every BASELINE workload at its stated pattern shape (tests/workloads.py, the generators
of the 1 GiB parity tests and of bench.py), raw streams ordered-equal; wide budgets (m up to 400, k up to 40: the
regimes of tests/test_gpu_limits.py); and the consolidation of the large generic stream against the reference's
consolidate_overlapping_matches, tie-aware.  (tests/test_oracle_vs_reference.py covers thousands of tiny cases: n <= 60.)
The reference's answers were recorded with all four of its native extensions bound (tests/golden/gen_reference_results.py
-> tests/golden/reference_results.json.gz); the inputs are regenerated here and checked against the digest stored with them."""
import random

import oracle
from fuzzysearch_amd import _native
from oracle import ref_loader
from tests import golden_io, workloads

N = 16 << 20


def configs1_case():
    seq, pat, planted = workloads.cfg2(N, 64)
    return pat.tobytes(), seq.tobytes(), len(planted)


def configs2_case():
    seq, pat, planted = workloads.cfg3(N, 64)
    return pat.tobytes(), seq.tobytes(), len(planted)


def configs3_case():
    seq, pat, _planted = workloads.cfg4(N, 64)
    return pat.tobytes(), seq.tobytes()


def test_configs1_dna_levenshtein_m20_k2():
    p, t, n_planted = case = configs1_case()
    (exp, api), = golden_io.recorded("configs1_lev_m20_k2", [case])
    exp, api = golden_io.as_triples(exp), golden_io.as_triples(api)
    got = oracle.lev_ngrams_raw(p, t, 2)
    assert [r[:3] for r in got] == exp and len(exp) >= n_planted > 40
    # the CPU leg of `bench.py --full` (oracle/ref_glue: the reference's natives under a restated outer loop) is the same
    # stream — where those natives were built (oracle/_ref: build() next to the reference's sources)
    if ref_loader.have_ref_natives():
        from oracle import ref_glue
        assert ref_glue.lev_ngrams_raw(p, t, 2) == exp
    # ... and the public API's answer, tie-aware
    assert golden_io.equal_modulo_ties(oracle.consolidate(got), api, got)


def test_configs2_ascii_substitutions_m32_k3():
    p, t, n_planted = case = configs2_case()
    (exp, api), = golden_io.recorded("configs2_subs_m32_k3", [case])
    api = golden_io.as_triples(api)
    got = oracle.subs_ngrams_raw(p, t, 3)
    assert [r[0] for r in got] == exp and len(exp) >= n_planted > 40
    # the reference's own Match construction + group-list-order reduction (substitutions_only.py:258-282)
    best, _hull = oracle.group_best(got)
    assert [(s, e, d) for (s, e, d, _g) in best] == api
    mine = _native.group_best([tuple(r) for r in got])
    assert [tuple(r[:3]) for r in mine] == api


def test_configs3a_utf8_levenshtein_m64_k5():
    p, t = case = configs3_case()
    exp, = golden_io.recorded("configs3a_lev_m64_k5", [case])
    exp = golden_io.as_triples(exp)
    got = oracle.lev_ngrams_raw(p, t, 5)
    assert [r[:3] for r in got] == exp and len(exp) > 100
    assert {d for (_s, _e, d) in exp} >= {0, 1, 2, 3, 4, 5}             # every distance of the 0..5-edit plants occurs


def test_configs3b_utf8_generic_m64_limits_and_its_consolidation():
    p, t = case = configs3_case()
    (exp, ref_cons, api), = golden_io.recorded("configs3b_generic_m64_5225", [case])
    exp, ref_cons, api = golden_io.as_triples(exp), golden_io.as_triples(ref_cons), golden_io.as_triples(api)
    got = oracle.generic_ngrams_raw(p, t, 5, 2, 2, 5)
    assert [r[:3] for r in got] == exp and len(exp) > 3000                # ordered list, duplicates included
    # consolidation of the large stream: the reference's own function on its own Match objects, against the oracle's and
    # the product's host-side consolidation (fz_consolidate needs no device), tie-aware
    mine = oracle.consolidate(got)
    assert len(mine) == len(ref_cons) > 30
    assert golden_io.equal_modulo_ties(mine, ref_cons, got)
    prod = [tuple(r[:3]) for r in _native.consolidate([tuple(r) for r in got])]
    assert golden_io.equal_modulo_ties(prod, ref_cons, got) and prod == mine
    # ... and the reference's public API takes this route for these limits
    assert golden_io.equal_modulo_ties(mine, api, got)


def _plant(rnd, t, p, alpha, k):
    v = bytearray(p)
    for _ in range(rnd.randint(0, k)):
        q = rnd.randrange(len(v))
        op = rnd.random()
        if op < 0.4:
            v[q] = rnd.choice(alpha)
        elif op < 0.7 and len(v) > k + 1:
            del v[q]
        else:
            v.insert(q, rnd.choice(alpha))
    at = rnd.randint(0, max(0, len(t) - len(v)))
    t[at:at + len(v)] = v


def wide_budget_cases():
    """-> (it, p, t, k, ks, generic limits) — ks: the substitutions budget on every third case, else None; generic limits
    (max_substitutions, max_insertions, max_deletions, max_l_dist) as handed to LevenshteinSearchParams on every fourth."""
    rnd = random.Random(404)
    out = []
    for it in range(90):
        sigma = rnd.choice([2, 3, 4, 4, 20])
        alpha = bytes(rnd.sample(range(33, 127), sigma))
        m = rnd.randint(60, 400)
        k = rnd.randint(8, 40)
        if m // (k + 1) < 3:                                     # the n-gram regime of the reference's dispatcher (levenshtein.py:19-30)
            continue
        p = bytes(rnd.choice(alpha) for _ in range(m))
        t = bytearray(rnd.choice(alpha) for _ in range(rnd.randint(2000, 6000) if sigma >= 4 else rnd.randint(1200, 2500)))
        for _ in range(rnd.randint(1, 4)):
            _plant(rnd, t, p, alpha, k)
        t = bytes(t)
        ks = min(k, 12) if it % 3 == 0 else None
        limits = None
        if it % 4 == 0:
            kg = min(k, 6)
            limits = (rnd.randint(0, kg), rnd.randint(0, kg), rnd.randint(0, kg), kg)
        out.append((it, p, t, k, ks, limits))
    return out


def test_wide_budgets_long_patterns():
    """m in 60..400, k in 8..40 (Levenshtein n-grams: lane-per-cell and big verification regimes on the GPU), plus the
    generic and substitutions routes at such shapes."""
    cases = wide_budget_cases()
    exp = golden_io.recorded("wide_budgets", cases)
    n_lev = n_hits = 0
    for (it, p, t, k, ks, limits), (lev, subs, gen) in zip(cases, exp):
        lev = golden_io.as_triples(lev)
        assert [r[:3] for r in oracle.lev_ngrams_raw(p, t, k)] == lev, (it, len(p), k)
        n_lev += 1
        n_hits += bool(lev)
        if ks is not None:
            assert [r[0] for r in oracle.subs_ngrams_raw(p, t, ks)] == subs, (it, len(p), ks)
        if limits is not None:
            a, rows = gen
            if len(p) // (a[3] + 1) >= 1:
                assert [r[:3] for r in oracle.generic_ngrams_raw(p, t[:3000], *a)] == golden_io.as_triples(rows), (it, len(p), a)
    assert n_lev >= 50 and n_hits >= 40
