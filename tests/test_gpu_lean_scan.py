"""-m gpu: the lean and the full instance of the in-memory register-band / Hamming-count scan (fz_lean_scan_kernel /
fz_scan_kernel<..., 0>) against the oracle — ordered, bit-exact raw streams through the C-ABI, on the smallest inputs that
reach every path in which the two instances differ: the rare path's queue stores (one entry per firing lane, or one per
member of an equal-n-gram set), the register bands of the mid-scan and the pooled flush (k = 1, 2 in both; k = 3, 4 in the
full one only), the Hamming count, and the tile enumeration behind a queue overflow.

Texts are three tiles plus five bytes of seeded DNA with variants of the pattern planted at offset 0, across both tile seams,
inside a tile and at the very end.  Which instance a case runs is asserted through fz_debug_scan_instance."""
import numpy as np
import pytest

import oracle
from fuzzysearch_amd import _native
from tests import workloads
from tests.scan_instance_case import LEV, SUBS, REPEATED, reload_switches, scan_instance

pytestmark = pytest.mark.gpu

TILE = 16 << 10
N = 3 * TILE + 5                                         # 49 157 bytes
FORM_FUSED_BAND = _native.FORM_FUSED_BAND


def _variants(p, subs_only):
    """exact, one substitution, one deletion, one insertion (substitutions-only: two and three substitutions instead)."""
    p = bytes(p)
    other = lambda c: b"ACGT"[(b"ACGT".index(c) + 1) % 4] if c in b"ACGT" else ord("A")
    sub = lambda s, q: s[:q] + bytes([other(s[q])]) + s[q + 1:]
    m = len(p)
    if subs_only:
        return [p, sub(p, m // 2), sub(sub(p, 1), m - 2), sub(sub(sub(p, 0), m // 3), m - 1)]
    return [p, sub(p, m // 2), p[:m // 3] + p[m // 3 + 1:], p[:2 * m // 3] + bytes([other(p[2 * m // 3])]) + p[2 * m // 3:]]


def _text(p, seed, subs_only=False, run=None):
    """Seeded DNA of N bytes with the variants at offset 0, across the seam of tiles 0 | 1 and 1 | 2, inside tile 1 and
    ending with the text; `run` = (start, length, character): a run of one character (planted before the variants)."""
    seq = workloads.dna(N, seed).copy()
    if run:
        seq[run[0]:run[0] + run[1]] = run[2]
    v = _variants(p, subs_only)
    m = len(p)
    plants = [(0, v[1]), (TILE - m // 2, v[2]), (2 * TILE - 3, v[3]), (TILE + 5000, v[0]), (N - len(v[2]), v[2]), (2 * TILE + 7001, v[1])]
    for at, var in plants:
        seq[at:at + len(var)] = np.frombuffer(var, dtype=np.uint8)
    return seq


def _check(engine, kind, p, k, seq, lean, min_rows=4):
    p = bytes(p)
    mode = SUBS if kind == "subs" else LEV
    nl, which, form = scan_instance(mode, p, k, len(seq))
    assert form == FORM_FUSED_BAND and which == [lean] * nl, "the case does not run the instance it is meant for"
    t = seq.tobytes()
    want = oracle.subs_ngrams_raw(p, t, k) if kind == "subs" else oracle.lev_ngrams_raw(p, t, k)
    assert len(want) >= min_rows
    h = engine.upload(seq)
    try:
        got = engine.subs_ngrams(h, p, k) if kind == "subs" else engine.lev_ngrams(h, p, k)
        assert engine.stats()["verify_form"] == FORM_FUSED_BAND
    finally:
        h.release()
    assert got == want
    return want


@pytest.fixture
def no_bits(monkeypatch):
    monkeypatch.setenv("FZ_NO_BITS", "1")
    reload_switches()
    yield
    monkeypatch.delenv("FZ_NO_BITS")
    reload_switches()


@pytest.mark.parametrize("k", [1, 2])
def test_lean_levenshtein_distinct_blocks(engine, k):
    p = workloads.dna(20, 1).tobytes()
    _check(engine, "lev", p, k, _text(p, 100 + k), lean=True)


def test_full_equal_ngrams_one_candidate_per_set_member(engine):
    """Three equal 6-grams: every firing offset queues one entry per block of the set; the stream carries the same match
    once per block that finds it."""
    want = _check(engine, "lev", REPEATED, 2, _text(REPEATED, 103), lean=False)
    assert len({blk for (_s, _e, _d, blk) in want}) == 3


def test_lean_substitutions_only(engine):
    p = workloads.dna(32, 5).tobytes()
    _check(engine, "subs", p, 3, _text(p, 104, subs_only=True), lean=True)


@pytest.mark.parametrize("m,k", [(24, 3), (40, 4)])
def test_full_bands_three_and_four(engine, no_bits, m, k):
    p = workloads.dna(m, 7 + k).tobytes()
    _check(engine, "lev", p, k, _text(p, 105 + k), lean=False)


@pytest.mark.parametrize("lean", [True, False])
def test_queue_overflow_enumerates_the_tile(engine, lean):
    """A 20 000-byte run of A against a pattern that contains AAAAAA as an n-gram: every offset of the run fires, the
    queue overflows and the tiles of the run are enumerated — through the lean instance (distinct blocks) and through the
    full one (the 6-gram twice: an equal-n-gram set on top)."""
    p = b"AAAAAA" + b"CGTACG" + (b"TTGCAT" if lean else b"AAAAAA") + b"GC"
    _check(engine, "lev", p, 2, _text(p, 110, run=(TILE // 2 + 3, 20000, ord("A"))), lean=lean)


def test_lean_two_searches_in_flight(engine):
    p = workloads.dna(20, 1).tobytes()
    texts = [_text(p, 120 + i) for i in range(2)]
    texts[1][1000:1020] = np.frombuffer(p, dtype=np.uint8)       # one more match: the two streams differ
    assert scan_instance(LEV, p, 2, N) == (1, [True], FORM_FUSED_BAND)
    want = [oracle.lev_ngrams_raw(p, t.tobytes(), 2) for t in texts]
    assert all(len(w) >= 4 for w in want) and want[0] != want[1]
    hs = [engine.upload(t) for t in texts]
    try:
        engine.lev_ngrams_begin(hs[0], p, 2)
        for i in range(6):
            if i + 1 < 6:
                engine.lev_ngrams_begin(hs[(i + 1) % 2], p, 2)
            assert engine.lev_ngrams_end() == want[i % 2], i
    finally:
        for h in hs:
            h.release()
