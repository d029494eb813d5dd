"""-m gpu: symbol classes on the multi-pattern pass (fz_mp_verify_cls_kernel / fz_mp_batch_verify_cls_kernel behind
fz_subs_ngrams_multi_cls, fz_batch_search_multi_cls, fz_batch_assign_cls and the ``classes`` keyword of the three public
calls) against a numpy brute-force model of the class distance (tests/classes_model.py): W = every window within k, the raw
stream = W per class-exact n-gram block, the public value = that stream through the host function fz_group_best."""
import random

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, classes
from tests import classes_model as model

pytestmark = pytest.mark.gpu

TILE = 16384
N_TEXT = 3 * TILE + 37                                     # several tiles and a ragged tail
IUPAC = fa.IUPAC_DNA
TABLES = classes.class_tables(IUPAC)
A = model.accept_table(IUPAC)
LETTERS = b"RYSWKMBDHVN"
ODD = b"Nacgt\n\x00\xff"                                   # sequence bytes that are no base symbol
SUBS = {"max_insertions": 0, "max_deletions": 0}
# a table none of whose keys occurs in a DNA pattern: the class kernels on the input of the plain ones
UNUSED = {ord("N"): b"ACGT", ord("R"): b"AG", ord("x"): b"Tt"}
# (m, k) with L = m // (k + 1) >= 4: L = 6, 5, 5, 10, 6, 14; k = 1 and k = 8 among them
ANCHOR_SHAPES = [(12, 1), (20, 3), (23, 3), (32, 2), (61, 8), (128, 8)]
CLASS_SHAPES = [(12, 2), (23, 3), (40, 3), (32, 2), (61, 8), (128, 8)]


def _dna(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def _rows(matches):
    return [(x.start, x.end, x.dist) for x in matches]


def _spell(rnd, p):
    return bytes(rnd.choice(IUPAC[c]) if c in IUPAC else c for c in p)


def _variant(rnd, p, nsub, odd=ODD):
    """A spelling of p with exactly nsub positions that do not class-match (where every base matches: a byte of `odd`)."""
    q = bytearray(_spell(rnd, p))
    for pos in rnd.sample(range(len(p)), nsub):
        q[pos] = rnd.choice([t for t in b"ACGT" if not A[p[pos], t]] or odd)
    return bytes(q)


def _degenerate(rnd, m, where):
    p = bytearray(_dna(rnd, m))
    for q in where:
        p[q] = rnd.choice(LETTERS)
    return bytes(p)


def _class_patterns(rnd, m, k):
    """Patterns with 1 to 4 IUPAC letters: at position 0, at the last position, inside a block's hashed bytes, at block
    offset >= 8 (L > 8), in the tail behind the last block (where there is one), mixtures, and one without any."""
    L = m // (k + 1)
    tail = list(range((m // L) * L, m))
    wheres = [[0], [m - 1], [L + 1, L + min(L, 8) - 1], [0, L + 2, m - 1], [2, L + 2, 2 * L + 1, m - 2], []]
    if L > 8:
        wheres.append([8, L + L - 1, L + 9])
    if tail:
        wheres.append(tail[-3:])
    return [_degenerate(rnd, m, w) for w in wheres]


def _planted_text(rnd, n, pats, k):
    """DNA with, per pattern, occurrences at distance 0, k and k + 1 (a near miss), a non-base byte right behind or in
    front of some of them, one flush with each end of the text."""
    text = bytearray(_dna(rnd, n))
    m = len(pats[0])
    slots = list(range(m + 5, n - 2 * m - 5, 2 * m + 7))
    rnd.shuffle(slots)
    at = iter(slots)
    for p in pats:
        for nsub in (0, k, k + 1):
            s = next(at)
            text[s:s + m] = _variant(rnd, p, nsub)
            if rnd.random() < 0.6:
                text[s + m] = rnd.choice(ODD)
            if rnd.random() < 0.3:
                text[s - 1] = rnd.choice(ODD)
    text[0:m] = _variant(rnd, pats[0], 0)
    text[n - m:n] = _variant(rnd, pats[-1], min(1, k))
    return bytes(text)


# ---- 4. anchor: the class kernels against the existing ones on identical input

@pytest.fixture(scope="module")
def anchor_reads():
    rnd = random.Random(50)
    return [_dna(rnd, rnd.choice([0, 3, 11, 40, 150, 200])) for _ in range(120)]


@pytest.mark.parametrize("m,k", ANCHOR_SHAPES)
def test_anchor_unused_classes_change_nothing(engine, anchor_reads, m, k):
    rnd = random.Random(51 + m)
    pats = [_dna(rnd, m) for _ in range(70)]                                       # two groups
    text = bytearray(_dna(rnd, N_TEXT))
    for i, p in enumerate(pats):
        v = bytearray(p)
        for q in rnd.sample(range(m), i % (k + 2)):
            v[q] = rnd.choice([c for c in b"ACGT" if c != v[q]])
        s = 13 + i * (N_TEXT // 71)
        text[s:s + m] = v
    text = bytes(text)
    kw = dict(max_substitutions=k, **SUBS)
    seq = fa.resident(text, engine=engine)
    plain = fa.find_near_matches_multi(pats, seq, **kw)
    cls = fa.find_near_matches_multi(pats, seq, classes=UNUSED, **kw)
    assert engine.stats()["verify_form"] == 5 and engine.stats()["filter_launches"] >= 2
    assert cls == plain
    assert sum(1 for x in plain if x) >= sum(1 for i in range(70) if i % (k + 2) <= k)   # (every copy planted within the budget)
    tables = classes.class_tables(UNUSED)
    assert engine.subs_ngrams_multi_classes(seq.handle, pats, k, tables) == engine.subs_ngrams_multi(seq.handle, pats, k)
    seq.release()
    reads = list(anchor_reads)
    for i in range(0, 70, 3):
        reads[i] = reads[i][:20] + pats[i] + reads[i][20:]
    held = fa.resident_batch(reads, engine=engine)
    plain = fa.find_near_matches_multi_batch(pats, held, **kw)
    assert fa.find_near_matches_multi_batch(pats, held, classes=UNUSED, **kw) == plain
    assert sum(len(y) for x in plain for y in x) >= 24
    best, best_cls = fa.find_best_matches_batch(pats, held, **kw), fa.find_best_matches_batch(pats, held, classes=UNUSED, **kw)
    for name in fa.BestMatches.__slots__:
        assert np.array_equal(getattr(best, name), getattr(best_cls, name)), name
    assert int((best.pattern >= 0).sum()) >= 24
    held.release()


# ---- 5. classes on one sequence

@pytest.mark.parametrize("m,k", CLASS_SHAPES)
def test_classes_on_one_sequence(engine, m, k):
    rnd = random.Random(60 + m)
    pats = _class_patterns(rnd, m, k)
    text = _planted_text(rnd, N_TEXT, pats, k)
    seq = fa.resident(text, engine=engine)
    raw = engine.subs_ngrams_multi_classes(seq.handle, pats, k, TABLES)
    st = engine.stats()
    assert st["verify_form"] == 5 and st["raw_matches"] == sum(len(r) for r in raw)
    public = fa.find_near_matches_multi(pats, seq, max_substitutions=k, classes=IUPAC, **SUBS)
    for i, p in enumerate(pats):
        W = model.windows_within(p, text, k, A)
        dists = set(d for _, d in W)
        assert 0 in dists and k in dists, ("planted at 0 and at k", i)
        assert len(set((r[0], r[3]) for r in raw[i])) == len(raw[i]), ("a (window, block) twice", i)
        assert sorted(set((r[0], r[2]) for r in raw[i])) == W, ("raw vs W", i, p)
        assert raw[i] == model.raw_rows(p, text, k, A), ("raw stream", i, p)
        assert _rows(public[i]) == model.best_of_groups(p, text, k, A), ("public", i, p)
        assert sorted(_rows(public[i])) == model.best_of_windows(p, text, k, A)
        assert all(x.matched == text[x.start:x.end] for x in public[i])
    # a list of one is searched by the pass, not refused and not looped
    one = fa.find_near_matches_multi([pats[0]], seq, max_substitutions=k, classes=IUPAC, **SUBS)
    assert engine.stats()["verify_form"] == 5 and engine.stats()["filter_launches"] >= 1
    assert _rows(one[0]) == model.best_of_groups(pats[0], text, k, A)
    seq.release()
    # bytes, not a handle: the same value
    short = text[:TILE + 5]
    got = fa.find_near_matches_multi(pats[:2], short, max_substitutions=k, classes=IUPAC, **SUBS)
    assert [_rows(g) for g in got] == [model.best_of_groups(p, short, k, A) for p in pats[:2]]


def test_sequence_in_two_shards(engine):
    """The sequence uploaded as two shards with an m-byte halo: together the rows of the whole."""
    rnd = random.Random(61)
    m, k = 23, 3
    pats = _class_patterns(rnd, m, k)
    n = 2 * TILE + 301
    text = bytearray(_planted_text(rnd, n, pats, k))
    cut = TILE + 150
    text[cut - 11:cut - 11 + m] = _variant(rnd, pats[3], 0)                         # across the cut: blocks on both sides
    text[cut - m - 30:cut - 30] = _variant(rnd, pats[0], 1)
    text[cut + 30:cut + 30 + m] = _variant(rnd, pats[1], k)
    text = bytes(text)
    whole = engine.upload(text)
    want = engine.subs_ngrams_multi_classes(whole, pats, k, TABLES)
    whole.release()
    a = engine.upload_shard(text[:cut + m], 0, 0, cut, n)
    b = engine.upload_shard(text[cut - m:], cut - m, cut, n, n)
    ra, rb = (engine.subs_ngrams_multi_classes(h, pats, k, TABLES) for h in (a, b))
    a.release()
    b.release()
    for i, p in enumerate(pats):
        got = sorted(ra[i] + rb[i], key=lambda r: (r[3], r[0]))
        assert got == want[i] == model.raw_rows(p, text, k, A), i
    assert any(s < cut < s + m for r in want for (s, _e, _d, _g) in r)


# ---- 6. / 7. batches

BATCH_K = 2
BATCH_PATS = [b"ACGTTGCAAGGCTTCANNN", b"NNNGATTACAGATTACAGG", b"TTGACCRYGGTCAAGTCCA", b"CCATGGCATNNCAGTAGCA", b"ACGTTGCAAGGCTTCAGGG"]   # m = 19: L = 6


@pytest.fixture(scope="module")
def reads_case():
    """Some 300 reads of 0 .. 200 bytes (DNA, N and lower case): empty reads, reads shorter than the patterns, planted
    occurrences inside reads and straddling the seam between two reads, reads that end 1, 2 or 3 bytes short of a full
    window whose missing bytes would all be class positions (the next read starts with bases that would complete it), a read
    two degenerate patterns fit equally well, and one that fits its pattern through a class letter only."""
    rnd = random.Random(70)
    k, pats = BATCH_K, BATCH_PATS
    m = len(pats[0])
    reads = []
    for i in range(290):
        n = rnd.choice([0, 0, 1, 5, m - 1, m, m + 1, 40, 77, 150, 200])
        r = bytearray(_dna(rnd, n))
        for _ in range(n // 40):
            r[rnd.randrange(n)] = rnd.choice(b"Nacgt")
        if n >= m and rnd.random() < 0.7:
            s = rnd.choice([0, n - m, rnd.randint(0, n - m)])
            r[s:s + m] = _variant(rnd, rnd.choice(pats), rnd.choice([0, 1, k, k + 1]), b"acgt")
        reads.append(bytes(r))
    for cutoff in range(1, m):                                                      # an occurrence across a seam
        v = _variant(rnd, pats[cutoff % len(pats)], 0, b"acgt")
        reads.append(_dna(rnd, 30) + v[:cutoff])
        reads.append(v[cutoff:] + _dna(rnd, 25))
    for short in (1, 2, 3):                                                         # ...NNN cut short; the next read would complete it
        reads.append(_dna(rnd, 9) + pats[0][:m - short])
        reads.append(b"ACG" + _dna(rnd, 30))
        reads.append(pats[1][short:m] + _dna(rnd, 8))                               # NNN... cut short at the front, bases in front
    reads.append(b"TT" + b"ACGTTGCAAGGCTTCAGGG" + b"AC")                             # patterns 0 and 4 at distance 0: tied
    reads.append(b"G" + b"TTGACCATGGTCAAGTCCA" + b"T")                               # pattern 2 through R = A and Y = T only
    reads.append(b"G" + b"TTGACCATGGTCAAGTCCC" + b"T")                               # ... and one true mismatch: 1 with classes, 3 without
    assert not any(b"\n" in r for r in reads)                                       # (they are FASTQ lines too)
    return reads


@pytest.fixture(scope="module")
def reads_model(reads_case):
    raw = [[model.raw_rows(p, r, BATCH_K, A) for r in reads_case] for p in BATCH_PATS]
    best = [[model.best_of_groups(p, r, BATCH_K, A) for r in reads_case] for p in BATCH_PATS]
    return raw, best, model.assignment(BATCH_PATS, reads_case, BATCH_K, A)


def _check_batch(engine, held, reads, reads_model):
    raw_want, best_want, _ = reads_model
    k, pats = BATCH_K, BATCH_PATS
    raw = engine.batch_search_multi_classes(held.handle, pats, k, TABLES, reduced=False)
    assert engine.stats()["verify_form"] == 5
    public = fa.find_near_matches_multi_batch(pats, held, max_substitutions=k, classes=IUPAC, **SUBS)
    n_rows = 0
    for i in range(len(pats)):
        rows, seq_of = raw[i]
        got = [[] for _ in reads]
        for r, j in zip(rows.tolist(), seq_of.tolist()):
            got[j].append(tuple(r))
        assert got == raw_want[i], ("raw", i)
        assert all(0 <= s and e <= len(reads[j]) for j, g in enumerate(got) for (s, e, _d, _b) in g), "a window across a seam"
        assert [_rows(x) for x in public[i]] == best_want[i], ("public", i)
        n_rows += len(rows)
    return n_rows


def test_batch(engine, reads_case, reads_model):
    held = fa.resident_batch(reads_case, engine=engine)
    assert len(reads_case) >= 300 and _check_batch(engine, held, reads_case, reads_model) > 200
    held.release()
    # not a handle: packed and uploaded by the call
    few = reads_case[:40]
    got = fa.find_near_matches_multi_batch(BATCH_PATS, few, max_substitutions=BATCH_K, classes=IUPAC, **SUBS)
    assert [[_rows(x) for x in per] for per in got] == [b[:40] for b in reads_model[1]]


def test_batch_from_fastq_records(engine, reads_case, reads_model):
    fastq = b"".join(b"@r%d\n%s\n+\n%s\n" % (j, r, b"I" * len(r)) for j, r in enumerate(reads_case))
    held = fa.resident_records(fastq, engine=engine)
    assert len(held) == len(reads_case)
    assert _check_batch(engine, held, reads_case, reads_model) > 200
    held.release()


def test_assignment(engine, reads_case, reads_model):
    want = reads_model[2]
    held = fa.resident_batch(reads_case, engine=engine)
    got = fa.find_best_matches_batch(BATCH_PATS, held, max_substitutions=BATCH_K, classes=IUPAC, **SUBS)
    held.release()
    rows = list(zip(got.pattern.tolist(), got.dist.tolist(), got.tied.tolist(), got.start.tolist(), got.end.tolist()))
    assert rows == want
    n = len(reads_case)
    assert want[n - 3] == (0, 0, True, 2, 21)                                       # two degenerate patterns, one distance
    assert want[n - 2] == (2, 0, False, 1, 20) and want[n - 1] == (2, 1, False, 1, 20)
    plain = fa.find_best_matches_batch(BATCH_PATS, reads_case[n - 2:], max_substitutions=BATCH_K, **SUBS)
    assert plain.dist.tolist() == [2, -1]                                           # without classes R and Y are mismatches
    assert sum(1 for w in want if w[0] >= 0) > 60 and sum(1 for w in want if w[2]) >= 1


# ---- 8. many candidates: the hit lists overflow and the launch is run again with what its counters ask for

def test_every_offset_is_a_candidate():
    """An engine of its own: result buffers only grow, and other tests count on the shared engine's first sizing."""
    n, k = 64 << 10, 2
    text = b"A" * n
    p = b"AAAANAAAAAAARAAAAAAAAAAM"                                                # m = 24: L = 8, three blocks
    m = len(p)
    eng = _native.Engine([0])
    try:
        seq = fa.resident(text, engine=eng)
        raw = eng.subs_ngrams_multi_classes(seq.handle, [p, b"C" + p[1:]], k, TABLES, as_array=True)
        st = eng.stats()
        assert st["filter_launches"] >= 2, "the first attempt's lists were too small: the group ran again"
        assert st["verify_form"] == 5
        nw = n - m + 1
        for i, dist, blocks in ((0, 0, [0, 1, 2]), (1, 1, [1, 2])):              # (the C breaks block 0 of the second pattern)
            got = raw[i]
            assert len(got) == nw * len(blocks)
            assert np.array_equal(got["start"], np.tile(np.arange(nw), len(blocks)))
            assert np.array_equal(got["block"], np.repeat(blocks, nw)) and np.all(got["dist"] == dist)
            assert np.array_equal(got["end"], got["start"] + m)
        public = fa.find_near_matches_multi([p], seq, max_substitutions=k, classes=IUPAC, **SUBS)
        assert _rows(public[0]) == [(0, m, 0)] == model.best_of_windows(p, text, k, A)
        seq.release()
    finally:
        eng.close()
