"""Substitutions-only multi-pattern search, the parts that need no GPU: a whole group run on the host by the functions the
kernels run (fz_device.h compiled with g++: tests/mp_subs_emul.cpp) against the oracle's stream of every pattern, the planner
in substitutions mode (fz_debug_multi_plan_mode) and the argument handling of find_near_matches_multi with the substitutions
keywords."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import oracle
from fuzzysearch_amd import _native
from tests.test_multi_host import MAX_BLOCKS, MAX_M, MAX_PATS, _check_plan, _in_domain, _random_list

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(tempfile.gettempdir(), "fz_mp_subs_emul_%d.so" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                           os.path.join(HERE, "mp_subs_emul.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.mp_subs_emul_group.restype = ctypes.c_longlong
    L.mp_subs_emul_group.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_longlong]
    yield L
    os.remove(out)


def _group_rows(L_, pats, k, L, text):
    """-> per pattern, the rows (start, end, dist, block) the host model of the group produces, ordered by (block, index)."""
    blob, offs = _native.pack_patterns(pats)
    cap = 1 << 18
    out = (ctypes.c_int64 * (5 * cap))()
    c = L_.mp_subs_emul_group(blob, offs, len(pats), k, L, text, len(text), out, cap)
    assert 0 <= c <= cap, c
    per = [[] for _ in pats]
    for i in range(c):
        per[out[5 * i]].append((out[5 * i + 2], out[5 * i + 3], out[5 * i + 4], out[5 * i + 1]))
    return per


def _mutate(rnd, p, alpha, nsub):
    q = bytearray(p)
    for at in rnd.sample(range(len(q)), min(nsub, len(q))):
        q[at] = rnd.choice([c for c in alpha if c != q[at]] or [q[at] ^ 1])
    return bytes(q)


def _group(rnd, sigma, L, k):
    alpha = bytes(rnd.sample(range(1, 256), sigma)) if rnd.random() < 0.8 else bytes(rnd.sample(range(0, 256), sigma))
    npat = rnd.randint(1, 24)
    pats, blocks = [], 0
    while len(pats) < npat:
        m = rnd.randint(L * (k + 1), min(MAX_M, L * (k + 1) + k))
        if blocks + m // L > MAX_BLOCKS:
            break
        kind = rnd.random()
        if kind < 0.15 and pats:
            p = rnd.choice(pats)                                          # a duplicate pattern
        elif kind < 0.3 and pats:
            q = rnd.choice(pats)                                          # a shift of another pattern
            p = (q[rnd.randint(1, L):] + bytes(rnd.choice(alpha) for _ in range(m)))[:m]
        elif kind < 0.4:
            p = bytes([rnd.choice(alpha)]) * m                            # one symbol repeated
        else:
            p = bytes(rnd.choice(alpha) for _ in range(m))
        pats.append(p)
        blocks += len(p) // L
    return alpha, pats


def _text(rnd, alpha, pats, k, L, n):
    text = bytearray(rnd.choice(alpha) for _ in range(n))
    for _ in range(rnd.randint(0, 30) if n else 0):
        p = rnd.choice(pats)
        piece = _mutate(rnd, p, alpha, rnd.randint(0, k + 1))             # a copy with 0 .. k + 1 substitutions
        if rnd.random() < 0.15:
            piece = bytes([rnd.choice(alpha)]) * rnd.randint(L, 3 * L)    # a run of one symbol
        if len(piece) <= n:
            at = rnd.choice([0, n - len(piece), rnd.randint(0, n - len(piece))])
            text[at:at + len(piece)] = piece
    return bytes(text)


def test_group_model_equals_the_oracle(emul):
    rnd = random.Random(31)
    rows = groups = 0
    for it in range(100):
        k = rnd.choice([1, 2, 3, 4, 8])
        L = rnd.choice([4, 5, 6, 7, 8, 9, 10, 11, 12, 13]) if k < 8 else rnd.choice([4, 5, 8, 13])
        sigma = rnd.choice([2, 2, 4, 4, 20, 200])
        alpha, pats = _group(rnd, sigma, L, k)
        n = rnd.choice([0, 3, L, 100, 5000, 5000, 20000]) if sigma > 2 else rnd.choice([0, 3, L, 100, 2000])
        text = _text(rnd, alpha, pats, k, L, n)
        got = _group_rows(emul, pats, k, L, text)
        for p, g in zip(pats, got):
            want = oracle.subs_ngrams_raw(p, text, k)
            assert g == want, (it, k, L, len(p), n, g[:3], want[:3])
            rows += len(want)
        groups += 1
    print("group model: %d groups, %d rows" % (groups, rows))
    assert rows > 1000          # (some 60 groups with text to plant in, 15 copies each on average, most within the budget: a row at least each)


def test_every_window_alignment_and_pattern_tail(emul):
    """The dword path can go wrong where the window start is not a multiple of 4 and where the pattern's last dword is
    partial: one pattern of every length m mod 4 (two of each in the group, so that the longest differs from the lane's),
    copies with 0 .. k + 1 substitutions at every start mod 4, a substitution in the first and in the last character included,
    the window flush with both ends of the text."""
    rnd = random.Random(32)
    alpha = b"ACGT"
    checked, tails = 0, set()
    for k, L in ((1, 4), (2, 5), (3, 6), (2, 9)):
        pats = [bytes(rnd.choice(alpha) for _ in range(L * (k + 1) + extra)) for extra in range(k + 1) for _ in range(2)]
        tails |= set(len(p) % 4 for p in pats)
        for align in range(4):
            for nsub in range(k + 2):
                parts, starts = [bytes(rnd.choice(alpha) for _ in range(align))], []
                for p in pats:
                    q = bytearray(p)
                    where = ([0, len(p) - 1] + rnd.sample(range(1, len(p) - 1), k))[:nsub] if nsub != 1 else [rnd.choice([0, len(p) - 1])]
                    for at in where:                                      # the first and the last character among them
                        q[at] = rnd.choice([c for c in alpha if c != p[at]])
                    starts.append(sum(len(x) for x in parts))
                    parts.append(bytes(q))
                    parts.append(bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 3))))
                parts[-1] = b""                                           # the last window ends with the text
                text = b"".join(parts)
                got = _group_rows(emul, pats, k, L, text)
                for p, g, st in zip(pats, got, starts):
                    want = oracle.subs_ngrams_raw(p, text, k)
                    assert g == want, (k, L, align, nsub, len(p))
                    assert (nsub <= k) == any(r[0] == st for r in want), (k, L, align, nsub)
                    assert len(set(st % 4 for st in starts)) > 1 or len(pats) < 3
                    checked += 1
    assert checked > 100 and tails == {0, 1, 2, 3}


def test_block_that_does_not_match_gives_no_row(emul):
    """A window within the budget whose substitutions all lie in block 0: rows for blocks 1 and 2 only — and a text whose
    n-gram HASH equals block 0's (the first 8 bytes agree, the 9th differs: the filter reports it) gives none for block 0."""
    p = b"ACGTACGTTGGCATGCAATTCCGGATCGATC"                                # m = 31, k = 2: L = 10, blocks at 0, 10, 20
    other = b"TTGACCAGTCATGACCATGATTTACAGGACA"
    hit = bytearray(p)
    hit[8] = ord("A") if p[8] != ord("A") else ord("C")                    # byte 9 of block 0: behind the hashed 8
    text = b"GG" + bytes(hit) + b"T"
    got = _group_rows(emul, [p, other], 2, 10, text)
    assert got[0] == oracle.subs_ngrams_raw(p, text, 2) == [(2, 33, 1, 1), (2, 33, 1, 2)]
    assert got[1] == []


def test_plan_subs_partitions_random_lists():
    rnd = random.Random(33)
    for _ in range(150):
        pats, k = _random_list(rnd)
        group_of, ng = _native.multi_plan(pats, k, mode=_native.MODE_SUBS)
        assert len(group_of) == len(pats)
        _check_plan(pats, k, group_of, ng)
        for i, p in enumerate(pats):
            if not _in_domain(len(p), k):
                assert group_of[i] is None


def test_plan_subs_is_a_function_of_the_arguments():
    rnd = random.Random(34)
    lists = [_random_list(rnd) for _ in range(30)]
    first = [_native.multi_plan(p, k, mode=_native.MODE_SUBS) for p, k in lists]
    order = list(range(len(lists)))
    for _ in range(3):
        rnd.shuffle(order)
        for j in order:
            assert _native.multi_plan(*lists[j], mode=_native.MODE_SUBS) == first[j]
            assert _native.multi_plan(*lists[j], _native.MODE_LEV) == _native.multi_plan(*lists[j])


def test_plan_without_a_mode_is_the_levenshtein_plan():
    """The lists of test_multi_host.test_plan_full_groups, with the answers it holds them to."""
    rnd = random.Random(13)
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(24)) for _ in range(64)]
    assert _native.multi_plan(pats, 3) == ([0] * 64, 1)
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(65)]
    assert _native.multi_plan(pats, 2) == ([0] * 64 + [None], 1)
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(300)]
    assert _native.multi_plan(pats, 2) == ([i // 64 for i in range(300)], 5)
    dna = lambda m, c: [bytes(rnd.choice(b"ACGT") for _ in range(m)) for _ in range(c)]
    for m, c, k in ((32, 2, 2), (12, 64, 2), (20, 4, 2), (20, 16, 2), (32, 4, 2)):
        ps = dna(m, c)
        assert _native.multi_plan(ps, k) == _native.multi_plan(ps, k, _native.MODE_LEV)
    assert _native.multi_plan(dna(20, 4), 2) == ([None] * 4, 0)
    assert _native.multi_plan(dna(20, 16), 2) == ([0] * 16, 1)
    assert _native.multi_plan(dna(32, 4), 2) == ([0] * 4, 1)
    with pytest.raises(ValueError):
        _native.multi_plan([b"ACGT" * 5, b"ACGT" * 5], 2, mode=3)


def test_plan_subs_domain_and_cost_rule():
    rnd = random.Random(35)
    dna = lambda m, c: [bytes(rnd.choice(b"ACGT") for _ in range(m)) for _ in range(c)]
    S = _native.MODE_SUBS
    # the domain is the Levenshtein one
    assert _native.multi_plan([b"A" * 11, b"C" * 11], 2, S) == ([None, None], 0)          # L = 3
    assert _native.multi_plan([b"A" * 20, b"C" * 20], 0, S) == ([None, None], 0)
    assert _native.multi_plan([b"A" * 129, b"C" * 129], 2, S) == ([None, None], 0)
    assert _native.multi_plan([b"A" * 90, b"C" * 90], 9, S) == ([None, None], 0)
    assert _native.multi_plan([], 2, S) == ([], 0)
    assert _native.multi_plan(dna(20, 1), 2, S) == ([None], 0)
    # sparse candidates, enough patterns: one pass; 64 + 64 + ... by the pattern limit
    assert _native.multi_plan(dna(32, 64), 2, S) == ([0] * 64, 1)
    assert _native.multi_plan(dna(32, 16), 2, S) == ([0] * 16, 1)
    group_of, ng = _native.multi_plan(dna(32, 150), 2, S)
    assert ng == 3 and group_of == [i // 64 for i in range(150)]
    # two patterns cost less as a loop than the pass's fixed part; the measured cells of DESIGN.md section 6 go where they
    # were faster: 4 x (m = 20 / 23, k = 3) to the loop, 16 of them and 4 x (m = 32, k = 2) to a pass
    assert _native.multi_plan(dna(32, 2), 2, S) == ([None] * 2, 0)
    assert _native.multi_plan(dna(20, 4), 3, S) == ([None] * 4, 0)
    assert _native.multi_plan(dna(23, 4), 3, S) == ([None] * 4, 0)
    assert _native.multi_plan(dna(20, 16), 3, S) == ([0] * 16, 1)
    assert _native.multi_plan(dna(23, 64), 3, S) == ([0] * 64, 1)
    assert _native.multi_plan(dna(32, 4), 2, S) == ([0] * 4, 1)
    with pytest.raises(ValueError):
        _native.multi_plan([b"ACGT", b""], 1, S)


def test_find_near_matches_multi_substitutions_arguments():
    import fuzzysearch_amd as fa
    kw = {"max_substitutions": 2, "max_insertions": 0, "max_deletions": 0}
    assert fa.find_near_matches_multi([], b"ACGT", **kw) == []
    assert fa.find_near_matches_multi(iter(()), "text", max_l_dist=1, **kw) == []
    for bad in ({"max_substitutions": -1, "max_insertions": 0, "max_deletions": 0},
                {"max_substitutions": "2", "max_insertions": 0, "max_deletions": 0}):
        with pytest.raises(TypeError) as single:
            fa.find_near_matches(b"ACGTACGTACGT", b"ACGTACGT", **bad)
        with pytest.raises(TypeError) as multi:
            fa.find_near_matches_multi([b"ACGTACGTACGT"], b"ACGTACGT", **bad)
        assert str(multi.value) == str(single.value)
    for kw2 in ({"max_insertions": 0, "max_deletions": 0}, {"max_substitutions": 1, "max_deletions": 0}):
        with pytest.raises(ValueError) as single:
            fa.find_near_matches(b"ACGTACGTACGT", b"ACGTACGT", **kw2)
        with pytest.raises(ValueError) as multi:
            fa.find_near_matches_multi([b"ACGTACGTACGT"], b"ACGTACGT", **kw2)
        assert str(multi.value) == str(single.value)
    assert {"subs_ngrams_multi", "subs_ngrams_multi_best"} <= set(dir(_native.Engine))
    assert MAX_PATS == 64
