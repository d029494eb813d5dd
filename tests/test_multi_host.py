"""Multi-pattern search, the parts that need no GPU: the planner (fz_debug_multi_plan), the filter's table as the kernel
uses it (fz_device.h's fz_mp_* functions compiled with g++: tests/mp_table_emul.cpp) and the argument handling of
find_near_matches_multi."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from fuzzysearch_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_PATS, MAX_BLOCKS, MAX_M, MAX_K, MIN_L = 64, 256, 128, 8, 4      # fz_device.h: FZ_MP_*


def _in_domain(m, k):
    return 1 <= k <= MAX_K and m <= MAX_M and m // (k + 1) >= MIN_L


def _blocks(m, k):
    L = m // (k + 1)
    return m // L


def _random_list(rnd):
    k = rnd.choice([0, 1, 1, 2, 2, 3, 4, 8, 9])
    n = rnd.randint(0, 200)
    lengths = [rnd.choice([k + 1, 4 * (k + 1), 5 * (k + 1) + 1, 20, 32, 64, 128, 129, 200]) for _ in range(rnd.randint(1, 4))]
    pats = []
    for _ in range(n):
        m = max(k + 1, rnd.choice(lengths))
        pats.append(bytes(rnd.choice(b"ACGT") for _ in range(m)))
    return pats, k


def _check_plan(pats, k, group_of, ng):
    groups = {}
    for i, g in enumerate(group_of):
        m = len(pats[i])
        if g is None:
            continue
        assert 0 <= g < ng
        assert _in_domain(m, k), (m, k)
        groups.setdefault(g, []).append(i)
    assert sorted(groups) == list(range(ng))                      # every group number is used
    for g, members in groups.items():
        assert len(set(len(pats[i]) // (k + 1) for i in members)) == 1, "the patterns of a group share L"
        assert 2 <= len(members) <= MAX_PATS
        assert sum(_blocks(len(pats[i]), k) for i in members) <= MAX_BLOCKS
    # a pattern inside the domain rides alone only when its L has no partner left: at most one single per L and
    # closed group boundary
    first = [members[0] for _, members in sorted(groups.items())]
    assert first == sorted(first), "groups are numbered in the order of their first pattern"


def test_plan_partitions_random_lists():
    rnd = random.Random(11)
    for _ in range(150):
        pats, k = _random_list(rnd)
        group_of, ng = _native.multi_plan(pats, k)
        assert len(group_of) == len(pats)
        _check_plan(pats, k, group_of, ng)
        for i, p in enumerate(pats):
            if not _in_domain(len(p), k):
                assert group_of[i] is None


def test_plan_is_a_function_of_the_arguments():
    rnd = random.Random(12)
    lists = [_random_list(rnd) for _ in range(30)]
    first = [_native.multi_plan(p, k) for p, k in lists]
    order = list(range(len(lists)))
    for _ in range(3):
        rnd.shuffle(order)
        for j in order:
            assert _native.multi_plan(*lists[j]) == first[j]
            assert _native.multi_plan(*lists[j]) == first[j]


def test_plan_full_groups():
    rnd = random.Random(13)
    # 64 patterns, 4 blocks each = 256 blocks of one L: ONE group
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(24)) for _ in range(64)]
    assert _native.multi_plan(pats, 3) == ([0] * 64, 1)
    # 64 patterns of m = 20, k = 2 (3 blocks each): one group; the 65th starts another, which it has to itself: single route
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(65)]
    assert _native.multi_plan(pats[:64], 2) == ([0] * 64, 1)
    assert _native.multi_plan(pats, 2) == ([0] * 64 + [None], 1)
    # 300 of one length: 64 + 64 + 64 + 64 + 44
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20)) for _ in range(300)]
    group_of, ng = _native.multi_plan(pats, 2)
    assert ng == 5 and group_of == [i // 64 for i in range(300)]
    # the block limit closes a group before the pattern limit: m = 44, k = 8 -> L = 4, 11 blocks; 23 patterns = 253 blocks
    # (over 20 symbols: on four letters 253 blocks of 4 characters would make every offset a candidate, and the planner's cost
    #  rule gives such a list to the loop — below)
    pats = [bytes(rnd.choice(b"ACDEFGHIKLMNPQRSTVWY") for _ in range(44)) for _ in range(46)]
    group_of, ng = _native.multi_plan(pats, 8)
    assert ng == 2 and group_of == [0] * 23 + [1] * 23
    # two lengths interleaved: grouped by L, in input order
    pats = [bytes(rnd.choice(b"ACGT") for _ in range(20 if i % 2 == 0 else 32)) for i in range(16)]
    assert _native.multi_plan(pats, 2) == ([0, 1] * 8, 2)
    # one pattern, and everything outside the domain: the single route
    assert _native.multi_plan(pats[:1], 2) == ([None], 0)
    assert _native.multi_plan([b"A" * 11, b"C" * 11], 2) == ([None, None], 0)        # L = 3
    assert _native.multi_plan([b"A" * 20, b"C" * 20], 0) == ([None, None], 0)
    assert _native.multi_plan([b"A" * 129, b"C" * 129], 2) == ([None, None], 0)
    assert _native.multi_plan([b"A" * 90, b"C" * 90], 9) == ([None, None], 0)
    assert _native.multi_plan([], 2) == ([], 0)
    # the cost rule (fzhip.hip: mp_worth_a_pass): two or three patterns cost less as a loop than the pass's
    # fixed part, and so do lists whose expected candidates are dense — 64 DNA patterns of 12 characters at k = 2 make 192 of the
    # 256 possible 4-mers blocks; four of 20 characters at k = 2 measured a tie and go to the loop, sixteen ride one pass
    dna = lambda m, c: [bytes(rnd.choice(b"ACGT") for _ in range(m)) for _ in range(c)]
    assert _native.multi_plan(dna(32, 2), 2) == ([None] * 2, 0)
    assert _native.multi_plan(dna(12, 64), 2) == ([None] * 64, 0)
    assert _native.multi_plan(dna(20, 4), 2) == ([None] * 4, 0)
    assert _native.multi_plan(dna(20, 16), 2) == ([0] * 16, 1)
    assert _native.multi_plan(dna(32, 4), 2) == ([0] * 4, 1)
    with pytest.raises(ValueError):
        _native.multi_plan([b"ACGT", b""], 1)
    with pytest.raises(ValueError):
        _native.multi_plan([b"ACGTACGT", b"AC"], 2)


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(tempfile.gettempdir(), "fz_mp_emul_%d.so" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                           os.path.join(HERE, "mp_table_emul.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.mp_emul_scan.restype = ctypes.c_longlong
    L.mp_emul_scan.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64,
                               ctypes.c_void_p, ctypes.c_longlong]
    L.mp_emul_check_tables.restype = ctypes.c_int
    L.mp_emul_check_tables.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    yield L
    os.remove(out)


def _scan(L_, pats, L, text):
    blob, offs = _native.pack_patterns(pats)
    assert L_.mp_emul_check_tables(blob, offs, len(pats), L) == 0
    cap = 1 << 20
    out = (ctypes.c_uint64 * (3 * cap))()
    c = L_.mp_emul_scan(blob, offs, len(pats), L, text, len(text), out, cap)
    assert 0 <= c <= cap
    return set((out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(c)), c


def _true_hits(pats, L, text):
    want = set()
    for pid, p in enumerate(pats):
        for g in range(len(p) // L):
            ng = p[g * L:g * L + L]
            at = text.find(ng)
            while at >= 0:
                want.add((at, pid, g))
                at = text.find(ng, at + 1)
    return want


def _group(rnd, sigma, L, k):
    alpha = bytes(rnd.sample(range(1, 256), sigma)) if rnd.random() < 0.8 else bytes(rnd.sample(range(0, 256), sigma))
    npat = rnd.randint(1, MAX_PATS)
    pats, blocks = [], 0
    while len(pats) < npat:
        m = rnd.randint(L * (k + 1), min(MAX_M, L * (k + 1) + k))
        assert m // (k + 1) == L
        if blocks + m // L > MAX_BLOCKS:
            break
        kind = rnd.random()
        if kind < 0.15 and pats:
            p = rnd.choice(pats)                                          # a duplicate pattern
            m = len(p)
        elif kind < 0.3 and pats:
            q = rnd.choice(pats)                                          # a shift of another pattern: shared n-grams at other blocks
            sh = rnd.randint(1, L)
            p = (q[sh:] + bytes(rnd.choice(alpha) for _ in range(m)))[:m]
        elif kind < 0.4:
            p = bytes([rnd.choice(alpha)]) * m                            # one symbol repeated
        else:
            p = bytes(rnd.choice(alpha) for _ in range(m))
        pats.append(p)
        blocks += len(p) // L
    return alpha, pats


def test_table_model_never_misses_an_occurrence(emul):
    rnd = random.Random(14)
    false_pos = total = 0
    for it in range(120):
        k = rnd.choice([1, 2, 3, 4, 8])
        L = rnd.choice([4, 5, 6, 7, 8, 9, 10, 13]) if k < 8 else rnd.choice([4, 5, 8, 14])
        sigma = rnd.choice([2, 2, 3, 4, 4, 20, 200])
        alpha, pats = _group(rnd, sigma, L, k)
        n = rnd.choice([0, 3, L, 100, 5000, 20000])
        text = bytearray(rnd.choice(alpha) for _ in range(n))
        for _ in range(rnd.randint(0, 30)):                                # planted n-grams and whole patterns, runs of one symbol
            p = rnd.choice(pats)
            piece = p if rnd.random() < 0.5 else p[rnd.randrange(len(p)):][:L + 2]
            if rnd.random() < 0.2:
                piece = bytes([rnd.choice(alpha)]) * rnd.randint(L, 3 * L)
            if len(piece) <= n:
                at = rnd.randint(0, n - len(piece))
                text[at:at + len(piece)] = piece
        text = bytes(text)
        got, count = _scan(emul, pats, L, text)
        assert count == len(got), "an (offset, block) pair is reported once"
        want = _true_hits(pats, L, text)
        assert want <= got, (it, sorted(want - got)[:5])
        false_pos += len(got - want)
        total += len(got)
    print("table model: %d reported, %d of them false positives" % (total, false_pos))
    assert total > 10000


def test_find_near_matches_multi_arguments():
    import fuzzysearch_amd as fa
    assert "find_near_matches_multi" in fa.__all__
    assert fa.find_near_matches_multi([], b"ACGT", max_l_dist=1) == []
    assert fa.find_near_matches_multi([], b"ACGT") == []                  # the comprehension over nothing raises nothing
    assert fa.find_near_matches_multi(iter(()), "text", max_l_dist=2) == []
    for kw in ({}, {"max_substitutions": 1}, {"max_substitutions": 1, "max_insertions": 1}):
        with pytest.raises(ValueError) as single:
            fa.find_near_matches(b"ACGT", b"ACGTACGT", **kw)
        with pytest.raises(ValueError) as multi:
            fa.find_near_matches_multi([b"ACGT"], b"ACGTACGT", **kw)
        assert str(multi.value) == str(single.value)
    with pytest.raises(TypeError):
        fa.find_near_matches_multi([b"ACGT"], b"ACGTACGT", max_l_dist=-1)
    with pytest.raises(TypeError):
        fa.find_near_matches_multi([b"ACGT"], b"ACGTACGT", max_l_dist="1")
