"""Many patterns over many sequences, the parts that need no GPU: a whole ragged group run on the host by the functions
the kernels run (fz_device.h compiled with g++: tests/mp_batch_emul.cpp — the filter's over-reporting across seams, then
fz_segment_ragged, fz_mp_rag_accept and fz_verify_lev / fz_mp_verify_subs per hit) against the oracle run per (pattern,
sequence) in both modes; the same core as a program of its own; the pure routing of find_near_matches_multi_batch."""
import ctypes
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from fuzzysearch_amd import _native, batch, multi_batch
from fuzzysearch_amd.common import LevenshteinSearchParams
from tests import gpu_cases

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 16384
LEV, SUBS = 1, 2
MAX_M, MAX_BLOCKS = 128, 256


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(tempfile.gettempdir(), "fz_mp_batch_emul_%d.so" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "mp_batch_emul.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.mp_batch_emul_group.restype = ctypes.c_longlong
    L.mp_batch_emul_group.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_longlong]
    yield L
    os.remove(out)


def _group_rows(L_, mode, pats, k, L, seqs):
    """-> {(pattern, sequence): rows (start, end, dist, block) in local coordinates, ordered by (block, index)} of the host
    model of the group over the packed sequences."""
    blob, offs = _native.pack_patterns(pats)
    text = b"".join(seqs)
    so = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, seqs), dtype=np.uint64, count=len(seqs)), out=so[1:])
    cap = 1 << 18
    out = (ctypes.c_int64 * (6 * cap))()
    c = L_.mp_batch_emul_group(mode, blob, offs, len(pats), k, L, text or b"\0", so.ctypes.data, len(seqs), out, cap)
    assert 0 <= c <= cap, c
    per = {}
    for i in range(c):
        pid, j, g, st, en, d = out[6 * i:6 * i + 6]
        per.setdefault((pid, j), []).append((st, en, d, g))
    return per


def _want(mode, p, s, k, cache):
    key = (mode, p, s, k)
    if key not in cache:
        cache[key] = oracle.lev_ngrams_raw(p, s, k) if mode == LEV else oracle.subs_ngrams_raw(p, s, k)
    return cache[key]


def _compare(emul, mode, pats, k, L, seqs, cache, what):
    got = _group_rows(emul, mode, pats, k, L, seqs)
    rows = cells = 0
    for i, p in enumerate(pats):
        for j, s in enumerate(seqs):
            want = _want(mode, p, s, k, cache)
            assert got.get((i, j), []) == want, (what, mode, k, L, len(p), i, j, len(s))
            rows += len(want)
            cells += bool(want)
    return rows, cells


def _edit(rnd, mode, p, n, alpha):
    if mode == LEV:
        return gpu_cases.edited(rnd, p, n, alpha)
    q = bytearray(p)
    for at in rnd.sample(range(len(q)), min(n, len(q))):
        q[at] = rnd.choice(alpha)
    return bytes(q)


def _patterns(rnd, alpha, L, k, npat):
    pats, blocks = [], 0
    while len(pats) < npat:
        m = rnd.randint(L * (k + 1), min(MAX_M, L * (k + 1) + k))
        if blocks + m // L > MAX_BLOCKS:
            break
        if pats and rnd.random() < 0.15:
            q = rnd.choice(pats)                                          # a shift of another pattern
            p = (q[rnd.randint(1, L):] + bytes(rnd.choices(alpha, k=m)))[:m]
        else:
            p = bytes(rnd.choices(alpha, k=m))
        pats.append(p)
        blocks += m // L
    return pats


def _batch(rnd, mode, pats, k, L, alpha, n_seqs, n_big):
    """Sequences of 0 .. 400 bytes (and n_big longer than a tile) with edited copies of the patterns at their first and last
    bytes and elsewhere, and copies cut in two by a seam."""
    seqs = []
    bigs = set(rnd.sample(range(n_seqs), min(n_big, n_seqs)))
    for j in range(n_seqs):
        kind = rnd.random()
        if j in bigs:
            n = TILE + rnd.randint(1, 600)
        elif kind < 0.12:
            n = 0
        elif kind < 0.3:
            n = rnd.randint(1, L + 2)
        elif kind < 0.5:
            m = len(rnd.choice(pats))
            n = rnd.randint(max(0, m - k - 2), m + 2 * k + 2)
        else:
            n = rnd.randint(40, 400)
        t = bytearray(rnd.choices(alpha, k=n))
        for _ in range(2):
            v = _edit(rnd, mode, rnd.choice(pats), rnd.randint(0, k), alpha)
            if len(v) <= n and rnd.random() < 0.6:
                st = rnd.choice([0, 0, n - len(v), n - len(v), rnd.randint(0, n - len(v))])      # first and last bytes
                t[st:st + len(v)] = v
        seqs.append(t)
    for j in range(len(seqs) - 1):
        if rnd.random() < 0.3:
            p = rnd.choice(pats)
            cut = rnd.randint(1, len(p) - 1)
            a, b = seqs[j], seqs[j + 1]
            if len(a) >= cut and len(b) >= len(p) - cut:
                a[len(a) - cut:] = p[:cut]
                b[:len(p) - cut] = p[cut:]
    return [bytes(s) for s in seqs]


def test_ragged_group_model_equals_the_oracle(emul):
    rnd = random.Random(111)
    rows = cells = groups = big = 0
    for it in range(36):
        mode = LEV if it % 2 == 0 else SUBS
        sigma = [2, 4, 20, 200][(it // 2) % 4]
        # (two symbols: every offset is a candidate of most blocks — the oracle's cost; short patterns, small budgets)
        k = rnd.choice([1, 2]) if sigma == 2 else rnd.choice([1, 2, 3, 4, 8])
        L = rnd.choice([4, 5, 6]) if sigma == 2 else (rnd.choice([4, 5, 8, 13]) if k == 8 else rnd.choice([4, 5, 6, 7, 9, 12]))
        alpha = bytes(rnd.sample(range(1, 256), sigma))
        pats = _patterns(rnd, alpha, L, k, rnd.randint(2, 6))
        n_big = (1 if it % 4 == 0 else 2 if it % 12 == 6 else 0) if sigma > 2 else 0
        n_seqs = rnd.choice([1, 2, rnd.randint(3, 40), rnd.randint(100, 300)]) if sigma > 2 else rnd.randint(1, 40)
        seqs = _batch(rnd, mode, pats, k, L, alpha, n_seqs, n_big)
        big += n_big
        r, c = _compare(emul, mode, pats, k, L, seqs, {}, it)
        rows += r
        cells += c
        groups += 1
    print("ragged group model: %d groups, %d rows, %d (pattern, sequence) cells with rows, %d long sequences" % (groups, rows, cells, big))
    # (floors well below what the seed gives — 36 groups, a planted copy within the budget in most longer sequences)
    assert groups == 36 and rows > 3000 and cells > 300 and big >= 8


@pytest.mark.parametrize("mode", [LEV, SUBS])
def test_copies_cut_by_a_seam_at_every_split(emul, mode):
    """A copy with 0 .. k edits across the seam between two sequences, at every split 1 .. m - 1: found for neither; a copy
    ending at the seam and one starting at it: found, each in its own sequence."""
    rnd = random.Random(112 + mode)
    alpha = b"ACGT"
    bg = b"xyz"                                            # free of the patterns' symbols
    cache = {}
    for m, k in ((20, 2), (33, 2)):
        L = m // (k + 1)
        pats = [bytes(rnd.choices(alpha, k=m)) for _ in range(4)]
        seqs, across = [], []
        for cut in range(1, m):
            p = pats[cut % len(pats)]
            v = _edit(rnd, mode, p, cut % (k + 1), alpha)
            c = min(cut, len(v) - 1)
            a = bytes(rnd.choices(bg, k=30)) + v[:c]
            b = v[c:] + bytes(rnd.choices(bg, k=30))
            across.append((len(seqs), cut % len(pats)))
            seqs += [a, b]
        p = pats[0]
        flush = len(seqs)
        seqs += [bytes(rnd.choices(bg, k=25)) + p, p + bytes(rnd.choices(bg, k=25)), b"", p, p[:-1], p[1:]]
        got = _group_rows(emul, mode, pats, k, L, seqs)
        for i, q in enumerate(pats):
            for j, s in enumerate(seqs):
                assert got.get((i, j), []) == _want(mode, q, s, k, cache), (mode, m, i, j)
        for j, i in across:
            # (either half alone may hold a match of its own when the cut leaves m - k characters on one side: the oracle says)
            if not _want(mode, pats[i], seqs[j], k, cache) and not _want(mode, pats[i], seqs[j + 1], k, cache):
                assert (i, j) not in got and (i, j + 1) not in got
        assert any(r[:3] == (25, 25 + m, 0) for r in got[(0, flush)])
        assert any(r[:3] == (0, m, 0) for r in got[(0, flush + 1)])
        assert any(r[:3] == (0, m, 0) for r in got[(0, flush + 3)])
        assert sum(1 for j, i in across if (i, j) not in got and (i, j + 1) not in got) >= (m - 1) // 2


def test_seam_at_a_tile_boundary_and_degenerate_sequences(emul):
    rnd = random.Random(113)
    alpha = b"ACGT"
    m, k = 20, 2
    L = m // (k + 1)
    pats = [bytes(rnd.choices(alpha, k=m)) for _ in range(3)]
    p = pats[0]
    cache = {}
    rows = 0
    for mode in (LEV, SUBS):
        for seam in (TILE - (L - 1), TILE - 1, TILE, TILE + 1, TILE + (L - 1)):
            a = bytearray(rnd.choices(alpha, k=seam))
            b = bytearray(rnd.choices(alpha, k=300))
            a[seam - m:] = p                               # ends exactly at the seam
            b[:m] = pats[1]                                # starts exactly at it
            a[:m] = pats[2]                                # first sequence at offset 0
            b[300 - m:] = p                                # last sequence ends with the buffer
            shorts = [p[:n] for n in (0, 1, L - 1, L, m - k - 1, m - k, m)]
            seqs = [bytes(a)] + shorts + [bytes(b)]
            r, _ = _compare(emul, mode, pats, k, L, seqs, cache, seam)
            rows += r
        assert _compare(emul, mode, pats, k, L, [b""] * 7, cache, "empty") == (0, 0)
        r, _ = _compare(emul, mode, pats, k, L, [p + pats[1] + pats[2]], cache, "one")
        rows += r
    assert rows > 100


def test_stand_alone_model():
    """The same core as a program of its own (every sequence alone against the batch): the form that also runs under
    -fsanitize=address,undefined, which needs the compiler's runtime and is therefore not part of the suite."""
    exe = os.path.join(tempfile.gettempdir(), "fz_mp_batch_emul_%d" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DMP_BATCH_EMUL_MAIN",
                           os.path.join(HERE, "mp_batch_emul.cpp"), "-o", exe])
    try:
        out = subprocess.check_output([exe]).decode()
    finally:
        os.remove(exe)
    assert "rows agree" in out


# ---- routing ------------------------------------------------------------------------------------------------------

P9, P8 = b"ACGTACGTA", b"ACGTACGT"                          # 9 // 3 = 3: the n-gram route at k = 2; 8 // 3 = 2: linear programming
LIMITS = {
    "l2": dict(max_l_dist=2),
    "l0": dict(max_l_dist=0),
    "subs2": dict(max_substitutions=2, max_insertions=0, max_deletions=0),
    "generic": dict(max_substitutions=1, max_insertions=1, max_deletions=1, max_l_dist=2),
}


def _params(limits):
    return LevenshteinSearchParams(limits.get("max_substitutions"), limits.get("max_insertions"), limits.get("max_deletions"),
                                   limits.get("max_l_dist"))


def test_routes_every_kind_and_route():
    mixed = [P9, P8, P9.decode(), b"", bytearray(P9), [1, 2, 3, 4, 5, 6, 7, 8, 9], P9 + b"A", "ACGTACGTł"]
    R = multi_batch.multi_batch_routes
    # bytes sequences
    assert R(mixed, "bytes", _params(LIMITS["l2"])) == ([0, 4, 6], "lev", 2)
    assert R(mixed, "bytes", _params(LIMITS["subs2"])) == ([0, 4, 6], "subs", 2)
    assert R(mixed, "bytes", _params(LIMITS["l0"])) == ([], None, None)            # the exact route loops
    assert R(mixed, "bytes", _params(LIMITS["generic"])) == ([], None, None)
    # latin-1 str sequences: Levenshtein rides, substitutions-only loops (every window sorted by start, not the best of groups)
    assert R(mixed, "str", _params(LIMITS["l2"])) == ([2], "lev", 2)
    assert R(mixed, "str", _params(LIMITS["subs2"])) == ([], None, None)
    assert R(mixed, "str", _params(LIMITS["l0"])) == ([], None, None)
    assert R(mixed, "str", _params(LIMITS["generic"])) == ([], None, None)
    # other or mixed kinds, several devices: everything loops
    for name in LIMITS:
        assert R(mixed, None, _params(LIMITS[name])) == ([], None, None)
        assert R(mixed, "bytes", _params(LIMITS[name]), single_device=False) == ([], None, None)
    # per subsequence it is batch_route's decision
    for kind in ("bytes", "str", None):
        for name in LIMITS:
            riding, mode, k = R(mixed, kind, _params(LIMITS[name]))
            for i, p in enumerate(mixed):
                route = batch.batch_route(p, kind, _params(LIMITS[name]))
                assert (i in riding) == (route is not None and route[0] in ("lev", "subs"))
                if i in riding:
                    assert route == (mode, k)


class _NoRows(object):
    n, address = 0, 0

    def release(self):
        pass

    def to_array(self):
        return np.empty(0, dtype=_native._match_dtype())


class _StubHandle(object):
    def release(self):
        pass


class _StubEngine(object):
    devices = [0]

    def __init__(self, log):
        self.log = log

    def comm_info(self):
        return 0, -1, False

    def upload_batch(self, blob, offs):
        self.log.append(("upload", bytes(blob), [int(x) for x in offs]))
        return _StubHandle()

    def batch_multi_rows_call(self, handle, mode, patterns, k, reduced=True):
        self.log.append(("pass", mode, list(patterns), k, reduced))
        return _NoRows(), np.empty(0, dtype=np.uint32), [0] * (len(patterns) + 1)


@pytest.mark.parametrize("kind", ["bytes", "str", "mixed"])
@pytest.mark.parametrize("name", sorted(LIMITS))
def test_find_near_matches_multi_batch_routing_with_a_stub_engine(monkeypatch, kind, name):
    log = []
    seqs = {"bytes": [b"ACGTACGTAC", bytearray(b"TTT"), b""], "str": ["ACGTACGTAC", "caf\xe9", ""], "mixed": [b"ACGT", "ACGT"]}[kind]
    pats = [P9, "ACGTACGTA", P8, b"", bytearray(P9), "ACGTACGT"]
    held = batch.BatchSequences(seqs, engine=_StubEngine(log))
    assert held.kind == (None if kind == "mixed" else kind)
    assert [e[0] for e in log] == ([] if kind == "mixed" else ["upload"])

    def loop(p, sequences, *limits):
        assert sequences is held                          # the same held batch: no second upload
        log.append(("loop", p))
        return ["loop", p]

    monkeypatch.setattr(multi_batch, "find_near_matches_batch", loop)
    got = multi_batch.find_near_matches_multi_batch(pats, held, **LIMITS[name])
    riding, mode, k = multi_batch.multi_batch_routes(pats, held.kind, _params(LIMITS[name]))
    want_riding = {("bytes", "l2"): [0, 4], ("bytes", "subs2"): [0, 4], ("str", "l2"): [1]}.get((kind, name), [])
    assert riding == want_riding
    calls = [e for e in log if e[0] != "upload"]
    loops = [e for e in calls if e[0] == "loop"]
    assert [e[1] for e in loops] == [p for i, p in enumerate(pats) if i not in riding]      # input order
    if riding:
        assert calls[-1][0] == "pass" and calls[:-1] == loops                                # the loops first, then ONE pass
        coded = [pats[i].encode("latin-1") if kind == "str" else bytes(pats[i]) for i in riding]
        assert calls[-1] == ("pass", {"lev": LEV, "subs": SUBS}[mode], coded, 2, True)
    else:
        assert calls == loops
    for i, p in enumerate(pats):
        assert got[i] == ([[] for _ in seqs] if i in riding else ["loop", p])


def test_arguments_and_exports():
    import fuzzysearch_amd as fa
    assert "find_near_matches_multi_batch" in fa.__all__
    assert fa.find_near_matches_multi_batch is multi_batch.find_near_matches_multi_batch
    assert "fz_batch_search_multi" in _native.EXPORTED_SYMBOLS
    assert {"batch_search_multi", "batch_multi_rows_call"} <= set(dir(_native.Engine))
    assert fa.find_near_matches_multi_batch([], [b"ACGT"], max_l_dist=1) == []
    assert fa.find_near_matches_multi_batch([b"ACGT", b"AC"], [], max_l_dist=1) == [[], []]
    assert fa.find_near_matches_multi_batch(iter([b"ACGT"]), iter(()), max_l_dist=1) == [[]]
    with pytest.raises(ValueError) as single:
        fa.find_near_matches(b"ACGTACGTACGT", b"ACGTACGT", max_insertions=0, max_deletions=0)
    log = []
    held = batch.BatchSequences([b"ACGTACGT"], engine=_StubEngine(log))
    with pytest.raises(ValueError) as multi:
        fa.find_near_matches_multi_batch([b"ACGTACGTACGT"], held, max_insertions=0, max_deletions=0)
    assert str(multi.value) == str(single.value)
