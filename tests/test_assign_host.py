"""Best-pattern assignment per sequence, the parts that need no GPU: the order of the two table keys (fz_device.h:
fz_assign_key / fz_assign_key_hi, through a small g++ program's library), the fold of fz_batch_assign run on the host by the
functions its kernels run (fz_debug_assign_fold) against a ten-line model of the definition over the oracle's raw rows, and
the routing and merging of find_best_matches_batch with a stub engine.

Run as a program, the file prints the floors of the random draws (assigned sequences, tied sequences, winners other than
pattern 0), from the oracle alone."""
import ctypes
import os
import random
import subprocess
import tempfile
from collections import namedtuple

import numpy as np
import pytest

import oracle
from fuzzysearch_amd import _native, assign, batch
from tests.test_gpu_multi_batch import random_draw

HERE = os.path.dirname(os.path.abspath(__file__))
LEV, SUBS = 1, 2
REC_NONE = 0xffffffff
REC_DTYPE = np.dtype([("key", "<u8"), ("l", "<u4"), ("r", "<u4"), ("dist", "<u4"), ("aux", "<u4")])

KEY_PROGRAM = r"""
#include <cstddef>
#include <cstring>
#include "../fuzzysearch_amd/csrc/fz_device.h"
extern "C" {
unsigned long long key_lo(unsigned d, unsigned p, unsigned st, unsigned len, unsigned m, unsigned k) { return fz_assign_key(d, p, st, len, m, k); }
unsigned key_hi(unsigned d, unsigned p) { return fz_assign_key_hi(d, p); }
void key_decode(unsigned long long lo, unsigned hi, unsigned m, unsigned k, unsigned *out) {
    out[0] = fz_assign_key_dist(lo); out[1] = fz_assign_key_pattern(lo); out[2] = fz_assign_key_start(lo);
    out[3] = fz_assign_key_len(lo, m, k); out[4] = fz_assign_hi_dist(hi); out[5] = fz_assign_hi_pattern(hi);
}
}
"""


@pytest.fixture(scope="module")
def keys():
    tmp = tempfile.mkdtemp()
    src, out = os.path.join(tmp, "assign_keys.cpp"), os.path.join(tmp, "assign_keys.so")
    with open(src, "w") as f:
        f.write(KEY_PROGRAM.replace("../fuzzysearch_amd", os.path.join(HERE, "..", "fuzzysearch_amd")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", src, "-o", out])
    L = ctypes.CDLL(out)
    u = ctypes.c_uint32
    L.key_lo.restype = ctypes.c_uint64
    L.key_lo.argtypes = [u] * 6
    L.key_hi.restype = u
    L.key_hi.argtypes = [u, u]
    L.key_decode.restype = None
    L.key_decode.argtypes = [ctypes.c_uint64, u, u, u, ctypes.POINTER(u)]
    yield L
    os.remove(src)
    os.remove(out)
    os.rmdir(tmp)


def test_key_order_and_round_trip(keys):
    rnd = random.Random(1200)
    edge = [0, 1, 2, 126, 127]
    cases = []
    for _ in range(4000):
        k = rnd.choice([1, 2, 8, 100, 127])
        m = rnd.randint(k + 1, 65535)
        # (close neighbours: fields that differ in one position only are what an ordering gets wrong)
        d = rnd.choice(edge + [rnd.randint(0, 127)])
        p = rnd.choice([0, 1, 255, 256, 65534, rnd.randint(0, 65534)])
        st = rnd.choice([0, 1, 255, 256, (1 << 24) - 1, 1 << 24, (1 << 32) - 1, rnd.randrange(1 << 32)])
        ln = rnd.choice([m - k, m + k, rnd.randint(m - k, m + k)])
        cases.append((d, p, st, ln, m, k))
    out = (ctypes.c_uint32 * 6)()
    for d, p, st, ln, m, k in cases:
        keys.key_decode(keys.key_lo(d, p, st, ln, m, k), keys.key_hi(d, p), m, k, out)
        assert list(out) == [d, p, st, ln, d, p], "encode, then decode, is the identity"
        assert keys.key_lo(d, p, st, ln, m, k) != (1 << 64) - 1 and keys.key_hi(d, p) != (1 << 32) - 1, "all-ones is no key"
    for _ in range(4000):
        a, b = rnd.choice(cases), rnd.choice(cases)
        m, k = a[4], a[5]                                   # (one pattern length and budget: the last field is m + k - len)
        b = b[:3] + (min(max(b[3], m - k), m + k), m, k)
        ta, tb = (a[0], a[1], a[2], -a[3]), (b[0], b[1], b[2], -b[3])
        ka, kb = keys.key_lo(*a), keys.key_lo(*b)
        assert (ka < kb) == (ta < tb) and (ka == kb) == (ta == tb), (a, b)
        ha, hb = keys.key_hi(a[0], a[1]), keys.key_hi(b[0], b[1])
        assert (ha < hb) == ((a[0], -a[1]) < (b[0], -b[1])), "hi: the smaller distance, then the HIGHER pattern"


# ---- the model of the definition, and the draws shared with tests/test_gpu_assign.py ----------------------------------

def raw_rows(mode, p, s, k, cache):
    key = (mode, p, s, k)
    if key not in cache:
        cache[key] = oracle.lev_ngrams_raw(p, s, k) if mode == LEV else oracle.subs_ngrams_raw(p, s, k)
    return cache[key]


def model(rows_of, n_pats, n_seqs, k):
    """The definition, in pure Python.  rows_of(i, j) = the rows (start, end, dist, ...) of pattern i in sequence j ->
    per sequence (pattern, dist, tied, start, end), (-1, 0, 0, 0, 0) where nothing matches."""
    out = []
    for j in range(n_seqs):
        rows = [(r[2], i, r[0], -r[1]) for i in range(n_pats) for r in rows_of(i, j) if r[2] <= k]
        if not rows:
            out.append((-1, 0, 0, 0, 0))
            continue
        d, i, st, neg_end = min(rows)
        out.append((i, d, int(any(r[0] == d and r[1] != i for r in rows)), st, -neg_end))
    return out


def oracle_model(mode, pats, seqs, k, cache):
    return model(lambda i, j: raw_rows(mode, pats[i], seqs[j], k, cache), len(pats), len(seqs), k)


def as_tuples(rows):
    return [tuple(int(x) for x in r) for r in rows.tolist()]


def tally(want):
    """-> (assigned sequences, tied sequences, sequences whose winner is not pattern 0)."""
    return sum(w[0] >= 0 for w in want), sum(w[2] for w in want), sum(w[0] > 0 for w in want)


ASSIGN_SEED, ASSIGN_DRAWS = 1201, 16
# From the oracle alone (this file run as a program prints them): over all draws, the sequences that get a pattern, those
# with a tie, and those whose winner is not pattern 0.  A run that finds less found too little.
ASSIGN_FLOORS = (317, 13, 294)


def draws():
    rnd = random.Random(ASSIGN_SEED)
    return [(it,) + random_draw(rnd, it) for it in range(ASSIGN_DRAWS)]


def check_floors(total):
    assert all(f > 0 for f in ASSIGN_FLOORS), "floors are computed, not left empty"
    assert all(t >= f for t, f in zip(total, ASSIGN_FLOORS)), (total, ASSIGN_FLOORS)


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, seqs), dtype=np.uint64, count=len(seqs)), out=offs[1:])
    return b"".join(seqs), offs


def _records(rnd, mode, pats, seqs, offs, k, L, cache, single):
    """The oracle's rows of every (pattern, sequence) as verification records, shuffled: the n-gram hit somewhere inside the
    match (start = index - l, end = index + L + r), a block number in the key's upper bits, aux = the pattern's position (or
    noise when `single`: one table entry, aux ignored); plus empty slots and records beyond the budget, which do not count."""
    recs = []
    for i, p in enumerate(pats):
        for j, s in enumerate(seqs):
            for st, en, d, g in raw_rows(mode, p, s, k, cache):
                left = rnd.randint(0, en - st - L)
                idx = int(offs[j]) + st + left
                recs.append(((g << 48) | idx, left, en - st - L - left, d, rnd.randrange(1 << 20) if single else i))
    total = int(offs[-1])
    for _ in range(len(recs) // 5 + 3):
        if total:
            recs.append((rnd.randrange(total), 0, 0, rnd.choice([REC_NONE, k + 1, k + 100]), 0))
    rnd.shuffle(recs)
    return np.array(recs, dtype=REC_DTYPE) if recs else np.empty(0, dtype=REC_DTYPE)


def test_fold_hook_equals_the_model():
    total = [0, 0, 0]
    for it, mode, k, pats, seqs in draws():
        rnd = random.Random(it)
        cache = {}
        _, offs = pack(seqs)
        L = min(len(p) // (k + 1) for p in pats)            # (any n-gram length every match holds: only l + L + r counts)
        want = oracle_model(mode, pats, seqs, k, cache)
        pat_m = [len(p) for p in pats]
        table = [(i, len(p)) for i, p in enumerate(pats)]
        got = _native.assign_fold(offs, _records(rnd, mode, pats, seqs, offs, k, L, cache, False), L, table, pat_m, k)
        assert as_tuples(got) == want, (it, mode, k)
        total = [a + b for a, b in zip(total, tally(want))]
        # one pattern on its own: a table of one entry naming its list position, aux ignored
        i = rnd.randrange(len(pats))
        one = model(lambda _i, j: raw_rows(mode, pats[i], seqs[j], k, cache), 1, len(seqs), k)
        one = [(i if w[0] == 0 else -1,) + w[1:] for w in one]
        got = _native.assign_fold(offs, _records(rnd, mode, [pats[i]], seqs, offs, k, L, cache, True), L, [(i, len(pats[i]))], pat_m, k)
        assert as_tuples(got) == one, (it, mode, k, i)
    check_floors(total)


def test_fold_hook_edges():
    pat_m = [20, 20]
    table = [(0, 20), (1, 20)]
    none = (-1, 0, 0, 0, 0)
    offs = np.array([0, 0, 30, 30, 60], dtype=np.uint64)
    empty = np.empty(0, dtype=REC_DTYPE)
    assert as_tuples(_native.assign_fold(offs, empty, 6, table, pat_m, 2)) == [none] * 4
    assert as_tuples(_native.assign_fold(np.array([0], dtype=np.uint64), empty, 6, table, pat_m, 2)) == []
    assert as_tuples(_native.assign_fold(np.array([0, 0, 0], dtype=np.uint64), empty, 6, table, pat_m, 2)) == [none] * 2
    # flush against the seam on either side: the hit's own sequence; equal dist and start, two lengths: the longer one
    recs = np.array([(10 + 14, 14, 0, 1, 1), (30 + 6, 6, 8, 1, 0), (30 + 6, 6, 9, 1, 0), (30 + 6, 6, 7, 1, 0), (59, 0, 0, REC_NONE, 0),
                     (30 + 8, 6, 6, 2, 1)], dtype=REC_DTYPE)
    assert as_tuples(_native.assign_fold(offs, recs, 6, table, pat_m, 2)) == [none, (1, 1, 0, 10, 30), none, (0, 1, 0, 0, 21)]
    # outside the domain: refused
    for bad in (dict(k=128), dict(pat_m=[20] * 65536)):
        with pytest.raises(_native.UnsupportedSearch):
            _native.assign_fold(offs, recs, 6, table, bad.get("pat_m", pat_m), bad.get("k", 2))
    with pytest.raises(_native.UnsupportedSearch):
        _native.assign_fold(np.array([0, 1 << 32], dtype=np.uint64), empty, 6, table, pat_m, 2)
    with pytest.raises(ValueError):
        _native.assign_fold(offs, recs, 6, [(2, 20)], pat_m, 2)


# ---- the public call: routing and merging, with a stub engine -----------------------------------------------------------

M = namedtuple("M", "start end dist")
P9, P8 = b"ACGTACGTA", b"ACGTACGT"                          # 9 // 3 = 3: the n-gram route at k = 2; 8 // 3 = 2: linear programming


class _StubHandle(object):
    def release(self):
        pass


class _StubEngine(object):
    devices = [0]

    def __init__(self, log, rows):
        self.log, self.rows = log, rows

    def comm_info(self):
        return 0, -1, False

    def upload_batch(self, blob, offs):
        self.log.append(("upload",))
        return _StubHandle()

    def batch_assign(self, handle, mode, patterns, k):
        self.log.append(("assign", mode, list(patterns), k))
        return np.array(self.rows, dtype=_native.assign_dtype())


def test_public_routing_and_merge_with_a_stub_engine(monkeypatch):
    seqs = [b"s0", b"s1", b"s2", b"s3", b"s4", b"s5"]
    pats = [P8, P9, b"", bytearray(P9), P8[:7]]             # riding: 1 and 3 (the pass's patterns 0 and 1)
    # the pass: nothing / pattern 3 at 1 / pattern 1 at 1, tied / pattern 1 at 2 / pattern 3 at 0 / pattern 1 at 0
    rows = [(-1, 0, 0, 0, 0), (1, 1, 0, 5, 14), (0, 1, 1, 2, 11), (0, 2, 0, 0, 9), (1, 0, 0, 3, 12), (0, 0, 0, 1, 10)]
    loops = {
        bytes(P8): [[], [M(7, 15, 1), M(2, 10, 1), M(2, 11, 1), M(0, 9, 2)], [], [M(4, 12, 1)], [M(0, 8, 0)], [M(0, 8, 1)]],
        b"": [[], [], [], [], [], []],
        bytes(P8[:7]): [[M(1, 8, 2)], [], [M(3, 10, 1)], [M(0, 7, 1)], [], []],
    }
    log = []
    held = batch.BatchSequences(seqs, engine=_StubEngine(log, rows))

    def loop(p, sequences, *limits):
        assert sequences is held and limits == (None, None, None, 2)
        log.append(("loop", bytes(p)))
        return loops[bytes(p)]

    monkeypatch.setattr(assign, "find_near_matches_batch", loop)
    got = assign.find_best_matches_batch(pats, held, max_l_dist=2)
    assert log == [("upload",), ("loop", P8), ("loop", b""), ("loop", P8[:7]), ("assign", LEV, [P9, P9], 2)], "the loops first, then ONE pass"
    assert len(got) == 6
    assert got.pattern.dtype == np.int32 and got.dist.dtype == np.int32 and got.tied.dtype == np.bool_
    assert got.start.dtype == np.int64 and got.end.dtype == np.int64
    assert got.pattern.tolist() == [4, 0, 1, 0, 0, 1]
    assert got.dist.tolist() == [2, 1, 1, 1, 0, 0]
    # s1: patterns 0 and 3 at 1; s2: the pass's own tie, and pattern 4 at 1; s3: 0 and 4 at 1, the pass at 2; s4: 0 and 3 at 0
    assert got.tied.tolist() == [False, True, True, True, True, False]
    assert got.start.tolist() == [1, 2, 2, 4, 0, 1] and got.end.tolist() == [8, 11, 11, 12, 8, 10]
    # no patterns: all -1; no sequences: empty arrays; neither touches an engine
    none = assign.find_best_matches_batch([], [b"ACGT", b""], max_l_dist=1)
    assert len(none) == 2 and none.pattern.tolist() == [-1, -1] and none.dist.tolist() == [-1, -1]
    assert none.start.tolist() == [-1, -1] and none.end.tolist() == [-1, -1] and none.tied.tolist() == [False, False]
    assert len(assign.find_best_matches_batch([b"ACGT"], iter(()), max_l_dist=1)) == 0
    # the domain of the device tables
    with pytest.raises(_native.UnsupportedSearch):
        assign.find_best_matches_batch([b"A" * 600], held, max_l_dist=128)
    with pytest.raises(_native.UnsupportedSearch):
        assign.find_best_matches_batch([P9] * 65536, held, max_l_dist=2)


def test_exports_and_refusals():
    import fuzzysearch_amd as fa
    assert "find_best_matches_batch" in fa.__all__ and fa.find_best_matches_batch is assign.find_best_matches_batch
    assert {"fz_batch_assign", "fz_debug_assign_fold"} <= set(_native.EXPORTED_SYMBOLS)
    assert "batch_assign" in dir(_native.Engine)
    assert _native.assign_dtype().itemsize == 16
    with pytest.raises(ValueError) as single:
        fa.find_near_matches(b"ACGTACGTACGT", b"ACGTACGT", max_insertions=0, max_deletions=0)
    held = batch.BatchSequences([b"ACGTACGT"], engine=_StubEngine([], []))
    with pytest.raises(ValueError) as best:
        fa.find_best_matches_batch([b"ACGTACGTACGT"], held, max_insertions=0, max_deletions=0)
    assert str(best.value) == str(single.value)


if __name__ == "__main__":
    total = [0, 0, 0]
    for it, mode, k, pats, seqs in draws():
        total = [a + b for a, b in zip(total, tally(oracle_model(mode, pats, seqs, k, {})))]
    print("ASSIGN_FLOORS = (%d, %d, %d)" % tuple(total))
