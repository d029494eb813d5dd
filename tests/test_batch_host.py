"""CPU only: the host half of find_near_matches_batch — the ragged-segment lookup the kernels run (fz_segment_ragged with its
per-tile bound, through fz_debug_batch_segment), the routing decision and the packing."""
import ctypes

import numpy as np
import pytest

from fuzzysearch_amd import _native, batch
from fuzzysearch_amd.common import LevenshteinSearchParams

TILE = 16384


def _offs(lengths):
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lengths, dtype=np.uint64), out=offs[1:])
    return offs


def _check_table(lengths, every=1):
    offs = _offs(lengths)
    ends = offs[1:]
    total = int(offs[-1])
    idx = np.arange(0, total, every, dtype=np.uint64)
    want_j = np.searchsorted(ends, idx, 'right')
    # (the C function itself with its arguments made once: a million calls)
    fn = _native.load_library().fz_debug_batch_segment
    optr = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    j_, sa_, se_ = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rj, rsa, rse = ctypes.byref(j_), ctypes.byref(sa_), ctypes.byref(se_)
    lo, hi = offs[:-1].tolist(), offs[1:].tolist()
    for i, j in zip(idx.tolist(), want_j.tolist()):
        assert fn(optr, len(lengths), i, rj, rsa, rse) == 0
        assert (j_.value, sa_.value, se_.value) == (j, lo[j], hi[j]), (i, j)
    if total:
        assert _native.batch_segment(offs, total - 1) == (int(want_j[-1]), lo[int(want_j[-1])], hi[int(want_j[-1])])
    with pytest.raises(ValueError):
        _native.batch_segment(offs, total)
    return total


def test_lookup_small_tables():
    rnd = np.random.RandomState(5)
    tables = [
        [7],                                                     # a single sequence
        [3 * TILE + 5],                                          # ... of several tiles
        [0, 0, 0, 5, 0, 0, 9, 0],                                # empty sequences at the front, in runs and at the end
        [TILE, TILE, TILE],                                      # sequences exactly one tile long
        [TILE - 1, 1, TILE, 1, TILE + 1, 0, 0, 2],               # seams at and next to tile edges
        [0] * 40 + [2 * TILE + 3] + [0] * 40 + [1],
        list(rnd.randint(0, 300, size=400)),                     # many sequences per tile
        list(rnd.choice([0, 1, 150, TILE - 2, TILE + 2, 2 * TILE], size=12)),
    ]
    for lengths in tables:
        assert _check_table([int(x) for x in lengths]) == sum(int(x) for x in lengths)


def test_lookup_fifty_thousand_short_sequences():
    rnd = np.random.RandomState(6)
    lengths = rnd.randint(0, 41, size=50000)
    _check_table([int(x) for x in lengths])


def test_lookup_all_empty():
    offs = _offs([0, 0, 0])
    with pytest.raises(ValueError):
        _native.batch_segment(offs, 0)


LIMITS = {
    'l2': dict(max_l_dist=2),
    'l0': dict(max_l_dist=0),
    'subs2': dict(max_substitutions=2, max_insertions=0, max_deletions=0),
    'subs2_l': dict(max_substitutions=2, max_insertions=0, max_deletions=0, max_l_dist=2),
    'all2': dict(max_substitutions=2, max_insertions=2, max_deletions=2, max_l_dist=2),          # Levenshtein class
    'generic': dict(max_substitutions=1, max_insertions=1, max_deletions=1, max_l_dist=2),
    'generic_noins': dict(max_substitutions=2, max_insertions=0, max_deletions=1),
}


def _route(p, seqs, **limits):
    params = LevenshteinSearchParams(limits.get('max_substitutions'), limits.get('max_insertions'),
                                     limits.get('max_deletions'), limits.get('max_l_dist'))
    return batch.batch_route(p, batch.batch_kind(seqs), params)


def test_kinds():
    assert batch.batch_kind([b'ab', b'']) == 'bytes'
    assert batch.batch_kind([b'ab', bytearray(b'cd'), memoryview(b'ef')]) == 'bytes'
    assert batch.batch_kind(['ab', 'c\xe9']) == 'str'
    assert batch.batch_kind(['ab', 'cł']) is None           # not latin-1
    assert batch.batch_kind([b'ab', 'cd']) is None               # mixed
    assert batch.batch_kind([[1, 2], [3]]) is None               # lists of ints
    assert batch.batch_kind([(1, 2)]) is None
    assert batch.batch_kind([]) is None


def test_routing():
    p9 = b'ACGTACGTA'                       # 9 // 3 = 3: n-gram route at k = 2
    p8 = b'ACGTACGT'                        # 8 // 3 = 2: linear programming at k = 2
    seqs = [b'ACGTACGTAC', bytearray(b'TTT'), b'']
    assert _route(p9, seqs, **LIMITS['l2']) == ('lev', 2)
    assert _route(p8, seqs, **LIMITS['l2']) is None
    assert _route(p9, seqs, **LIMITS['all2']) == ('lev', 2)
    assert _route(p9, seqs, **LIMITS['l0']) == ('exact', 0)
    assert _route(b'A', seqs, **LIMITS['l0']) == ('exact', 0)
    assert _route(p9, seqs, **LIMITS['subs2']) == ('subs', 2)
    assert _route(p9, seqs, **LIMITS['subs2_l']) == ('subs', 2)
    assert _route(p8, seqs, **LIMITS['subs2']) is None
    assert _route(p9, seqs, **LIMITS['generic']) is None
    assert _route(p9, seqs, **LIMITS['generic_noins']) is None
    assert _route(bytearray(p9), seqs, **LIMITS['l2']) == ('lev', 2)
    assert _route(b'', seqs, **LIMITS['l2']) is None                       # the loop raises
    assert _route('ACGTACGTA', seqs, **LIMITS['l2']) is None               # str subsequence, bytes sequences
    # str batches
    strs = ['ACGTACGTAC', 'caf\xe9', '']
    assert _route('ACGTACGTA', strs, **LIMITS['l2']) == ('lev', 2)
    assert _route('ACGTACGTA', strs, **LIMITS['l0']) == ('exact', 0)
    assert _route('ACGTACGTA', strs, **LIMITS['subs2']) is None            # str: every window, not the best of groups
    assert _route('ACGTACGTł', strs, **LIMITS['l2']) is None          # subsequence outside latin-1
    assert _route(p9, strs, **LIMITS['l2']) is None                        # bytes subsequence, str sequences
    assert _route('ACGTACGTA', strs + ['ł'], **LIMITS['l2']) is None  # a sequence outside latin-1
    # other and mixed kinds
    assert _route(p9, [b'ACGT', 'ACGT'], **LIMITS['l2']) is None
    assert _route([1, 2, 3, 4, 5, 6, 7, 8, 9], [[1, 2, 3], [4]], **LIMITS['l2']) is None
    # an engine of several devices or in a communicator
    params = LevenshteinSearchParams(None, None, None, 2)
    assert batch.batch_route(p9, 'bytes', params, single_device=False) is None
    assert batch.batch_route(p9, 'bytes', params, single_device=True) == ('lev', 2)


def test_routing_agrees_with_the_single_call_rules():
    """The boundary between the n-gram and the linear-programming routes is where the strategy classes put it."""
    for k in (1, 2, 3, 4, 8):
        params = LevenshteinSearchParams(None, None, None, k)
        for m in range(1, 6 * (k + 1)):
            want = ('lev', k) if m // (k + 1) >= 3 else None
            assert batch.batch_route(b'A' * m, 'bytes', params) == want, (m, k)
        sub = LevenshteinSearchParams(k, 0, 0, None)
        for m in range(1, 6 * (k + 1)):
            want = ('subs', k) if m // (k + 1) >= 3 else None
            assert batch.batch_route(b'A' * m, 'bytes', sub) == want, (m, k)


def test_packing():
    seqs = [b'abc', bytearray(b''), memoryview(b'defgh'), b'', b'i']
    blob, offs = batch.pack_sequences(seqs, 'bytes')
    assert blob == b'abcdefghi'
    assert offs.dtype == np.uint64 and offs.tolist() == [0, 3, 3, 8, 8, 9]
    blob, offs = batch.pack_sequences(['ab', '', 'c\xe9'], 'str')
    assert blob == b'abc\xe9' and offs.tolist() == [0, 2, 2, 4]
    blob, offs = batch.pack_sequences([b''], 'bytes')
    assert blob == b'' and offs.tolist() == [0, 0]


def test_exports():
    import fuzzysearch_amd as fa
    assert 'find_near_matches_batch' in fa.__all__ and 'resident_batch' in fa.__all__
    assert fa.find_near_matches_batch is batch.find_near_matches_batch
    assert fa.find_near_matches_batch(b'abc', [], max_l_dist=1) == []
