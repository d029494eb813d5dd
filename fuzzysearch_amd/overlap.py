"""find_end_overlaps_batch: the beginning of a subsequence at the END of every sequence of a batch.

A read that runs into its adapter near its 3' end holds only the first 5, 12 or 25 bases of the adapter and then stops.  The
searches of this package find a whole subsequence within k edits; none of them sees such a read.  This call looks at the
last few dozen items of every sequence and answers, per sequence, which subsequence's strictly partial prefix ends there:

* the prefix lengths ``min_overlap <= i <= len(subsequence) - 1`` are considered (a whole occurrence, also one that ends at
  the sequence's end, is find_near_matches_batch's to find), each with the scaled budget ``k_i = k * i // len(subsequence)``;
* Levenshtein limits: ``E(i)`` = the smallest edit distance between the prefix and any suffix of the sequence, the suffix
  being the longest one at that distance (a prefix with deletions may be longer than the whole sequence);
  mismatch-only limits: ``E(i)`` = the Hamming distance to the last ``i`` items;
* a length qualifies when ``E(i) <= k_i``; the subsequence answers with the most matched items ``i - E(i)``, then the smaller
  ``E(i)``; the sequence answers with the subsequence of the largest ``i - d``, then the smaller ``d``, then the lower list
  position.

It is computed on the device in one launch per 8 (Levenshtein) or 64 (mismatch-only) subsequences (fz_batch_end_overlaps)
and comes back as arrays of one entry per sequence.  ``start`` is directly a cut position:
``reads.derive(ends=numpy.minimum(full_cut, overlaps.start))``.  There is no CPU fallback.
"""
import numpy as np

from . import _native
from .batch import BatchSequences, batch_kind, _single_device
from .common import LevenshteinSearchParams
from .engine import is_byteslike

__all__ = ['find_end_overlaps_batch', 'EndOverlaps']

# the domain of the device call (csrc/fz_device.h: FZ_OVL_*)
MAX_M, MAX_K, MAX_PATTERNS = 64, 16, 65534


class EndOverlaps(object):
    """The result of find_end_overlaps_batch: four numpy arrays of one entry per sequence.

    ``pattern`` (int32)  the list position of the subsequence whose prefix ends the sequence; -1 for none
    ``overlap`` (int32)  the length of that prefix, or 0
    ``dist`` (int32)     its distance to the end of the sequence, or -1
    ``start`` (int64)    where the overlap starts in the sequence; the sequence's length for none"""
    __slots__ = ('pattern', 'overlap', 'dist', 'start')

    def __init__(self, lengths):
        n = len(lengths)
        self.pattern = np.full(n, -1, dtype=np.int32)
        self.overlap = np.zeros(n, dtype=np.int32)
        self.dist = np.full(n, -1, dtype=np.int32)
        self.start = np.asarray(lengths, dtype=np.int64).copy()

    def __len__(self):
        return len(self.pattern)

    def __repr__(self):
        return 'EndOverlaps(%d sequences, %d found)' % (len(self), int((self.pattern >= 0).sum()))


def _from_rows(rows):
    """fz_overlap rows (Engine.batch_end_overlaps) -> EndOverlaps, no per-row Python work."""
    out = EndOverlaps.__new__(EndOverlaps)
    out.pattern = rows['pattern'].astype(np.int32)
    none = out.pattern == 0xffff
    out.pattern[none] = -1
    out.overlap = rows['overlap'].astype(np.int32)
    out.dist = rows['dist'].astype(np.int32)
    out.dist[none] = -1
    out.start = rows['start'].astype(np.int64)
    return out


def overlap_route(search_params):
    """-> ('lev' | 'subs', k) of the limits, or UnsupportedSearch: mismatch-only limits count mismatches, limits that the
    Levenshtein n-gram search serves count edits, and separate substitution / insertion / deletion limits have no form here."""
    max_subs, max_ins, max_dels, max_l = search_params.unpacked
    if max_ins == 0 and max_dels == 0:
        return 'subs', max_l
    if max_l <= min(max_subs, max_ins, max_dels):
        return 'lev', max_l
    raise _native.UnsupportedSearch('end overlaps take max_l_dist alone or mismatch-only limits: separate substitution / insertion / '
                                    'deletion limits are not supported')


def _checked_patterns(subsequences, k):
    patterns = []
    if len(subsequences) > MAX_PATTERNS:
        raise _native.UnsupportedSearch('end overlaps take at most %d subsequences' % MAX_PATTERNS)
    if k > MAX_K:
        raise _native.UnsupportedSearch('end overlaps take budgets up to %d' % MAX_K)
    for q, p in enumerate(subsequences):
        if not is_byteslike(p):
            raise _native.UnsupportedSearch('subsequence %d is not bytes-like: end overlaps compare bytes' % q)
        p = bytes(p)
        if not p:
            raise ValueError('subsequence %d is empty' % q)
        if len(p) > MAX_M:
            raise _native.UnsupportedSearch('subsequence %d is longer than %d bytes' % (q, MAX_M))
        if k >= len(p):
            raise _native.UnsupportedSearch('subsequence %d is not longer than the budget %d' % (q, k))
        patterns.append(p)
    return patterns


def find_end_overlaps_batch(subsequences, sequences,
                            max_substitutions=None,
                            max_insertions=None,
                            max_deletions=None,
                            max_l_dist=None,
                            min_overlap=3):
    """per sequence, the subsequence whose strictly partial prefix ends it -> EndOverlaps (arrays ``pattern``, ``overlap``,
    ``dist``, ``start`` of one entry per sequence; ``len()`` = the number of sequences).

    ``subsequences``: a list of bytes-like objects of 1 .. 64 bytes, or one of them.  ``sequences``: a list of bytes-like
    objects (packed and uploaded once, released afterwards) or a handle of resident_batch, resident_records,
    resident_fasta or derive.  ``max_l_dist`` alone (up to 16, below every subsequence's length) counts edits;
    ``max_insertions == max_deletions == 0`` counts mismatches.  Everything else raises UnsupportedSearch before anything is
    uploaded: other limits, a budget or a subsequence outside the domain (its list position is named), sequences that are
    not bytes, engines of several devices or in a communicator."""
    search_params = LevenshteinSearchParams(max_substitutions, max_insertions, max_deletions, max_l_dist)
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, int):
        raise TypeError('min_overlap must be an integer')
    if min_overlap < 1:
        raise ValueError('min_overlap must be at least 1')
    if is_byteslike(subsequences):
        subsequences = [subsequences]
    mode, k = overlap_route(search_params)
    patterns = _checked_patterns(list(subsequences), k)
    held = sequences if isinstance(sequences, BatchSequences) else None
    if held is None:
        seqs = list(sequences)
        if not seqs:
            return EndOverlaps([])
        if batch_kind(seqs) != 'bytes':
            raise _native.UnsupportedSearch('end overlaps take bytes-like sequences of one kind')
        engine = _native.default_engine()
    else:
        if held.kind != 'bytes' or held.handle is None:
            raise _native.UnsupportedSearch('end overlaps take a resident batch of bytes-like sequences')
        engine = held.engine
    if not _single_device(engine):
        raise _native.UnsupportedSearch('end overlaps are computed by single-device, non-collective engines')
    own = None
    if held is None:
        held = own = BatchSequences(seqs, engine)
    try:
        return _from_rows(engine.batch_end_overlaps(held.handle, _native.MODE_LEV if mode == 'lev' else _native.MODE_SUBS, patterns, k,
                                                    min_overlap))
    finally:
        if own is not None:
            own.release()
