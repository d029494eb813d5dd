"""find_best_matches_batch: many subsequences, many sequences, ONE answer per sequence.

Demultiplexing reads against a barcode list, screening against an adapter or primer panel and counting guides do not want
the P x S lists of Match that find_near_matches_multi_batch returns; they want, per sequence, which subsequence fits best,
at what distance, where, and whether another one fits equally well.  For the subsequences whose route is the Levenshtein
or the substitutions-only n-gram search that answer is computed on the device (fz_batch_assign: behind every verification
launch one more kernel folds the records, where they lie, into a per-sequence minimum) and comes back as arrays of one
entry per sequence: no rows are copied, ordered or turned into objects.

Everything else — the exact and linear-programming routes, separate substitution / insertion / deletion limits, ``str``
under substitutions-only limits, subsequences of another kind than the sequences — takes find_near_matches_batch over the
same held batch, pattern by pattern, in input order and before the pass runs (what those routes refuse raises before
anything is searched in bulk), and is folded into the arrays with the same ordering.
"""
import numpy as np

from . import _native
from .batch import BatchSequences, find_near_matches_batch, _MODES
from .common import LevenshteinSearchParams
from .multi_batch import multi_batch_routes, _pattern_bytes

__all__ = ['find_best_matches_batch', 'BestMatches']

# what the device tables' keys have room for (csrc/fz_device.h: fz_assign_key)
MAX_K, MAX_PATTERNS = 127, 65535                     # (a sequence of 2^32 bytes or more: refused by fz_batch_assign itself)


class BestMatches(object):
    """The result of find_best_matches_batch: five numpy arrays of one entry per sequence.

    ``pattern`` (int32)  the lowest index among the subsequences whose smallest distance in the sequence is the smallest
                         of all; -1 when none matches
    ``dist`` (int32)     that distance, or -1
    ``tied`` (bool)      at least one OTHER list position reaches the same distance in this sequence (a subsequence listed
                         twice ties with itself); False: every other one is at least one edit worse, or absent
    ``start``, ``end`` (int64, -1 when absent)  one occurrence of ``pattern`` at ``dist`` in the sequence's coordinates"""
    __slots__ = ('pattern', 'dist', 'start', 'end', 'tied')

    def __init__(self, n):
        self.pattern = np.full(n, -1, dtype=np.int32)
        self.dist = np.full(n, -1, dtype=np.int32)
        self.start = np.full(n, -1, dtype=np.int64)
        self.end = np.full(n, -1, dtype=np.int64)
        self.tied = np.zeros(n, dtype=bool)

    def __len__(self):
        return len(self.pattern)

    def __repr__(self):
        return 'BestMatches(%d sequences, %d assigned, %d tied)' % (len(self), int((self.pattern >= 0).sum()), int(self.tied.sum()))

    def merge(self, other):
        """Fold another partial result over the same sequences into this one: per sequence the smaller (dist, pattern)
        wins and keeps its position and its own ``tied``; equal distances from the two sides set ``tied``."""
        have, theirs = self.pattern >= 0, other.pattern >= 0
        both = have & theirs
        equal = both & (self.dist == other.dist)
        take = theirs & (~have | (other.dist < self.dist) | (equal & (other.pattern < self.pattern)))
        for name in self.__slots__:
            getattr(self, name)[take] = getattr(other, name)[take]
        self.tied |= equal
        return self


def _from_rows(rows):
    """fz_assign rows (Engine.batch_assign) -> BestMatches, no per-row Python work."""
    out = BestMatches(len(rows))
    have = rows['pattern'] >= 0
    out.pattern[:] = rows['pattern']
    out.dist[have] = rows['dist'][have]
    out.start[have] = rows['start'][have]
    out.end[have] = rows['end'][have]
    out.tied[:] = rows['tied'] != 0
    return out


def _from_matches(index, per_sequence):
    """One subsequence's public matches per sequence -> its partial result: the smallest distance, and among the matches
    at that distance the smallest start, then the largest end."""
    out = BestMatches(len(per_sequence))
    for j, matches in enumerate(per_sequence):
        if matches:
            best = min(matches, key=lambda x: (x.dist, x.start, -x.end))
            out.pattern[j], out.dist[j], out.start[j], out.end[j] = index, best.dist, best.start, best.end
    return out


def _best_with_classes(subsequences, sequences, limits, classes):
    from .multi_batch import held_for_classes
    subsequences = list(subsequences)
    if len(subsequences) > MAX_PATTERNS:
        raise _native.UnsupportedSearch('best-pattern assignment takes at most %d subsequences' % MAX_PATTERNS)
    patterns, k, tables, seqs, held, own = held_for_classes(subsequences, sequences, limits, classes)
    if held is None:
        return BestMatches(len(seqs))
    try:
        return _from_rows(held.engine.batch_assign_classes(held.handle, patterns, k, tables))
    finally:
        if own is not None:
            own.release()


def find_best_matches_batch(subsequences, sequences,
                            max_substitutions=None,
                            max_insertions=None,
                            max_deletions=None,
                            max_l_dist=None,
                            classes=None):
    """the best-fitting subsequence per sequence -> BestMatches (arrays ``pattern``, ``dist``, ``start``, ``end``, ``tied``
    of one entry per sequence; ``len()`` = the number of sequences).

    ``pattern``, ``dist`` and ``tied`` are what one computes from find_near_matches_multi_batch's output: the smallest
    distance any subsequence reaches in the sequence, the lowest list position that reaches it, and whether another
    position reaches it too (a consolidation group keeps its minimum distance, so consolidated and raw matches agree on
    all three).  Only the position is defined on the RAW matches, because overlap groups are not a device-side notion:
    for the subsequences on the Levenshtein or substitutions-only n-gram route (``start``, ``end``) is, among the winning
    subsequence's raw n-gram matches at ``dist`` in that sequence (``Engine.batch_search(..., reduced=False)``), the one
    with the smallest start, then the largest end; for every other route it is chosen the same way among the public
    matches of find_near_matches_batch.  Which route a subsequence takes is a function of the arguments (batch_route).

    ``sequences`` may be a ``resident_batch()`` handle.  Refusals are those of find_near_matches_batch, with its exception
    types and texts; in addition UnsupportedSearch for an n-gram budget above 127, more than 65 535 subsequences or a
    sequence of 2^32 items or more.  No subsequences: every entry is -1.  No sequences: empty arrays.

    ``classes`` (a mapping such as ``fuzzysearch_amd.IUPAC_DNA``): the same answer under the class distance of
    find_near_matches_multi — mismatch-only limits, bytes-like sequences, every subsequence on the pass (fz_batch_assign_cls)."""
    if classes is not None:
        return _best_with_classes(subsequences, sequences, (max_substitutions, max_insertions, max_deletions, max_l_dist), classes)
    subsequences = list(subsequences)
    limits = (max_substitutions, max_insertions, max_deletions, max_l_dist)
    held = sequences if isinstance(sequences, BatchSequences) else None
    seqs = held.sequences if held is not None else list(sequences)
    result = BestMatches(len(seqs))
    if not subsequences or not seqs:
        return result
    if len(subsequences) > MAX_PATTERNS:
        raise _native.UnsupportedSearch('best-pattern assignment takes at most %d subsequences' % MAX_PATTERNS)
    search_params = LevenshteinSearchParams(*limits)
    own = None
    if held is None:
        held = own = BatchSequences(seqs)                 # one pack, one upload (kinds the batched call cannot hold: kept only)
    try:
        kind, engine = held.kind, held.engine
        riding, mode, k = multi_batch_routes(subsequences, kind, search_params)
        if riding and k > MAX_K:
            raise _native.UnsupportedSearch('best-pattern assignment takes n-gram budgets up to %d' % MAX_K)
        on_pass = set(riding)
        for i, p in enumerate(subsequences):              # the per-pattern routes first: what they refuse raises before the pass runs
            if i not in on_pass:
                result.merge(_from_matches(i, find_near_matches_batch(p, held, *limits)))
        if riding:
            patterns = [_pattern_bytes(subsequences[i], kind) for i in riding]
            part = _from_rows(engine.batch_assign(held.handle, _MODES[mode], patterns, k))
            have = part.pattern >= 0
            part.pattern[have] = np.asarray(riding, dtype=np.int32)[part.pattern[have]]      # list positions (ascending, as the pass's)
            result.merge(part)
        return result
    finally:
        if own is not None:
            own.release()
