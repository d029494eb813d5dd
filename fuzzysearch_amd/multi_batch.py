"""find_near_matches_multi_batch: many subsequences, many sequences, one call.

The value (and any exception) is that of ``[find_near_matches_batch(p, sequences, ...) for p in subsequences]``.  What is
new is the cost: the sequences are packed and uploaded once for the whole call (or are a ``resident_batch()`` handle), and
the subsequences whose route is the Levenshtein or the substitutions-only n-gram search go through ONE C-ABI call
(fz_batch_search_multi) that streams the packed bytes once per group of up to 64 subsequences and verifies every candidate
inside its own sequence — demultiplexing reads against a barcode list, screening reads for a panel of adapters or primers,
counting guides.

Everything else — the exact and linear-programming routes, separate substitution / insertion / deletion limits, ``str``
under substitutions-only limits, subsequences of another kind than the sequences, mixed kinds, an empty subsequence — takes
find_near_matches_batch over the same held batch, pattern by pattern, in input order, and before the pass runs: what those
routes refuse raises before anything is searched in bulk.
"""
import numpy as np

from . import _native
from .batch import BatchSequences, batch_route, find_near_matches_batch, _MODES, _fzmatch
from .common import LevenshteinSearchParams, RawMatches
from .engine import is_byteslike

__all__ = ['find_near_matches_multi_batch', 'multi_batch_routes']


def multi_batch_routes(subsequences, kind, search_params, single_device=True):
    """The routing decision, pure: -> (riding, mode, k).  `riding` = the positions of the subsequences that share the one
    fz_batch_search_multi call of mode `mode` ('lev' / 'subs') and budget k; every other position takes
    find_near_matches_batch.  batch_route decides per subsequence; the limits are the same for all of them, so every
    n-gram route it returns names the same mode and budget (None, None when nothing rides)."""
    riding, mode, k = [], None, None
    for i, p in enumerate(subsequences):
        route = batch_route(p, kind, search_params, single_device)
        if route is not None and route[0] in ('lev', 'subs'):
            if mode is None:
                mode, k = route
            elif (mode, k) != route:
                raise AssertionError('one set of limits selected two n-gram routes: %r and %r' % ((mode, k), route))
            riding.append(i)
    return riding, mode, k


def _pattern_bytes(p, kind):
    if kind == 'str':
        return p.encode('latin-1')
    return p if isinstance(p, bytes) else bytes(memoryview(p))


def _matches_per_pattern(rows, seq_of, bounds, sequences):
    """OwnedRows of every riding pattern's rows (pattern i: bounds[i] .. bounds[i + 1], each slice in sequence order) and
    the rows' sequence numbers -> per pattern one list of Match per sequence; the buffer is released."""
    out = []
    try:
        base = rows.address
        arr = None if _fzmatch is not None else rows.to_array()
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            per = [[] for _ in range(len(sequences))]
            if hi > lo:
                which, first = np.unique(seq_of[lo:hi], return_index=True)      # non-decreasing within a pattern's slice
                cuts = np.append(first, hi - lo).tolist()
                for j, a, b in zip(which.tolist(), cuts[:-1], cuts[1:]):
                    if arr is None:
                        per[j] = _fzmatch.make_matches_at(base + 24 * (lo + a), b - a, sequences[j], 0)
                    else:
                        per[j] = RawMatches(arr[lo + a:lo + b], sequences[j]).materialize()
            out.append(per)
        return out
    finally:
        rows.release()


def held_for_classes(subsequences, sequences, limits, classes):
    """What the two batch calls with ``classes`` share: every check (classes.class_call) before anything is uploaded, then
    the batch.  -> (patterns, k, tables, sequences as a list, held batch or None when there is nothing to search, owned)."""
    from .classes import class_call
    subsequences = list(subsequences)
    held = sequences if isinstance(sequences, BatchSequences) else None
    seqs = held.sequences if held is not None else list(sequences)
    if held is not None:
        byteslike = held.kind == 'bytes' or not seqs
    else:
        byteslike = all(is_byteslike(s) for s in seqs)
    patterns, k, tables = class_call(subsequences, limits, classes, byteslike)
    if not patterns or not seqs:
        return patterns, k, tables, seqs, None, None
    own = None
    if held is None:
        held = own = BatchSequences(seqs)
        if held.kind != 'bytes':
            own.release()
            raise _native.UnsupportedSearch('classes are searched by single-device, non-collective engines')
    return patterns, k, tables, seqs, held, own


def _find_with_classes(subsequences, sequences, limits, classes):
    patterns, k, tables, seqs, held, own = held_for_classes(subsequences, sequences, limits, classes)
    if held is None:
        return [[] for _ in patterns]
    try:
        rows, seq_of, bounds = held.engine.batch_multi_rows_call_classes(held.handle, patterns, k, tables, reduced=True)
        return _matches_per_pattern(rows, seq_of, bounds, seqs)
    finally:
        if own is not None:
            own.release()


def find_near_matches_multi_batch(subsequences, sequences,
                                  max_substitutions=None,
                                  max_insertions=None,
                                  max_deletions=None,
                                  max_l_dist=None,
                                  classes=None):
    """search for near-matches of every subsequence in every sequence -> a list with, per subsequence, one list of Match
    per sequence: ``[find_near_matches_batch(p, sequences, ...) for p in subsequences]`` (same limits for all of them).

    ``sequences`` may be a ``resident_batch()`` handle; otherwise the sequences are packed and uploaded once for the whole
    call.

    ``classes`` (a mapping such as ``fuzzysearch_amd.IUPAC_DNA``): the class distance of find_near_matches_multi, per
    sequence; mismatch-only limits, bytes-like sequences, every subsequence on the pass (fz_batch_search_multi_cls)."""
    if classes is not None:
        return _find_with_classes(subsequences, sequences, (max_substitutions, max_insertions, max_deletions, max_l_dist), classes)
    subsequences = list(subsequences)
    limits = (max_substitutions, max_insertions, max_deletions, max_l_dist)
    if not subsequences:
        return []
    held = sequences if isinstance(sequences, BatchSequences) else None
    seqs = held.sequences if held is not None else list(sequences)
    if not seqs:
        return [[] for _ in subsequences]
    search_params = LevenshteinSearchParams(*limits)
    own = None
    if held is None:
        held = own = BatchSequences(seqs)                 # one pack, one upload (kinds the batched call cannot hold: kept only)
    try:
        kind, engine = held.kind, held.engine
        riding, mode, k = multi_batch_routes(subsequences, kind, search_params)
        results = [None] * len(subsequences)
        on_pass = set(riding)
        for i, p in enumerate(subsequences):              # the per-pattern routes first: what they refuse raises before the pass runs
            if i not in on_pass:
                results[i] = find_near_matches_batch(p, held, *limits)
        if riding:
            patterns = [_pattern_bytes(subsequences[i], kind) for i in riding]
            rows, seq_of, bounds = engine.batch_multi_rows_call(held.handle, _MODES[mode], patterns, k, reduced=True)
            for i, per in zip(riding, _matches_per_pattern(rows, seq_of, bounds, seqs)):
                results[i] = per
        return results
    finally:
        if own is not None:
            own.release()
