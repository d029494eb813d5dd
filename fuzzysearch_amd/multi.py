"""find_near_matches_multi: many subsequences, one sequence, one call.

The value (and any exception) is that of ``[find_near_matches(p, sequence, ...) for p in subsequences]``.  What is new
is the cost: the sequence is prepared once (one residency-cache acquire, or one upload), and the patterns on an n-gram
route go through ONE C-ABI call that tests every byte offset of the sequence against the n-gram blocks of up to 64 patterns
per pass:

* the Levenshtein n-gram route (``max_l_dist`` alone, or limits that do not bind): fz_lev_ngrams_multi_consolidated;
* the substitutions-only n-gram route (``max_insertions=0, max_deletions=0`` — mismatch lists such as guides, barcodes and
  primers): fz_subs_ngrams_multi_best for bytes-like sequences (the best match of every overlap group), the raw
  fz_subs_ngrams_multi for latin-1 ``str`` sequences, whose result is every window once, sorted by start.

Everything else — the generic class, the exact and linear-programming routes, sequences whose coding depends on the
subsequence — takes the per-pattern code inside the same call, with the results in input order.

``classes=`` (classes.py: IUPAC patterns) is answered by the pass alone: fz_subs_ngrams_multi_best_cls for the whole list.
"""
from ._native import MODE_LEV, MODE_SUBS, UnsupportedSearch
from .common import LevenshteinSearchParams, matches_from_rows_multi
from .engine import DeviceSequence, is_byteslike, prepare_shared

__all__ = ['find_near_matches_multi']


def _batch_pattern(p, byteslike):
    """The bytes of subsequence `p` as the resident sequence is coded, or None when it cannot ride the batched call."""
    if byteslike:
        return bytes(memoryview(p)) if is_byteslike(p) else None
    if isinstance(p, str):
        try:
            return p.encode('latin-1')
        except UnicodeEncodeError:
            return None
    return None


def _find_with_classes(subsequences, sequence, limits, classes):
    from .classes import class_call
    subsequences = list(subsequences)
    byteslike = sequence.byteslike if isinstance(sequence, DeviceSequence) else is_byteslike(sequence)
    patterns, k, tables = class_call(subsequences, limits, classes, byteslike)
    if not patterns:
        return []
    shared = prepare_shared(sequence)
    if shared is None:
        raise UnsupportedSearch('classes are searched in bytes-like sequences only')
    pr = shared[0]
    try:
        rows, bounds = pr.engine.multi_rows_call_classes(pr.handle, patterns, k, tables)
        return matches_from_rows_multi(rows, bounds, pr.original)
    finally:
        pr.release()


def find_near_matches_multi(subsequences, sequence,
                            max_substitutions=None,
                            max_insertions=None,
                            max_deletions=None,
                            max_l_dist=None,
                            classes=None):
    """search for near-matches of every subsequence in sequence -> a list with one list of Match per subsequence,
    equal to ``[find_near_matches(p, sequence, ...) for p in subsequences]`` (same limits for all of them).

    ``sequence`` may be a ``resident()`` handle.  The first subsequence that ``find_near_matches`` would refuse raises
    its exception before anything is searched.

    ``classes`` (a mapping such as ``fuzzysearch_amd.IUPAC_DNA``: pattern byte -> the sequence bytes it accepts) searches
    under the class distance instead: mismatch-only limits, a bytes-like sequence, every subsequence on the multi-pattern
    pass (``UnsupportedSearch`` otherwise, naming the list position).  Per subsequence: every window within the budget,
    reduced to the best match of every overlap group."""
    if classes is not None:
        return _find_with_classes(subsequences, sequence, (max_substitutions, max_insertions, max_deletions, max_l_dist), classes)
    from . import find_near_matches, choose_search_class, LevenshteinSearch, SubstitutionsOnlySearch
    from .substitutions_only import _finish_ngrams
    subsequences = list(subsequences)
    if not subsequences:
        return []
    limits = (max_substitutions, max_insertions, max_deletions, max_l_dist)
    search_params = LevenshteinSearchParams(*limits)
    search_class = choose_search_class(search_params)
    subs = search_class is SubstitutionsOnlySearch
    k = min(search_params.max_l_dist, search_params.max_substitutions) if subs else search_params.max_l_dist
    batched_class = (subs or search_class is LevenshteinSearch) and k > 0
    shared = prepare_shared(sequence) if all(len(p) for p in subsequences) else None
    if shared is None:
        # nothing to share (or an empty subsequence, which raises at its turn): today's code, pattern by pattern
        return [find_near_matches(p, sequence, *limits) for p in subsequences]
    pr, view = shared
    try:
        results = [None] * len(subsequences)
        batch = []
        for i, p in enumerate(subsequences):
            pb = _batch_pattern(p, pr.byteslike) if batched_class and len(p) // (k + 1) >= 3 else None
            if pb is not None:
                batch.append((i, pb))
        riding = set(i for i, _ in batch)
        for i, p in enumerate(subsequences):             # the per-pattern routes first: what they refuse raises before the batch runs
            if i not in riding:
                # (a subsequence of the wrong kind for the sequence meets the sequence itself: find_near_matches' own error)
                fits = is_byteslike(p) if pr.byteslike else isinstance(p, str)
                results[i] = find_near_matches(p, view if fits else sequence, *limits)
        if batch and subs and not pr.byteslike:
            # str: every window once, sorted by start — from the raw streams, as the single call makes it
            raws = pr.engine.subs_ngrams_multi(pr.handle, [pb for _, pb in batch], k, as_array=True)
            for (i, _), raw in zip(batch, raws):
                results[i] = _finish_ngrams(raw, pr.original, False)
        elif batch:
            rows, bounds = pr.engine.multi_rows_call(pr.handle, [pb for _, pb in batch], k, MODE_SUBS if subs else MODE_LEV)
            for (i, _), matches in zip(batch, matches_from_rows_multi(rows, bounds, pr.original)):
                results[i] = matches
        return results
    finally:
        pr.release()
