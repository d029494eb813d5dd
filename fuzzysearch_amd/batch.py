"""find_near_matches_batch: one subsequence, many sequences, one call.

The value (and any exception) is that of ``[find_near_matches(subsequence, s, ...) for s in sequences]``.  What is new is
the cost: sequences of one kind — all bytes-like, or all latin-1 ``str`` — are packed back to back, uploaded once and
searched by ONE C-ABI call (fz_batch_search) that streams the packed bytes once and verifies every candidate inside its
own sequence, whatever the number of sequences.  The routes that call does not serve — separate substitution / insertion /
deletion limits, the linear-programming routes of short subsequences, other sequence kinds, mixed kinds, engines of several
devices or in a communicator — take the per-sequence code inside the same call.

``resident_batch(sequences)`` packs and uploads once and is accepted wherever ``sequences`` is: the way to keep millions
of reads in device memory across subsequences.  (The residency cache is not involved: a list can change.)
"""
import numpy as np

from . import _native
from .common import LevenshteinSearchParams, RawMatches
from .engine import is_byteslike

try:                                                # csrc/_fzmatch.c, built by fuzzysearch_amd.build
    from . import _fzmatch
    if not hasattr(_fzmatch, 'make_matches_at'):
        _fzmatch = None
except ImportError:
    _fzmatch = None

__all__ = ['find_near_matches_batch', 'resident_batch', 'BatchSequences', 'batch_route', 'pack_sequences']

_MODES = {'exact': _native.MODE_EXACT, 'lev': _native.MODE_LEV, 'subs': _native.MODE_SUBS}


def batch_kind(sequences):
    """'bytes' when every sequence is bytes-like, 'str' when every one is a latin-1 str, else None (other or mixed kinds)."""
    if not sequences:
        return None
    if all(is_byteslike(s) for s in sequences):
        return 'bytes'
    if all(isinstance(s, str) for s in sequences):
        try:
            for s in sequences:
                s.encode('latin-1')
        except UnicodeEncodeError:
            return None
        return 'str'
    return None


def batch_route(subsequence, kind, search_params, single_device=True):
    """The routing decision, pure: -> (mode, k) of the fz_batch_search call that answers for every sequence of a batch of
    kind `kind` ('bytes' / 'str' / None, see batch_kind), or None when the per-sequence loop runs.

    Batched: the subsequence is of the batch's kind (bytes-like, or a latin-1 str), and the strategy class the limits
    select sends a subsequence of this length down its exact or n-gram route with a result one C-ABI call delivers
    (the classes' one_call_route states their own rules)."""
    from . import choose_search_class
    if kind is None or not single_device:
        return None
    if kind == 'bytes':
        if not is_byteslike(subsequence):
            return None
    else:
        if not isinstance(subsequence, str):
            return None
        try:
            subsequence.encode('latin-1')
        except UnicodeEncodeError:
            return None
    if not len(subsequence):
        return None                                  # the loop raises what find_near_matches raises
    route_of = getattr(choose_search_class(search_params), 'one_call_route', None)
    if route_of is None:
        return None                                  # generic limits
    return route_of(len(subsequence), search_params, kind == 'bytes')


def pack_sequences(sequences, kind):
    """-> (the sequences' bytes back to back, numpy uint64 offsets of len(sequences) + 1 entries): one join, one cumulative sum."""
    if kind == 'str':
        blob = ''.join(sequences).encode('latin-1')
        lengths = np.fromiter(map(len, sequences), dtype=np.uint64, count=len(sequences))
    else:
        parts = [s if isinstance(s, (bytes, bytearray)) else memoryview(s) for s in sequences]
        blob = b''.join(parts)
        lengths = np.fromiter(map(len, parts), dtype=np.uint64, count=len(parts))
    offs = np.zeros(len(sequences) + 1, dtype=np.uint64)
    np.cumsum(lengths, out=offs[1:])
    return blob, offs


class BatchSequences(object):
    """Sequences packed and made resident once (fz_batch_upload); pass it as ``sequences`` to find_near_matches_batch.

    Sequences the batched call cannot hold (other or mixed kinds, an engine of several devices) are only kept: every
    search over them is the per-sequence loop.  ``len()``, indexing and ``matched`` come from the original objects, which
    are kept alive."""

    released = False                                # release() has been called: nothing can be derived from it any more

    def __init__(self, sequences, engine=None):
        self.sequences = list(sequences)
        self.engine = engine or _native.default_engine()
        self.kind = batch_kind(self.sequences) if _single_device(self.engine) else None
        self.handle = None
        if self.kind is not None:
            blob, offs = pack_sequences(self.sequences, self.kind)
            self.handle = self.engine.upload_batch(blob, offs)

    def __len__(self):
        return len(self.sequences)

    def __getitem__(self, item):
        return self.sequences[item]

    def release(self):
        self.released = True
        if self.handle is not None:
            self.handle.release()
            self.handle = None
            self.kind = None

    def derive(self, index=None, starts=None, ends=None, reverse=False, translate=None):
        """derive_batch(self, ...): a batch of cuts of these sequences, made on the device (derive.py)."""
        from .derive import derive_batch
        return derive_batch(self, index, starts, ends, reverse, translate)

    def score_cuts(self, scores=None, scores_5p=None, stop=True, max_miss_rate=None):
        """find_score_cuts_batch(self, ...): the cut positions of these sequences by a running sum of scores (cuts.py)."""
        from .cuts import find_score_cuts_batch
        return find_score_cuts_batch(self, scores, scores_5p, stop, max_miss_rate)

    def format(self, format=None, literals=None, out=None):
        """format_records(self, ...): the text of this one column, assembled on the device (egress.py); no format and no
        literals: 'lines'.  (A RecordBatch keeps the name of its record format in ``.format``: format_records(batch, 'lines').)"""
        from .egress import format_records
        if format is None and literals is None:
            format = 'lines'
        return format_records(self, format, literals, out)


def resident_batch(sequences, engine=None):
    """Pack ``sequences`` and upload them to HBM once -> a handle usable as ``sequences`` of find_near_matches_batch."""
    return BatchSequences(sequences, engine)


def _single_device(engine):
    if len(engine.devices) != 1:
        return False
    world, _rank, collective = engine.comm_info()
    return not (world and collective)


def _matches_per_sequence(rows, seq_of, sequences):
    """OwnedRows in sequence order + the rows' sequence numbers -> one list of Match per sequence; the buffer is released."""
    out = [[] for _ in range(len(sequences))]
    try:
        if rows.n == 0:
            return out
        which, first = np.unique(seq_of, return_index=True)      # seq_of is non-decreasing: slices of equal numbers
        bounds = np.append(first, len(seq_of)).tolist()
        if _fzmatch is not None:
            base = rows.address
            for j, lo, hi in zip(which.tolist(), bounds[:-1], bounds[1:]):
                out[j] = _fzmatch.make_matches_at(base + 24 * lo, hi - lo, sequences[j], 0)
        else:
            arr = rows.to_array()
            for j, lo, hi in zip(which.tolist(), bounds[:-1], bounds[1:]):
                out[j] = RawMatches(arr[lo:hi], sequences[j]).materialize()
        return out
    finally:
        rows.release()


def find_near_matches_batch(subsequence, sequences,
                            max_substitutions=None,
                            max_insertions=None,
                            max_deletions=None,
                            max_l_dist=None):
    """search for near-matches of subsequence in every sequence -> a list with one list of Match per sequence, equal to
    ``[find_near_matches(subsequence, s, ...) for s in sequences]`` (``matched`` and the coordinates are those of the
    sequence itself; a sequence without matches gives ``[]``, no sequences give ``[]``).

    ``sequences`` may be a ``resident_batch()`` handle."""
    from . import find_near_matches
    limits = (max_substitutions, max_insertions, max_deletions, max_l_dist)
    held = sequences if isinstance(sequences, BatchSequences) else None
    seqs = held.sequences if held is not None else list(sequences)
    if not seqs:
        return []
    search_params = LevenshteinSearchParams(*limits)
    if held is not None:
        kind, engine = held.kind, held.engine
    else:
        engine = _native.default_engine()
        kind = batch_kind(seqs) if _single_device(engine) else None
    route = batch_route(subsequence, kind, search_params)
    if route is None:
        return [find_near_matches(subsequence, s, *limits) for s in seqs]
    mode, k = route
    pattern = subsequence.encode('latin-1') if kind == 'str' else subsequence
    if held is not None:
        rows, seq_of = engine.batch_rows_call(held.handle, _MODES[mode], pattern, k, reduced=True)
    else:
        blob, offs = pack_sequences(seqs, kind)
        handle = engine.upload_batch(blob, offs)
        try:
            rows, seq_of = engine.batch_rows_call(handle, _MODES[mode], pattern, k, reduced=True)
        finally:
            handle.release()
    return _matches_per_sequence(rows, seq_of, seqs)
