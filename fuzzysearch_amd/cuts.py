"""find_score_cuts_batch: where to cut every sequence of a batch by a running sum of scores taken from its end.

Quality trimming (the running-sum rule of BWA) and poly-A trimming are the same computation: a table of one signed score
per byte value, a running sum from the sequence's end, and the position where that sum peaks.  Per sequence ``r`` of ``n``
items, a table ``w``, a flag ``stop`` and an optional miss rate ``num / den`` (a miss: an item with ``w < 0``)::

    cut3(r):  s = best = miss = 0; cut = n
              for i = n - 1 down to 0:
                  s += w[r[i]]; miss += (w[r[i]] < 0)
                  if stop and s < 0: break
                  if s > best and (no rate or miss * den <= num * (n - i)): best = s; cut = i
              return cut
    cut5(r) = n - cut3(reversed r)

The comparison is strict: of equal peaks the one nearest the end wins.  ``quality_cuts`` is the table ``cutoff - (b - base)``
with ``stop``; ``poly_tail_cuts`` scores the base +1 and every other byte -2 without ``stop``, under a miss rate of 1 / 5.

It is computed on the device in one launch, one lane per sequence (fz_batch_score_cuts), and comes back as two arrays of one
entry per sequence.  Both are cut positions as they stand: ``reads.derive(starts=cuts.start, ends=cuts.end)``, or
``numpy.minimum(adapter_cut, cuts.end)`` next to an adapter's.  There is no CPU fallback.
"""
from fractions import Fraction

import numpy as np

from . import _native
from .batch import BatchSequences, batch_kind, _single_device
from .engine import is_byteslike

__all__ = ['find_score_cuts_batch', 'quality_cuts', 'poly_tail_cuts', 'ScoreCuts', 'score_table']


class ScoreCuts(object):
    """The result of find_score_cuts_batch: two numpy arrays (int64) of one entry per sequence.

    ``start``  what the 5' side cuts: the sequence keeps ``[start, end)``; 0 when that side was not asked for
    ``end``    what the 3' side cuts; the sequence's length when that side was not asked for
    Both sides asked for and nothing left between them: both are 0, the empty sequence."""
    __slots__ = ('start', 'end')

    def __init__(self, start, end):
        self.start = np.asarray(start, dtype=np.int64)
        self.end = np.asarray(end, dtype=np.int64)

    def __len__(self):
        return len(self.end)

    def __repr__(self):
        return 'ScoreCuts(%d sequences)' % len(self)


def _from_rows(rows):
    """fz_cut rows (Engine.batch_score_cuts) -> ScoreCuts, no per-row Python work."""
    return ScoreCuts(rows['start'].astype(np.int64), rows['end'].astype(np.int64))


def _byte_of(key):
    if isinstance(key, (bytes, bytearray)) and len(key) == 1:
        return key[0]
    if isinstance(key, int) and not isinstance(key, bool) and 0 <= key <= 255:
        return key
    raise ValueError('a score table is keyed by byte values: integers 0 .. 255 or bytes of length 1, not %r' % (key,))


def score_table(scores):
    """``scores`` -> a numpy int16 array of 256 scores.  Either 256 integers, or a mapping from a byte (an ``int`` or ``bytes``
    of length 1) to an integer with the key ``'default'`` for every byte it does not name (0 without it).  Scores outside
    the int16 range raise ValueError."""
    if hasattr(scores, 'items'):
        items = dict(scores)
        values = [items.pop('default', 0)] * 256
        for key, value in items.items():
            values[_byte_of(key)] = value
    else:
        values = list(scores)
        if len(values) != 256:
            raise ValueError('a score table has 256 entries, not %d' % len(values))
    for b, v in enumerate(values):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError('the score of byte %d is not an integer' % b)
        if not -32768 <= v <= 32767:
            raise ValueError('the score of byte %d is outside the int16 range: %d' % (b, v))
    return np.array(values, dtype=np.int16)


def _rate(max_miss_rate):
    if max_miss_rate is None:
        return None
    if isinstance(max_miss_rate, Fraction):
        num, den = max_miss_rate.numerator, max_miss_rate.denominator
    else:
        num, den = max_miss_rate
        if isinstance(num, bool) or isinstance(den, bool) or not isinstance(num, int) or not isinstance(den, int):
            raise TypeError('max_miss_rate is a pair of integers or a fractions.Fraction')
    if den <= 0 or num < 0:
        raise ValueError('max_miss_rate must be num / den with num >= 0 and den > 0')
    if num >= 1 << 32 or den >= 1 << 32:
        raise ValueError('max_miss_rate takes numerators and denominators below 2^32')
    return num, den


def find_score_cuts_batch(sequences, scores=None, scores_5p=None, stop=True, max_miss_rate=None):
    """per sequence, where the running sum of ``scores`` from its 3' end and / or of ``scores_5p`` from its 5' end peaks ->
    ScoreCuts (arrays ``start`` and ``end`` of one entry per sequence; ``len()`` = the number of sequences).

    ``scores`` / ``scores_5p``: a table (score_table: 256 integers, or a mapping byte -> integer with ``'default'``) or None
    for a side that is not asked for, which gives ``start = 0`` / ``end = lengths``.  ``stop``: the walk ends at the first
    negative sum.  ``max_miss_rate``: ``(num, den)`` or a ``fractions.Fraction``, in force without ``stop``: a cut is taken
    only where the items with a negative score are at most that share of what it cuts.  ``sequences``: a list of bytes-like
    objects (packed and uploaded once, released afterwards) or a handle of resident_batch, resident_records, resident_fasta
    or derive.  UnsupportedSearch is raised before anything is uploaded for sequences that are not bytes, mixed kinds, and
    engines of several devices or in a communicator."""
    if scores is None and scores_5p is None:
        raise ValueError('no table given: scores, scores_5p or both')
    w3 = None if scores is None else score_table(scores)
    w5 = None if scores_5p is None else score_table(scores_5p)
    rate = _rate(max_miss_rate)
    flags = (_native.CUT_STOP3 | _native.CUT_STOP5) if stop else 0
    if rate is not None and not stop:
        flags |= _native.CUT_RATE
    num, den = rate if rate is not None else (0, 1)
    held = sequences if isinstance(sequences, BatchSequences) else None
    if held is None:
        seqs = list(sequences)
        if not seqs:
            return ScoreCuts([], [])
        if batch_kind(seqs) != 'bytes':
            raise _native.UnsupportedSearch('score cuts take bytes-like sequences of one kind')
        engine = _native.default_engine()
    else:
        if held.kind != 'bytes' or held.handle is None:
            raise _native.UnsupportedSearch('score cuts take a resident batch of bytes-like sequences')
        engine = held.engine
    if not _single_device(engine):
        raise _native.UnsupportedSearch('score cuts are computed by single-device, non-collective engines')
    own = None
    if held is None:
        held = own = BatchSequences(seqs, engine)
    try:
        return _from_rows(engine.batch_score_cuts(held.handle, w3, w5, flags, num, den))
    finally:
        if own is not None:
            own.release()


def quality_cuts(quals, cutoff, cutoff_5p=None, base=33):
    """Quality trimming by the running-sum rule of BWA -> ScoreCuts.  ``quals``: the quality strings (a list or a batch handle,
    e.g. the third batch of ``resident_records(path, lines=(0, 1, 3))``); ``cutoff``: the 3' cutoff, None for none;
    ``cutoff_5p``: the 5' cutoff; ``base``: the byte of quality 0.  The table is ``cutoff - (b - base)``, with ``stop``."""
    if cutoff is None and cutoff_5p is None:
        raise ValueError('no cutoff given: cutoff, cutoff_5p or both')
    tables = [None if q is None else [q - (b - base) for b in range(256)] for q in (cutoff, cutoff_5p)]
    return find_score_cuts_batch(quals, tables[0], tables[1], stop=True)


def poly_tail_cuts(reads, base=b'A', hit=1, miss=-2, max_miss_rate=(1, 5)):
    """Poly-A (or poly-``base``) tail trimming -> ScoreCuts whose ``end`` is where the tail starts: ``base`` scores ``hit``,
    every other byte ``miss``, no ``stop``, and a tail is taken only while its other bytes are within ``max_miss_rate``."""
    return find_score_cuts_batch(reads, {_byte_of(base): hit, 'default': miss}, stop=False, max_miss_rate=max_miss_rate)
