"""derive_batch: a batch made from a batch on the device — select, trim, reverse, map.

One rule, whose model is three lines of Python::

    out[j] = X(src[i_j][a_j:b_j])            for j in range(n_out)
      i_j = index[j]   (index None: j, and n_out = len(src))
      a_j = starts[j]  (None: 0)
      b_j = ends[j]    (None: len(src[i_j]))
      X   = byte by byte through a 256-byte table (None: identity), then reversed if reverse=True

``starts`` / ``ends`` are per OUTPUT and local to the source sequence ``i_j``; ``index`` may repeat and come in any order (the
derived batch may be larger than its parent); empty outputs are sequences like any other.  An item is bad when
``i_j >= len(src)`` (``IndexError``), ``a_j > b_j`` or ``b_j > len(src[i_j])`` (``ValueError``): the smallest bad ``j`` is
named, nothing is made, and the next call works.

The parent's bytes are already in device memory and stay there (fz_batch_derive): the tables go up, one lane per output
measures and checks it, the lengths are scanned, the bytes are gathered.  The result is a ``BatchSequences``: pass it as
``sequences`` to find_near_matches_batch, find_near_matches_multi_batch and find_best_matches_batch, or derive from it again.
Cutting an adapter off where find_best_matches_batch found it is ``reads.derive(ends=...)``, the reads of one barcode
``reads.derive(index=mask)``, the reverse complement ``reads.derive(reverse=True, translate=DNA_COMPLEMENT)``.
"""
import numpy as np

from .batch import BatchSequences
from .engine import is_byteslike

__all__ = ['derive_batch', 'DerivedBatch', 'DNA_COMPLEMENT']


def _complement_table():
    table = bytearray(range(256))
    for a, b in ('AT', 'CG', 'RY', 'KM', 'BV', 'DH'):
        for x, y in ((a, b), (b, a)):
            table[ord(x)], table[ord(x.lower())] = ord(y), ord(y.lower())
    return bytes(table)


# A<->T, C<->G and the IUPAC pairs R<->Y, K<->M, B<->V, D<->H in both cases; S, W, N and every other byte map to themselves
DNA_COMPLEMENT = _complement_table()

# why an item is refused, in the library's words (fz_batch_derive)
_REASONS = {1: 'the index is not a sequence of the parent batch',
            2: 'the start lies behind the end',
            3: 'the end lies behind the end of the parent sequence'}


def _cut(s, a, b, reverse, translate):
    """X(s[a:b]) of one host-side sequence (bytes-like or a Contig: bytes; anything else: what its slice is)."""
    piece = s[a:b]
    if isinstance(piece, (bytes, bytearray, memoryview)) or is_byteslike(piece):
        piece = bytes(piece)
        if translate is not None:
            piece = piece.translate(translate)
    elif translate is not None:
        raise TypeError('translate takes a batch of bytes-like sequences, not of %s' % type(piece).__name__)
    return piece[::-1] if reverse else piece


class DerivedSequences(object):
    """The sequences of a DerivedBatch as a read-only sequence, cut from the parent's host-side sequences on demand."""

    def __init__(self, source, index, starts, ends, n_out, reverse, translate):
        self._source, self._index, self._starts, self._ends, self._n = source, index, starts, ends, n_out
        self._reverse, self._translate = reverse, translate

    def __len__(self):
        return self._n

    def _one(self, j):
        s = self._source[j if self._index is None else int(self._index[j])]
        a = None if self._starts is None else int(self._starts[j])
        b = None if self._ends is None else int(self._ends[j])
        return _cut(s, a, b, self._reverse, self._translate)

    def __getitem__(self, item):
        if isinstance(item, slice):
            return [self._one(j) for j in range(*item.indices(self._n))]
        j = item.__index__()
        if j < 0:
            j += self._n
        if not 0 <= j < self._n:
            raise IndexError('sequence index out of range')
        return self._one(j)

    def __iter__(self):
        return (self._one(j) for j in range(self._n))


def _table(name, values, n_out):
    """An optional table of n_out non-negative integers -> a uint64 array, or None."""
    if values is None:
        return None
    arr = np.asarray(values)
    if arr.ndim != 1:
        raise ValueError('%s is a flat array of one integer per output' % name)
    if arr.size == 0:
        arr = arr.astype(np.uint64)
    if np.issubdtype(arr.dtype, np.floating):
        # numpy promotes int64 with uint64 to float64 (where(best.pattern >= 0, best.start, reads.lengths)): whole numbers
        # that a double holds exactly are the integers they stand for, anything else is refused
        if not (np.isfinite(arr).all() and (arr == np.floor(arr)).all() and (np.abs(arr) < 2.0 ** 53).all()):
            raise TypeError('%s holds integers' % name)
        arr = arr.astype(np.int64)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise TypeError('%s holds integers' % name)
    if len(arr) != n_out:
        raise ValueError('%s has %d entries for %d outputs' % (name, len(arr), n_out))
    if arr.size and arr.min() < 0:
        raise ValueError('%s holds a negative value' % name)
    return np.ascontiguousarray(arr, dtype=np.uint64)


def _index(index, n_src):
    """index -> a uint32 array (a mask is resolved here; a value the C-ABI's type cannot hold is as bad as any other value
    beyond the parent, whose sequences number fewer than 2^32), or None."""
    if index is None:
        return None
    arr = np.asarray(index)
    if arr.ndim != 1:
        raise ValueError('index is a flat array of integers, or a mask of the parent batch')
    if arr.dtype == np.bool_:
        if len(arr) != n_src:
            raise ValueError('a mask of %d entries for a parent batch of %d sequences' % (len(arr), n_src))
        return np.flatnonzero(arr).astype(np.uint32)
    if arr.size == 0:
        return np.zeros(0, dtype=np.uint32)
    if not np.issubdtype(arr.dtype, np.integer):
        raise TypeError('index holds integers, or is a mask of the parent batch')
    if arr.min() < 0:
        raise ValueError('index holds a negative value')
    return np.minimum(arr, 0xffffffff).astype(np.uint32)


def _translate(translate, kind):
    if translate is None:
        return None
    if kind == 'str':
        raise TypeError('translate takes a batch of bytes-like sequences, not of str')
    table = bytes(memoryview(translate))                # TypeError for anything that is not bytes-like
    if len(table) != 256:
        raise ValueError('translate is a table of 256 bytes')
    return table


def _host_check(source, index, starts, ends, n_out):
    """The item rule in plain Python: the smallest bad j raises what the device's verdict raises."""
    n_src = len(source)
    for j in range(n_out):
        i = j if index is None else int(index[j])
        if i >= n_src:
            raise IndexError('derive: item %d: %s' % (j, _REASONS[1]))
        n = len(source[i])
        a = 0 if starts is None else int(starts[j])
        b = n if ends is None else int(ends[j])
        if a > b:
            raise ValueError('derive: item %d: %s' % (j, _REASONS[2]))
        if b > n:
            raise ValueError('derive: item %d: %s' % (j, _REASONS[3]))


class DerivedBatch(BatchSequences):
    """A BatchSequences made from another one (module docstring).  ``parent``; ``index``, ``starts``, ``lengths`` (numpy, one
    entry per sequence); ``sequences`` cuts ``X(parent.sequences[i][a:b])`` on demand, so only the parent's host-side
    sequences are needed afterwards: its device memory may be released."""

    def __init__(self, parent, index=None, starts=None, ends=None, reverse=False, translate=None):
        if not isinstance(parent, BatchSequences):
            raise TypeError('derive_batch takes a resident batch (resident_batch, resident_records, resident_fasta, a derived '
                            'batch), not %s' % type(parent).__name__)
        if parent.released:
            raise ValueError('the parent batch has been released')
        n_src = len(parent)
        self._idx = _index(index, n_src)
        n_out = n_src if self._idx is None else len(self._idx)
        self._starts = _table('starts', starts, n_out)
        self._ends = _table('ends', ends, n_out)
        self.reverse = bool(reverse)
        self.translate = _translate(translate, parent.kind)
        self.parent = parent
        self.engine = parent.engine
        self.handle = None
        self.kind = None
        self._n = n_out
        self._lengths = None
        view = DerivedSequences(parent.sequences, self._idx, self._starts, self._ends, n_out, self.reverse, self.translate)
        if parent.handle is not None:
            self.handle = self.engine.derive_batch(parent.handle, self._idx, self._starts, self._ends, n_out, self.reverse, self.translate)
            self.kind = parent.kind
            self.sequences = view
        else:                                       # the batched call does not serve this parent: plain Python, every search loops
            _host_check(parent.sequences, self._idx, self._starts, self._ends, n_out)
            self.sequences = list(view)

    def __len__(self):
        return self._n

    @property
    def index(self):
        return np.arange(self._n, dtype=np.uint32) if self._idx is None else self._idx

    @property
    def starts(self):
        return np.zeros(self._n, dtype=np.uint64) if self._starts is None else self._starts

    @property
    def lengths(self):
        if self._lengths is None:
            if self.handle is not None:
                _src, ends = self.engine.batch_tables(self.handle)
                self._lengths = ends.copy()
                if len(ends) > 1:
                    self._lengths[1:] -= ends[:-1]
            else:
                self._lengths = np.fromiter(map(len, self.sequences), dtype=np.uint64, count=self._n)
        return self._lengths


def derive_batch(sequences, index=None, starts=None, ends=None, reverse=False, translate=None):
    """``out[j] = X(sequences[index[j]][starts[j]:ends[j]])`` -> a DerivedBatch, made on the device when ``sequences`` is
    resident there (module docstring).  ``index``: integers, or a boolean mask of ``len(sequences)``; ``starts`` / ``ends``:
    one non-negative integer per output (whole-numbered floats, which numpy makes of int64 mixed with uint64, count as integers);
    ``translate``: 256 bytes (``DNA_COMPLEMENT``); each may be None for its default."""
    return DerivedBatch(sequences, index, starts, ends, reverse, translate)
