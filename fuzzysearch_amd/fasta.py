"""resident_fasta: the contigs of a FASTA file become a batch on the device.

The text crosses PCIe once and is split where it lies (fz_batch_upload_fasta: newlines counted and ranked, headers flagged
and ranked, one lane per contig measures it, one lane per line checks it, the lengths scanned, the bases gathered without
their newlines), so nothing is stripped, joined or upper-cased in Python.  The result is a ``BatchSequences`` whose sequences
are the contigs: pass it as ``sequences`` to find_near_matches_batch, find_near_matches_multi_batch and
find_best_matches_batch, and the matches come back in the coordinates of their contig.

The format is the rule of ``samtools faidx``.  Lines are resident_records' (a line ends at ``\\n`` or, the last one, at the end
of the text; one ``\\r`` in front of that end is not content; trailing empty lines are dropped first).  A line whose first byte
is ``>`` is a header and starts a record; every other line is a sequence line of the record the nearest header above it
opened; a record without sequence lines is an empty contig.  Per record ``linebases`` is the content length of its first
sequence line, ``linewidth`` the distance from that line's first byte to the next line's first byte, ``offset`` the position
of its first base.  Refused with a ``ValueError`` that names the record, the smallest (record, reason) first: a text that
does not start with ``>``; an empty sequence line inside a record; a sequence line, not the record's last, whose content
length or width differs from ``linebases`` / ``linewidth``, or a last line longer than ``linebases``.

Sequence bytes pass through untouched (IUPAC letters, ``*``, ``-``, lower case); ``upper=True`` clears bit 5 of every byte in
``a..z`` as the bases are gathered, exactly ``bytes.upper()``.

Not understood: ``;`` comment lines, blank lines between records and compressed files — decompress and pass the bytes.
"""
import numpy as np

from . import _native
from .batch import BatchSequences, _single_device
from .records import RecordSequences, _line_spans, _open_source, _refuse

__all__ = ['resident_fasta', 'FastaBatch', 'split_fasta']

_LOOP_LINES = 64                                    # slices of at most this many lines are cut line by line


class _Names(RecordSequences):
    """The headers up to their first space or tab."""

    def _one(self, j):
        head = RecordSequences._one(self, j)
        for i, c in enumerate(head):
            if c in b' \t':
                return head[:i]
        return head


class Contig(object):
    """One contig as a read-only sequence of bytes that is never materialised: ``len()``, and slices (``bytes``) and items
    (``int``) cut from the source by the closed form base q -> offset + q // linebases * linewidth + q % linebases."""

    def __init__(self, source, length, offset, linebases, linewidth, upper):
        self._source, self._n, self._off, self._lb, self._lw, self._upper = source, length, offset, linebases, linewidth, upper

    def __len__(self):
        return self._n

    def _cut(self, a, b):
        """Bases a .. b - 1 (0 <= a < b <= len)."""
        src, off, lb, lw = self._source, self._off, self._lb, self._lw
        first, last = a // lb, (b - 1) // lb
        if last - first < _LOOP_LINES:
            parts = []
            for line in range(first, last + 1):
                lo, hi = max(a, line * lb), min(b, (line + 1) * lb)
                s = off + line * lw + (lo - line * lb)
                parts.append(bytes(src[s:s + (hi - lo)]))
            out = b''.join(parts)
        else:                                       # whole lines as rows of linewidth bytes, their terminators cut off
            lines = last + 1 - first
            span = np.frombuffer(src, dtype=np.uint8, count=(lines - 1) * lw + (b - 1) % lb + 1, offset=off + first * lw)
            rows = np.zeros(lines * lw, dtype=np.uint8)
            rows[:len(span)] = span
            out = rows.reshape(lines, lw)[:, :lb].tobytes()[a - first * lb:b - first * lb]
        return out.upper() if self._upper else out

    def __getitem__(self, item):
        if isinstance(item, slice):
            a, b, step = item.indices(self._n)
            if step == 1:
                return self._cut(a, b) if a < b else b''
            picked = range(a, b, step)
            if not picked:
                return b''
            lo = min(picked[0], picked[-1])
            chunk = self._cut(lo, max(picked[0], picked[-1]) + 1)
            return bytes(chunk[i - lo] for i in picked)
        q = item.__index__()
        if q < 0:
            q += self._n
        if not 0 <= q < self._n:
            raise IndexError('index out of range')
        return self._cut(q, q + 1)[0]

    def __bytes__(self):
        return self._cut(0, self._n) if self._n else b''

    def __repr__(self):
        return 'Contig(%d bases)' % self._n


class FastaSequences(object):
    """The contigs of a FastaBatch: ``sequences[c]`` is a Contig (lazy), a slice a list of them; iterating yields every
    contig's ``bytes`` in turn (one contig in memory at a time: what the per-sequence routes of the searches consume)."""

    def __init__(self, source, rows, upper):
        self._source, self._rows, self._upper = source, rows, upper

    def __len__(self):
        return len(self._rows)

    def _one(self, c):
        r = self._rows[c]
        return Contig(self._source, int(r['length']), int(r['offset']), int(r['linebases']), int(r['linewidth']), self._upper)

    def __getitem__(self, item):
        if isinstance(item, slice):
            return [self._one(c) for c in range(*item.indices(len(self)))]
        c = item.__index__()
        if c < 0:
            c += len(self)
        if not 0 <= c < len(self):
            raise IndexError('sequence index out of range')
        return self._one(c)

    def __iter__(self):
        return (bytes(self._one(c)) for c in range(len(self)))


class FastaBatch(BatchSequences):
    """A BatchSequences made from a FASTA text.  numpy uint64 columns, together a ``.fai``: ``lengths``, ``offsets``,
    ``linebases``, ``linewidths`` (``starts`` is ``offsets``); ``names`` / ``headers`` cut ``bytes`` from the source, which is
    kept alive, on demand.  The index comes from the device at its first use (fz_batch_fasta_index)."""

    def __init__(self, source, upper=False, engine=None):
        self.upper = bool(upper)
        self.source = _open_source(source)
        self.engine = engine or _native.default_engine()
        self.handle = None
        self.kind = None
        self._rows = None
        self._sequences = None
        if _single_device(self.engine):
            self.handle = self.engine.upload_fasta(self.source, _native.FA_UPPER if self.upper else 0)
            self.kind = 'bytes'
            self._n = self.handle.n_seqs
        else:                                       # the batched call does not serve this engine: every search loops
            self._rows, self._sequences = split_fasta(self.source, self.upper)
            self._n = len(self._rows)

    @property
    def index(self):
        """The rows (structured array: header_start, header_len, length, offset, linebases, linewidth)."""
        if self._rows is None:                      # (before release(): the rows live with the handle)
            self._rows = self.engine.fasta_index(self.handle)
        return self._rows

    @property
    def sequences(self):
        if self._sequences is None:
            self._sequences = FastaSequences(self.source, self.index, self.upper)
        return self._sequences

    def __len__(self):
        return self._n

    lengths = property(lambda self: self.index['length'])
    offsets = property(lambda self: self.index['offset'])
    starts = offsets
    linebases = property(lambda self: self.index['linebases'])
    linewidths = property(lambda self: self.index['linewidth'])
    headers = property(lambda self: RecordSequences(self.source, self.index['header_start'], self.index['header_len']))
    names = property(lambda self: _Names(self.source, self.index['header_start'], self.index['header_len']))

    def fai(self):
        """The index as the text of a ``.fai`` file: name, length, offset, linebases, linewidth per contig."""
        return b''.join(b'%s\t%d\t%d\t%d\t%d\n' % (name, r['length'], r['offset'], r['linebases'], r['linewidth'])
                        for name, r in zip(self.names, self.index))

    def locate(self, c, pos):
        """The offset in the source of base ``pos`` of contig ``c``."""
        r = self.index[c]
        if not 0 <= pos < int(r['length']):
            raise IndexError('position outside the contig')
        lb = int(r['linebases'])
        return int(r['offset']) + pos // lb * int(r['linewidth']) + pos % lb


def resident_fasta(source, upper=False, engine=None):
    """``source`` (bytes-like, or the path of a file, which is mapped read-only) -> a FastaBatch: its contigs resident in
    device memory, usable as ``sequences`` of the batch searches.  ``upper``: fold ``a..z`` to upper case (module docstring)."""
    return FastaBatch(source, upper, engine)


def split_fasta(source, upper=False):
    """The split on the host, in plain Python (engines the batched call does not serve) -> (rows, the contigs as a list)."""
    data = bytes(source)
    spans = _line_spans(data)                       # (start, content length, width)
    bad, records = [], []
    if spans and data[:1] != b'>':
        bad.append((0, 5))
    for s, n, w in spans:
        if data[s:s + 1] == b'>':
            records.append([(s, n, w)])
        elif records:
            records[-1].append((s, n, w))
    rows = np.zeros(len(records), dtype=_native.fasta_dtype())
    contigs = []
    for r, rec in enumerate(records):
        (hs, hn, hw), body = rec[0], rec[1:]
        rows[r]['header_start'], rows[r]['header_len'], rows[r]['offset'] = hs + 1, hn - 1, hs + hw
        if body:
            lb, lw = body[0][1], body[0][2]
            rows[r]['offset'], rows[r]['linebases'], rows[r]['linewidth'] = body[0][0], lb, lw
            if any(n == 0 for _s, n, _w in body):
                bad.append((r, 6))
            if any(n != lb or w != lw for _s, n, w in body[:-1]) or body[-1][1] > lb:
                bad.append((r, 7))
        contig = b''.join(data[s:s + n] for s, n, _w in body)
        rows[r]['length'] = len(contig)
        contigs.append(contig.upper() if upper else contig)
    _refuse('fasta', bad)
    return rows, contigs
