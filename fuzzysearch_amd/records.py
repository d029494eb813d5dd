"""resident_records: a FASTQ file, or a file with one read / barcode / guide per line, becomes a batch on the device.

The text crosses PCIe once and is split where it lies (fz_batch_upload_records: newlines counted and ranked, one line kept
per record, the lengths scanned, the sequences gathered), so no Python object per read is ever made.  The result is a
``BatchSequences``: pass it as ``sequences`` to find_near_matches_batch, find_near_matches_multi_batch and
find_best_matches_batch.

What a line is: it ends at ``\\n`` or, the last one, at the end of the text; one ``\\r`` in front of that end is not content.

``format='lines'``   every line is a sequence, empty lines included.
``format='fastq'``   four lines per record, the sequence on the second; trailing empty lines are ignored.  Checked: the
                     line count is a multiple of 4, the first line starts with ``@``, the third with ``+``, the fourth is as
                     long as the second.  The first malformed record raises ``ValueError`` naming it.

``lines=(0, 1, 3)`` keeps several lines of every record — a FASTQ file's headers, bases and qualities — as one RecordBatch each,
from ONE upload of the text and one line table (fz_batch_upload_records_lines): what ``format_records`` (egress.py) takes to
write the file back.  The FASTQ checks are the same whichever lines are kept.

Not understood: FASTQ records whose sequence spans several lines and compressed files — decompress and pass the bytes.
FASTA (newlines inside a sequence have to be removed, which is another gather) is ``resident_fasta``'s (fasta.py).
"""
import mmap
import os

import numpy as np

from . import _native
from .batch import BatchSequences, _single_device

__all__ = ['resident_records', 'RecordBatch', 'split_records']

# why a record is refused: the reasons of fz_batch_upload_records (1-4) and fz_batch_upload_fasta (5-7), in the library's words
_REASONS = {1: 'the number of lines is not a multiple of 4 (truncated record)',
            2: "the header line does not start with '@'",
            3: "the separator line does not start with '+'",
            4: 'the quality line is not as long as the sequence line',
            5: "the text does not start with '>'",
            6: 'an empty line inside the sequence',
            7: 'the sequence lines are not of one length and width (all but the last, which may be shorter)'}


class RecordSequences(object):
    """The sequences of a RecordBatch as a read-only sequence of ``bytes``, cut from the source on demand."""

    def __init__(self, source, starts, lengths):
        self._source, self._starts, self._lengths = source, starts, lengths

    def __len__(self):
        return len(self._starts)

    def _one(self, j):
        s = int(self._starts[j])
        return bytes(self._source[s:s + int(self._lengths[j])])

    def __getitem__(self, item):
        if isinstance(item, slice):
            return [self._one(j) for j in range(*item.indices(len(self)))]
        j = item.__index__()
        if j < 0:
            j += len(self)
        if not 0 <= j < len(self):
            raise IndexError('sequence index out of range')
        return self._one(j)

    def __iter__(self):
        return (self._one(j) for j in range(len(self)))


class RecordBatch(BatchSequences):
    """A BatchSequences made from a text of records.  ``starts[j]`` = offset of sequence j's first byte in the source,
    ``lengths[j]`` its length (numpy uint64); ``sequences`` cuts ``bytes`` from the source, which is kept alive, on demand.
    ``line``: the line of every record that the sequences are."""

    def __init__(self, source, format='fastq', engine=None):
        if format not in _native.RECORD_FORMATS:
            raise ValueError('unknown record format %r (known: %s)' % (format, ', '.join(sorted(_native.RECORD_FORMATS))))
        self.format = format
        self.line = _native.RECORD_FORMATS[format][1]
        self.source = _open_source(source)
        self.engine = engine or _native.default_engine()
        self.handle = None
        self.kind = None
        if _single_device(self.engine):
            self.handle = self.engine.upload_records(self.source, *_native.RECORD_FORMATS[format])
            self.kind = 'bytes'
            self.starts, ends = self.engine.batch_tables(self.handle)
            self.lengths = ends.copy()
            if len(ends) > 1:
                self.lengths[1:] -= ends[:-1]
            self.sequences = RecordSequences(self.source, self.starts, self.lengths)
        else:                                       # the batched call does not serve this engine: every search loops
            self.starts, self.lengths = split_records(self.source, format)
            view = RecordSequences(self.source, self.starts, self.lengths)
            self.sequences = list(view)

    @classmethod
    def _of_line(cls, source, format, engine, line, handle):
        """The batch of one kept line of a several-line upload (handle: its batch handle; None: split on the host)."""
        self = cls.__new__(cls)
        self.format, self.line, self.source, self.engine, self.handle, self.kind = format, line, source, engine, handle, None
        if handle is not None:
            self.kind = 'bytes'
            self.starts, ends = engine.batch_tables(handle)
            self.lengths = ends.copy()
            if len(ends) > 1:
                self.lengths[1:] -= ends[:-1]
            self.sequences = RecordSequences(source, self.starts, self.lengths)
        else:
            self.starts, self.lengths = split_records(source, format, line)
            self.sequences = list(RecordSequences(source, self.starts, self.lengths))
        return self


def _kept_lines(format, lines):
    period = _native.RECORD_FORMATS[format][0]
    kept = [l.__index__() for l in lines]
    if not 1 <= len(kept) <= period:
        raise ValueError('between 1 and %d lines of a %s record are kept, not %d' % (period, format, len(kept)))
    for l in kept:
        if not 0 <= l < period:
            raise ValueError('a %s record has the lines 0 .. %d, not %d' % (format, period - 1, l))
    if len(set(kept)) != len(kept):
        raise ValueError('a line is kept twice')
    return kept


def resident_records(source, format='fastq', engine=None, lines=None):
    """``source`` (bytes-like, or the path of a file, which is mapped read-only) -> a RecordBatch: its sequences resident in
    device memory, usable as ``sequences`` of the batch searches.  ``format``: 'fastq' or 'lines' (module docstring).
    ``lines``: several lines of every record, e.g. ``(0, 1, 3)`` of a FASTQ file -> a tuple of RecordBatch, one per entry in
    that order, from one upload; they share the one source object."""
    if lines is None:
        return RecordBatch(source, format, engine)
    if format not in _native.RECORD_FORMATS:
        raise ValueError('unknown record format %r (known: %s)' % (format, ', '.join(sorted(_native.RECORD_FORMATS))))
    kept = _kept_lines(format, lines)
    source = _open_source(source)
    engine = engine or _native.default_engine()
    if _single_device(engine):
        period, _line, flags = _native.RECORD_FORMATS[format]
        handles = engine.upload_records_lines(source, period, kept, flags)
    else:                                           # the batched call does not serve this engine: split in plain Python
        handles = [None] * len(kept)
    return tuple(RecordBatch._of_line(source, format, engine, l, h) for l, h in zip(kept, handles))


def _open_source(source):
    if isinstance(source, str) and ('\n' in source or '\r' in source):
        raise TypeError('the text of a file is passed as bytes, a str is a path')
    if isinstance(source, (str, os.PathLike)):
        with open(source, 'rb') as f:
            if os.fstat(f.fileno()).st_size == 0:
                return b''
            return mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    mv = memoryview(source)                         # TypeError for anything that is not bytes-like
    if mv.itemsize != 1 or mv.ndim != 1 or not mv.c_contiguous:
        raise TypeError('only contiguous sequences of single-byte values are supported')
    return source


def _line_spans(data, trim=True):
    """The lines of ``data`` (bytes) as a list of (start, content length, width): the content leaves out one ``\\r`` in front
    of the line's end, the width reaches to the next line's first byte.  ``trim``: trailing empty lines are no lines."""
    lines = data.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    spans, pos = [], 0
    for ln in lines:
        spans.append((pos, len(ln) - (1 if ln.endswith(b'\r') else 0), min(len(ln) + 1, len(data) - pos)))
        pos += len(ln) + 1
    while trim and spans and spans[-1][1] == 0:
        spans.pop()
    return spans


def _refuse(format, bad):
    """``bad``: (record, reason) pairs; the smallest one is the one reported, in the library's words."""
    if bad:
        r, why = min(bad)
        raise ValueError('%s: record %d: %s' % (format, r, _REASONS[why]))


def split_records(source, format, line=None):
    """The split on the host, in plain Python (engines the batched call does not serve) -> (starts, lengths) of line ``line``
    of every record (None: the format's sequence line)."""
    period, phase, flags = _native.RECORD_FORMATS[format]
    if line is not None:
        phase = line
    data = bytes(source)
    spans = [(s, n) for s, n, _w in _line_spans(data, trim=bool(flags & _native.REC_FASTQ_CHECKS))]
    if flags & _native.REC_FASTQ_CHECKS:
        bad = []
        if len(spans) % 4:
            bad.append((len(spans) // 4, 1))
        for r in range(len(spans) // 4):
            (h, hl), (s, sl), (p, pl), (q, ql) = spans[4 * r:4 * r + 4]
            if not hl or data[h:h + 1] != b'@':
                bad.append((r, 2))
            elif not pl or data[p:p + 1] != b'+':
                bad.append((r, 3))
            elif ql != sl:
                bad.append((r, 4))
            if bad and bad[-1][0] == r:
                break
        _refuse(format, bad)
    kept = spans[phase::period]
    starts = np.fromiter((s for s, _ in kept), dtype=np.uint64, count=len(kept))
    lengths = np.fromiter((n for _, n in kept), dtype=np.uint64, count=len(kept))
    return starts, lengths
