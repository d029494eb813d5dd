"""format_records / write_records: resident batches become the text of a file — FASTQ, FASTA, lines, TSV — on the device.

One rule, whose model is three lines of Python::

    text = b''.join(lit[0] + col[0][j] + lit[1] + col[1][j] + ... + col[C-1][j] + lit[C]   for j in range(n))

``col``: C resident batches (1 <= C <= 8) of ``n`` sequences each; ``lit``: C + 1 byte strings of at most 255 bytes.

``format='lines'``   one column; every sequence followed by ``\\n``.
``format='fastq'``   three columns — headers (with their ``@``), bases, qualities — as ``head\\nbases\\n+\\nquals\\n``; the bases
                     and the qualities of every record must be of one length.
``format='fasta'``   two columns — names, sequences — as ``>name\\nsequence\\n``, unwrapped.
``literals=(...)``   any other layout: ``(b'', b'\\t', b'\\n')`` is a TSV of two columns.

The columns are already in device memory (resident_batch, resident_records, resident_fasta, derive_batch) and stay there
(fz_batch_format): one lane per record measures and checks it, the lengths are scanned, the text is gathered by 16-byte
pieces of the destination from the columns' bytes and the literals, and ONE copy brings it to the host — into a numpy array,
into a buffer of the caller's, or (``write_records``) straight into the mapping of the file.  No Python object per read is made.
The smallest bad record raises ``ValueError`` naming it, nothing is written, and the next call works.  Columns without a
device handle (engines the batched calls do not serve) are joined in plain Python by the same rule, with the same errors.
"""
import mmap
import os

import numpy as np

from . import _native
from .batch import BatchSequences

__all__ = ['format_records', 'write_records', 'FORMATS']

FORMATS = _native.FORMAT_PRESETS

# why a record is refused, in the library's words (fz_batch_format)
_REASONS = {1: 'the two columns checked for equal length differ in length'}


def _layout(columns, format, literals):
    """-> (columns as a list, literals as a tuple of bytes, the pair of columns to check or None), checked."""
    if isinstance(columns, BatchSequences):
        columns = [columns]
    else:
        columns = list(columns)
    if (format is None) == (literals is None):
        raise TypeError('exactly one of format and literals is given')
    if not 1 <= len(columns) <= _native.FORMAT_MAX_COLUMNS:
        raise ValueError('between 1 and %d columns are formatted, not %d' % (_native.FORMAT_MAX_COLUMNS, len(columns)))
    for c in columns:
        if not isinstance(c, BatchSequences):
            raise TypeError('format_records takes resident batches (resident_batch, resident_records, resident_fasta, derived '
                            'batches), not %s' % type(c).__name__)
    equal = None
    if format is not None:
        if format not in FORMATS:
            raise ValueError('unknown format %r (known: %s)' % (format, ', '.join(sorted(FORMATS))))
        literals, equal = FORMATS[format]
        if len(columns) != len(literals) - 1:
            raise ValueError('format %r takes %d columns, not %d' % (format, len(literals) - 1, len(columns)))
    else:
        literals = tuple(bytes(memoryview(l)) for l in literals)        # TypeError for anything that is not bytes-like
        if len(literals) != len(columns) + 1:
            raise ValueError('%d columns take %d literals, not %d' % (len(columns), len(columns) + 1, len(literals)))
    for i, l in enumerate(literals):
        if len(l) > _native.FORMAT_MAX_LITERAL:
            raise ValueError('literal %d is longer than %d bytes' % (i, _native.FORMAT_MAX_LITERAL))
    for i, c in enumerate(columns):
        if c.released:
            raise ValueError('column %d has been released' % i)
        if len(c) != len(columns[0]):
            raise ValueError('column %d has %d sequences, column 0 has %d' % (i, len(c), len(columns[0])))
        if c.engine is not columns[0].engine:
            raise ValueError('column %d is resident on another engine than column 0' % i)
    resident = [c.handle is not None for c in columns]
    if any(resident):
        if not all(resident):
            raise ValueError('columns with and without a device handle cannot be formatted together')
        for i, c in enumerate(columns):
            if c.kind != 'bytes':
                raise TypeError('column %d is a batch of %s: a text is made of bytes-like sequences' % (i, c.kind))
    return columns, literals, equal


def _out_array(out, size):
    """The caller's buffer as a numpy uint8 array over it, or a new array of `size` bytes."""
    if out is None:
        return np.empty(size, dtype=np.uint8)
    mv = memoryview(out)
    if mv.itemsize != 1 or mv.ndim != 1 or not mv.c_contiguous:
        raise TypeError('out is a contiguous buffer of single bytes')
    if mv.readonly:
        raise ValueError('out is read-only')
    if mv.nbytes < size:
        raise ValueError('out holds %d bytes, the text has %d' % (mv.nbytes, size))
    return np.frombuffer(mv, dtype=np.uint8)


def _text_size(columns, literals):
    """The text's length, known before anything runs."""
    per_record = sum(len(l) for l in literals)
    if columns[0].handle is not None:
        return sum(len(c.handle) for c in columns) + len(columns[0]) * per_record
    return sum(sum(len(s) for s in c.sequences) for c in columns) + len(columns[0]) * per_record


def _host_join(columns, literals, equal):
    """The rule in plain Python: the smallest bad record raises what the device's verdict raises."""
    seqs = [c.sequences for c in columns]
    parts = []
    for j in range(len(columns[0])):
        row = [s[j] for s in seqs]
        row = [r.encode('latin-1') if isinstance(r, str) else bytes(r) for r in row]
        if equal is not None and len(row[equal[0]]) != len(row[equal[1]]):
            raise ValueError('format: record %d: %s' % (j, _REASONS[1]))
        parts.append(literals[0])
        for c, r in enumerate(row):
            parts += (r, literals[c + 1])
    return b''.join(parts)


def format_records(columns, format=None, literals=None, out=None):
    """The text of ``columns`` — a resident batch or a sequence of 1 to 8 of them — under ``format`` ('lines', 'fastq', 'fasta')
    or ``literals`` (module docstring) -> a numpy uint8 array of exactly the text.  ``out``: a writable C-contiguous byte
    buffer of at least the text's size (a numpy.memmap, a bytearray); its first bytes are filled and a view of them returned."""
    columns, literals, equal = _layout(columns, format, literals)
    if columns[0].handle is None:
        text = _host_join(columns, literals, equal)
        arr = _out_array(out, len(text))
        arr[:len(text)] = np.frombuffer(text, dtype=np.uint8)
        return arr[:len(text)]
    size = _text_size(columns, literals)
    arr = _out_array(out, size)
    return columns[0].engine.format_batch([c.handle for c in columns], literals, equal, arr)


def write_records(path, columns, format=None, literals=None):
    """format_records into the file ``path``: it is created at its final size, mapped, and the text copied from the device
    into the mapping -> the number of bytes written.  A text of 0 bytes makes an empty file."""
    columns, literals, equal = _layout(columns, format, literals)
    if columns[0].handle is None:
        text = _host_join(columns, literals, equal)
        with open(path, 'wb') as f:
            f.write(text)
        return len(text)
    size = _text_size(columns, literals)
    with open(path, 'w+b') as f:
        if size == 0:
            return 0
        f.truncate(size)
        m = mmap.mmap(f.fileno(), size)
    try:
        columns[0].engine.format_batch([c.handle for c in columns], literals, equal, np.frombuffer(m, dtype=np.uint8))
        m.flush()
    except BaseException:
        os.unlink(path)                                     # a refused text leaves no file (the mapping may outlive it)
        raise
    finally:
        try:
            m.close()
        except BufferError:                                 # a traceback still holds a view of the mapping: it goes with it
            pass
    return size
