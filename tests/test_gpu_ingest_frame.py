"""-m gpu: the frame the three batch uploads share (fz_batch_upload, fz_batch_upload_records, fz_batch_upload_fasta: one
admission, one line-table stage, one handle builder with one table layout).  The uploads in turn on one engine, with refusals
between them; one set of reads through all three makers; the timing spans of the text uploads."""
import math
import random

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import fasta_model as fm
from tests import records_model as rm

pytestmark = pytest.mark.gpu

TILE = 16384
FORMATS = _native.RECORD_FORMATS


def dna(rnd, n):
    return bytes(rnd.choice(b'ACGT') for _ in range(n))


def one_tile_texts():
    """-> (FASTQ, lines, FASTA): each packs to TILE + 3 bytes."""
    rnd = random.Random(TILE + 3)
    reads = [dna(rnd, 150) for _ in range(109)] + [dna(rnd, 37)]
    contigs = [dna(rnd, 16000), b'', dna(rnd, 387)]
    assert sum(map(len, reads)) == sum(map(len, contigs)) == TILE + 3
    return rm.fastq(reads), b''.join(r + b'\n' for r in reads), fm.fasta(contigs)


FASTQ, LINES, FASTA = one_tile_texts()
BAD_FASTQ = b'@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIII\n'                 # record 1: reason 4, a short quality line
BAD_FASTA = b'>a\nAC\n>b\nACGT\nAC\nACGT\n'                         # record 1: reason 7, a short line in the middle


def check_plain(engine, rnd):
    lengths = [0, 1, TILE - 1, 0, 6]                                # packed: TILE + 6 bytes; sequence 2 fills tile 0 to its last byte
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(lengths, out=offs[1:])
    blob = dna(rnd, int(offs[-1]))
    h = engine.upload_batch(blob, offs)
    try:
        assert h.n_seqs == 5 and len(h) == TILE + 6
        starts, ends = engine.batch_tables(h)
        assert np.array_equal(starts, offs[:-1]) and np.array_equal(ends, offs[1:])
        assert engine.batch_bytes(h) == blob
    finally:
        h.release()


def check_records(engine, text, fmt):
    starts, ends, packed, n_lines = rm.tables(text, fmt)
    h = engine.upload_records(text, *FORMATS[fmt])
    try:
        assert h.info['n_lines'] == n_lines and h.n_seqs == len(starts) and h.info['packed_bytes'] == len(packed) == len(h) == TILE + 3
        g_starts, g_ends = engine.batch_tables(h)
        assert np.array_equal(g_starts, starts) and np.array_equal(g_ends, ends)
        assert engine.batch_bytes(h) == packed
    finally:
        h.release()


def check_fasta(engine, text):
    rows, seqs = fm.model(text)
    packed = b''.join(seqs)
    h = engine.upload_fasta(text)
    try:
        assert h.n_seqs == len(rows) and h.info['packed_bytes'] == len(packed) == len(h) == TILE + 3
        starts, ends = engine.batch_tables(h)
        assert starts.tolist() == [r[3] for r in rows] and ends.tolist() == fm.ends_of(seqs)
        assert [tuple(int(r[f]) for f in fm.FIELDS) for r in engine.fasta_index(h)] == rows
        assert engine.batch_bytes(h) == packed
    finally:
        h.release()


def refused(upload, record, reason):
    with pytest.raises(ValueError, match="record %d:" % record) as e:
        upload().release()
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (record, reason)


def test_lifecycle_across_the_three_uploads(engine):
    """Every upload after every other one, released in between (the released buffer is the next upload's), a refusal
    before two of them; then the three empty inputs."""
    rnd = random.Random(3)
    for _round in range(2):
        check_plain(engine, rnd)
        refused(lambda: engine.upload_records(BAD_FASTQ, *FORMATS['fastq']), 1, 4)
        check_records(engine, FASTQ, 'fastq')
        check_records(engine, LINES, 'lines')
        refused(lambda: engine.upload_fasta(BAD_FASTA), 1, 7)
        check_fasta(engine, FASTA)
    for upload in (lambda: engine.upload_records(b'', *FORMATS['fastq']), lambda: engine.upload_records(b'', *FORMATS['lines']),
                   lambda: engine.upload_fasta(b''), lambda: engine.upload_batch(b'', np.zeros(1, dtype=np.uint64))):
        h = upload()
        try:
            assert h.n_seqs == 0 and len(h) == 0
            starts, ends = engine.batch_tables(h)
            assert len(starts) == 0 and len(ends) == 0 and engine.batch_bytes(h) == b''
        finally:
            h.release()


def test_one_handle_from_three_makers(engine):
    """The same five reads as a packed batch, as FASTQ and as FASTA of one line per contig: one handle, whoever made it."""
    rnd = random.Random(5)
    pattern = dna(rnd, 20)
    reads = [dna(rnd, n) for n in (150, 1, 149, 151, 150)]
    reads[-1] = reads[-1][:60] + pattern + reads[-1][80:]             # the planted match
    held = []
    try:
        held.append(fa.resident_batch(reads, engine=engine))
        held.append(fa.resident_records(rm.fastq(reads), engine=engine))
        held.append(fa.resident_fasta(fm.fasta(reads, width=151), engine=engine))
        tables = [engine.batch_tables(h.handle)[1].tolist() for h in held]
        assert tables[0] == tables[1] == tables[2] == np.cumsum([len(r) for r in reads]).tolist()
        assert [engine.batch_bytes(h.handle) for h in held] == [b''.join(reads)] * 3
        found = [[[(m.start, m.end, m.dist, bytes(m.matched)) for m in per] for per in fa.find_near_matches_batch(pattern, h, max_l_dist=1)]
                 for h in held]
        assert found[0] == found[1] == found[2]
        assert (60, 80, 0, pattern) in found[0][-1] and len(found[0]) == 5
    finally:
        for h in held:
            h.release()


def test_timing_spans(engine):
    """records_ms() after each text upload: with the events on, a copy, kernels and a call that took time; with them off,
    the call still did."""
    try:
        for upload in (lambda: engine.upload_records(FASTQ, *FORMATS['fastq']), lambda: engine.upload_fasta(FASTA)):
            engine.set_timing(True)
            upload().release()
            ms = engine.records_ms()
            assert sorted(ms) == ['call', 'ends_d2h', 'h2d', 'kernels'] and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
            assert ms['h2d'] > 0 and ms['kernels'] > 0 and ms['call'] > 0, ms
            engine.set_timing(False)
            upload().release()
            assert engine.records_ms()['call'] > 0
    finally:
        engine.set_timing(True)                                     # the session engine's setting
