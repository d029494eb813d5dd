"""-m gpu: a text of records split on the device (fz_batch_upload_records / Engine.upload_records / resident_records) against
the model of tests/records_model.py: the tables and the packed bytes exactly, at every seam of the tiles and of the scan,
the errors, and the handle against fz_batch_upload's for the same reads."""
import random

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from fuzzysearch_amd.batch import pack_sequences
from tests import records_model as rm

pytestmark = pytest.mark.gpu

TILE = 16384
FORMATS = _native.RECORD_FORMATS
LEV, SUBS, EXACT = _native.MODE_LEV, _native.MODE_SUBS, _native.MODE_EXACT


def check(engine, text, fmt, want=None):
    """upload_records(text) against the model (or `want` = starts, ends, packed, n_lines) -> the number of sequences."""
    starts, ends, packed, n_lines = want if want is not None else rm.tables(text, fmt)
    h = engine.upload_records(text, *FORMATS[fmt])
    try:
        assert h.info['n_lines'] == n_lines and h.n_seqs == len(starts) and h.info['packed_bytes'] == len(packed) == len(h)
        g_starts, g_ends = engine.batch_tables(h)
        assert np.array_equal(g_starts, starts), ("starts", fmt, len(text))
        assert np.array_equal(g_ends, ends), ("ends", fmt, len(text))
        assert engine.batch_bytes(h) == packed, ("packed bytes", fmt, len(text))
    finally:
        h.release()
    return len(starts)


def dna(rnd, n):
    return bytes(rnd.choice(b'ACGT') for _ in range(n))


@pytest.mark.parametrize("eol", [b'\n', b'\r\n'])
def test_tile_seams(engine, eol):
    """150-byte reads; the first header grows byte by byte over one record's length, so everything a record holds passes
    over the seam between tile 0 and tile 1.  What lay on the seam's two bytes is tallied from the model and asserted."""
    rnd = random.Random(16384)
    reads = [dna(rnd, 150) for _ in range(120)]
    record = len(rm.fastq(reads[:1], eol=eol))
    seen = set()
    for pad in range(record + 1):
        heads = [b'@' + b'h' * pad] + [b'@r%02d' % (r % 100) for r in range(1, len(reads))]
        text = rm.fastq(reads, heads=heads, eol=eol)
        starts, ends, packed, n_lines = want = rm.tables(text, 'fastq')
        check(engine, text, 'fastq', want)
        first, last = set(starts.tolist()), set((starts + 149).tolist())
        inside = set()
        for s in starts.tolist():
            if s < TILE - 1 and s + 149 > TILE:
                inside.add('seam inside a sequence')
        for side, at in (('last byte of tile 0', TILE - 1), ('first byte of tile 1', TILE)):
            if text[at:at + 1] == b'\n':
                seen.add(('newline', side))
            if text[at:at + 2] == b'\r\n':
                seen.add(('CR of a CRLF', side))
            if at in first:
                seen.add(('first byte of a sequence', side))
            if at in last:
                seen.add(('last byte of a sequence', side))
        seen |= inside
    sides = ('last byte of tile 0', 'first byte of tile 1')
    what = ['newline', 'first byte of a sequence', 'last byte of a sequence'] + (['CR of a CRLF'] if eol == b'\r\n' else [])
    assert seen >= {(w, s) for w in what for s in sides} | {'seam inside a sequence'}, seen


def test_long_sequences(engine):
    rnd = random.Random(40000)
    reads = [dna(rnd, 150) for _ in range(3)] + [dna(rnd, 40000)] + [dna(rnd, 150) for _ in range(3)]
    assert check(engine, rm.fastq(reads), 'fastq') == 7
    assert check(engine, rm.fastq(reads, eol=b'\r\n', final_eol=False), 'fastq') == 7
    assert check(engine, dna(rnd, 70000), 'lines') == 1          # one unterminated line of more than four tiles


def scan_seam_sizes():
    b = _native.scan_items()
    return [1, 63, 64, 65, b - 1, b, b + 1, 2 * b + 1, b * b + 3]


@pytest.mark.parametrize("n", scan_seam_sizes())
def test_scan_seams(engine, n):
    """'A\\n' n times: n sequences of one byte, n items to the scan of the lengths (the last size crosses the level above the
    workgroups' sums).  The model is numpy's."""
    text = b'A\n' * n
    want = (np.arange(n, dtype=np.uint64) * 2, np.arange(1, n + 1, dtype=np.uint64), b'A' * n, n)
    assert check(engine, text, 'lines', want) == n


def test_scan_seams_of_mixed_lengths(engine):
    """Lengths 0 .. 6 in a seeded order over more than two workgroups of the scan: ends[] is no arithmetic progression."""
    rnd = random.Random(1024)
    n = 2 * _native.scan_items() + 77
    lens = [rnd.randrange(7) for _ in range(n)]
    text = b''.join(b'ACGTAC'[:l] + b'\n' for l in lens)
    assert check(engine, text, 'lines') == n


def test_degenerate_texts(engine):
    assert check(engine, b'', 'lines') == 0 and check(engine, b'', 'fastq') == 0
    assert check(engine, b'\n' * 5000, 'lines') == 5000          # only newlines: 5000 empty sequences, nothing packed
    assert check(engine, b'\r\n' * 3, 'lines') == 3
    assert check(engine, b'\n\n\r\n', 'fastq') == 0             # only blank lines: no records
    assert check(engine, b'@one\nACGTACGT\n+\nIIIIIIII', 'fastq') == 1
    assert check(engine, b'@one\r\nACGTACGT\r\n+\r\nIIIIIIII\r', 'fastq') == 1
    # every sequence empty; the last record is not empty, or its quality line would be a trailing blank line (the model
    # drops those before it counts: test_records_host.py)
    text = b'@a\n\n+\n\n' * 700 + b'@z\nA\n+\nI\n'
    assert check(engine, text, 'fastq') == 701
    with pytest.raises(ValueError, match="record 699:"):
        engine.upload_records(b'@a\n\n+\n\n' * 700)
    h = fa.resident_records(b'', format='lines')
    assert len(h) == 0 and h.kind == 'bytes' and fa.find_near_matches_batch(b'ACGT', h, max_l_dist=1) == []
    h.release()


def damaged(n_records, damage, extra_lines=0):
    """FASTQ of 150-byte reads; damage = {record: reason}; extra_lines: lines of one more, truncated record."""
    rnd = random.Random(n_records)
    lines = []
    for r in range(n_records):
        rec = [b'@r%d' % r, dna(rnd, 150), b'+', b'I' * 150]
        why = damage.get(r)
        if why == rm.REASON_AT:
            rec[0] = b'r%d' % r
        elif why == rm.REASON_PLUS:
            rec[2] = b'-'
        elif why == rm.REASON_QUAL:
            rec[3] = b'I' * 149
        lines += rec
    lines += [b'@t', b'ACGT', b'+'][:extra_lines]
    return b''.join(l + b'\n' for l in lines)


@pytest.mark.parametrize("record", [2, 160])                     # in tile 0; in tile 3 (a record is 311 bytes)
@pytest.mark.parametrize("reason", [rm.REASON_COUNT, rm.REASON_AT, rm.REASON_PLUS, rm.REASON_QUAL])
def test_errors(engine, reason, record):
    if reason == rm.REASON_COUNT:
        text = damaged(record, {}, extra_lines=3)
    else:
        text = damaged(200, {record: reason})
    with pytest.raises(rm.Malformed) as m:
        rm.model(text, 'fastq')
    assert (m.value.record, m.value.reason) == (record, reason)
    with pytest.raises(ValueError) as e:
        engine.upload_records(text)
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (record, reason)
    assert 'fastq' in str(e.value) and 'record %d:' % record in str(e.value)
    assert check(engine, damaged(200, {}), 'fastq') == 200       # the engine goes on


@pytest.mark.parametrize("damage,first", [
    ({150: rm.REASON_AT, 7: rm.REASON_QUAL}, (7, rm.REASON_QUAL)),
    ({7: rm.REASON_PLUS, 150: rm.REASON_AT}, (7, rm.REASON_PLUS)),
    ({150: rm.REASON_QUAL, 151: rm.REASON_AT}, (150, rm.REASON_QUAL)),
])
def test_the_lower_bad_record_wins(engine, damage, first):
    for extra in (0, 2):                                         # ... also over the truncated record behind them
        text = damaged(200, damage, extra_lines=extra)
        with pytest.raises(ValueError) as e:
            engine.upload_records(text)
        assert (e.value.info['bad_record'], e.value.info['bad_reason']) == first
        with pytest.raises(ValueError, match="record %d:" % first[0]):
            fa.resident_records(text)


def planted_fastq(seed, n_reads, patterns):
    rnd = random.Random(seed)
    reads = []
    for _ in range(n_reads):
        read = bytearray(dna(rnd, rnd.randint(30, 300)))
        if rnd.random() < 0.5:
            p = bytearray(rnd.choice(patterns))
            for _ in range(rnd.randint(0, 2)):
                p[rnd.randrange(len(p))] = rnd.choice(b'ACGT')
            at = rnd.randint(0, len(read) - len(p))
            read[at:at + len(p)] = p
        reads.append(bytes(read))
    eols = [rnd.choice([b'\n', b'\n', b'\r\n']) for _ in range(4 * n_reads)]
    return rm.fastq(reads, eol=eols), reads


@pytest.fixture(scope="module")
def planted():
    rnd = random.Random(20)
    patterns = [dna(rnd, 20) for _ in range(6)]
    text, reads = planted_fastq(2026, 3000, patterns)
    assert rm.model(text, 'fastq')[1] == reads
    return text, reads, patterns


def test_the_handle_is_a_batch_handle(engine, planted):
    """batch_search, batch_search_multi and batch_assign over the record handle and over upload_batch of the model's reads:
    identical arrays."""
    text, reads, patterns = planted
    blob, offs = pack_sequences(reads, 'bytes')
    a, b = engine.upload_records(text), engine.upload_batch(blob, offs)
    try:
        assert a.n_seqs == b.n_seqs == len(reads) and len(a) == len(b)
        sa, ea = engine.batch_tables(a)
        sb, eb = engine.batch_tables(b)
        assert np.array_equal(ea, eb) and np.array_equal(eb, offs[1:]) and np.array_equal(sb, offs[:-1])
        rows = 0
        for mode, k, pats in ((LEV, 2, patterns), (SUBS, 2, patterns), (EXACT, 0, [p[:12] for p in patterns])):
            for reduced in (False, True):
                for p in pats[:2]:
                    ra, qa = engine.batch_search(a, mode, p, k, reduced=reduced)
                    rb, qb = engine.batch_search(b, mode, p, k, reduced=reduced)
                    assert np.array_equal(ra, rb) and np.array_equal(qa, qb), (mode, reduced)
                    rows += len(ra)
                if mode == EXACT:
                    continue
                for (ra, qa), (rb, qb) in zip(engine.batch_search_multi(a, mode, pats, k, reduced=reduced),
                                              engine.batch_search_multi(b, mode, pats, k, reduced=reduced)):
                    assert np.array_equal(ra, rb) and np.array_equal(qa, qb), (mode, reduced)
                    rows += len(ra)
            if mode != EXACT:
                ga, gb = engine.batch_assign(a, mode, pats, k), engine.batch_assign(b, mode, pats, k)
                assert np.array_equal(ga, gb) and int((ga['pattern'] >= 0).sum()) > len(reads) // 4
        assert rows > len(reads)
    finally:
        a.release()
        b.release()


def same_matches(a, b):
    return [[(m.start, m.end, m.dist, m.matched) for m in per] for per in a] == \
           [[(m.start, m.end, m.dist, m.matched) for m in per] for per in b]


def test_public_calls(engine, planted, tmp_path):
    text, reads, patterns = planted
    path = tmp_path / "reads.fastq"
    path.write_bytes(text)
    listed = fa.resident_batch(reads)
    for source in (text, str(path), path, bytearray(text), memoryview(text)):
        held = fa.resident_records(source)
        assert isinstance(held, fa.batch.BatchSequences) and held.kind == 'bytes' and len(held) == len(reads)
        assert held.starts.dtype == held.lengths.dtype == np.uint64
        assert held[5] == reads[5] and held.sequences[-1] == reads[-1] and held.sequences[10:13] == reads[10:13]
        best, want = fa.find_best_matches_batch(patterns, held, max_l_dist=2), fa.find_best_matches_batch(patterns, listed, max_l_dist=2)
        for name in ('pattern', 'dist', 'start', 'end', 'tied'):
            assert np.array_equal(getattr(best, name), getattr(want, name)), name
        assert int((best.pattern >= 0).sum()) > len(reads) // 4
        held.release()
    held = fa.resident_records(text)
    adapter = patterns[0]
    got = fa.find_near_matches_batch(adapter, held, max_l_dist=1)
    assert same_matches(got, fa.find_near_matches_batch(adapter, reads, max_l_dist=1)) and sum(map(len, got)) > 50
    assert all(m.matched == reads[j][m.start:m.end] for j, per in enumerate(got) for m in per)
    multi = fa.find_near_matches_multi_batch(patterns, held, max_l_dist=1)
    for per_pattern, want in zip(multi, fa.find_near_matches_multi_batch(patterns, reads, max_l_dist=1)):
        assert same_matches(per_pattern, want)
    # separate limits: the per-sequence loop, through the lazy view
    limits = dict(max_substitutions=1, max_insertions=1, max_deletions=0, max_l_dist=1)
    few = fa.resident_records(rm.fastq(reads[:200]))
    assert same_matches(fa.find_near_matches_batch(adapter, few, **limits), fa.find_near_matches_batch(adapter, reads[:200], **limits))
    few.release()
    # starts: the quality line is two lines on
    mv = memoryview(text)
    for j in range(0, len(reads), 97):
        s, n = int(held.starts[j]), int(held.lengths[j])
        assert bytes(mv[s:s + n]) == reads[j]
        after = text.index(b'\n', s + n) + 1                    # the '+' line
        q = text.index(b'\n', after) + 1
        assert text[after:after + 1] == b'+' and text[q:q + n] == b'I' * n and text[q + n:q + n + 1] in (b'\n', b'\r', b'')
    held.release()
    listed.release()
    lines = fa.resident_records(b'\n'.join(reads[:50]), format='lines')
    assert list(lines.sequences) == reads[:50]
    lines.release()
