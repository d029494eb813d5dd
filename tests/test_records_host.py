"""Records, the parts that need no GPU: the split of fz_batch_upload_records run on the host through the functions its kernels
run (fz_debug_records_split: fz_rec_line, fz_rec_measure, fz_rec_err_key of fz_device.h) against the model of
tests/records_model.py, the error order, and resident_records' plain-Python split for engines the batched call does not
serve."""
import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, records
from tests import records_model as rm

FORMATS = {'lines': (1, 0, 0), 'fastq': (4, 1, _native.REC_FASTQ_CHECKS)}
N_TEXTS = 10000


def check_against_model(text, fmt):
    """One text through both -> 'ok' / 'error'; asserts they agree."""
    try:
        starts, ends, packed, n_lines = rm.tables(text, fmt)
    except rm.Malformed as bad:
        with pytest.raises(ValueError) as e:
            _native.records_split(text, *FORMATS[fmt])
        assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (bad.record, bad.reason), text
        assert 'record %d' % bad.record in str(e.value) and fmt in str(e.value)
        return 'error'
    g_starts, g_ends, g_packed, info = _native.records_split(text, *FORMATS[fmt])
    assert info['n_lines'] == n_lines and info['n_seqs'] == len(starts) and info['bad_reason'] == 0, text
    assert info['packed_bytes'] == len(packed)
    assert np.array_equal(g_starts, starts) and np.array_equal(g_ends, ends) and g_packed == packed, text
    return 'ok'


def test_lines_split_matches_the_model_on_random_texts():
    rnd = rm.rng(20261)
    seen = set()
    for _ in range(N_TEXTS):
        text = rm.random_lines_text(rnd)
        assert check_against_model(text, 'lines') == 'ok'
        seen.add((text == b'', text.endswith(b'\n'), b'\r\n' in text, b'\n\n' in text or text.startswith(b'\n')))
    assert len(seen) >= 8                        # the empty text, with and without final terminator, CRLF, empty lines


def test_fastq_split_matches_the_model_on_random_texts():
    rnd = rm.rng(20262)
    outcomes = {'ok': 0, 'error': 0}
    for i in range(N_TEXTS):
        text = rm.random_fastq_text(rnd, break_it=(i % 4 == 3))
        outcomes[check_against_model(text, 'fastq')] += 1
    assert outcomes['ok'] >= N_TEXTS // 2 and outcomes['error'] >= N_TEXTS // 10


@pytest.mark.parametrize("text", [
    b'', b'\n', b'\r\n', b'\r', b'A', b'A\r', b'A\n', b'A\r\n', b'\n\n\n', b'A\n\nB', b'A\rB\n', b'\r\r\n', b'A\n\r', b'A\n\r\n\n',
])
def test_lines_corner_texts(text):
    assert check_against_model(text, 'lines') == 'ok'


@pytest.mark.parametrize("text", [
    b'', b'\n', b'\r\n\n', b'@a\nACGT\n+\nIIII', b'@a\nACGT\n+\nIIII\n', b'@a\r\nACGT\r\n+\r\nIIII\r\n', b'@a\nACGT\n+\nIIII\r',
    b'@a\nACGT\n+\n@+II\n', b'@a\nACGT\n+\n+@II\n\n\r\n\n', b'@a\n\n+\n\n@b\nA\n+\nI\n', b'@a\nA\rC\n+\nI\rI\n',
    b'@a\nACGT\r\n+\nIIII\n',
])
def test_fastq_corner_texts(text):
    assert check_against_model(text, 'fastq') == 'ok'


@pytest.mark.parametrize("text", [b'@a\n\n+\n\n@b\n\n+\n', b'@a\n\n+\n\n@b\n\n+\n\n', b'@a\n\n+\n\n'])
def test_an_empty_last_read_loses_its_quality_line_to_the_trailing_blank_lines(text):
    """The model drops trailing empty lines BEFORE it counts: the empty quality line of an empty last read is one of them, so
    such a file is a truncated record to the model, and to the split alike."""
    assert check_against_model(text, 'fastq') == 'error'


GOOD = [b'@h', b'ACGT', b'+', b'IIII']


def fastq_with(damage):
    """Three records; damage = {record: reason} -> text."""
    out = []
    for r in range(3):
        rec = list(GOOD)
        why = damage.get(r)
        if why == rm.REASON_AT:
            rec[0] = b'h'
        elif why == rm.REASON_PLUS:
            rec[2] = b''
        elif why == rm.REASON_QUAL:
            rec[3] = b'III'
        out += rec
    if damage.get(3) == rm.REASON_COUNT:
        out += [b'@h', b'AC']
    return b''.join(l + b'\n' for l in out)


@pytest.mark.parametrize("record,reason", [(3, rm.REASON_COUNT), (0, rm.REASON_AT), (1, rm.REASON_AT), (2, rm.REASON_PLUS),
                                           (0, rm.REASON_PLUS), (1, rm.REASON_QUAL), (2, rm.REASON_QUAL)])
def test_every_error_reason_on_its_own(record, reason):
    text = fastq_with({record: reason})
    with pytest.raises(rm.Malformed) as m:
        rm.model(text, 'fastq')
    assert (m.value.record, m.value.reason) == (record, reason)
    with pytest.raises(ValueError) as e:
        _native.records_split(text, *FORMATS['fastq'])
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (record, reason)
    assert 'fastq' in str(e.value) and 'record %d' % record in str(e.value)
    assert check_against_model(text, 'fastq') == 'error'


@pytest.mark.parametrize("damage,first", [
    ({2: rm.REASON_AT, 1: rm.REASON_QUAL}, (1, rm.REASON_QUAL)),
    ({0: rm.REASON_QUAL, 2: rm.REASON_AT}, (0, rm.REASON_QUAL)),
    ({3: rm.REASON_COUNT, 1: rm.REASON_PLUS}, (1, rm.REASON_PLUS)),
    ({3: rm.REASON_COUNT, 2: rm.REASON_AT}, (2, rm.REASON_AT)),
])
def test_the_smaller_record_and_reason_is_reported(damage, first):
    text = fastq_with(damage)
    with pytest.raises(ValueError) as e:
        _native.records_split(text, *FORMATS['fastq'])
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == first
    assert check_against_model(text, 'fastq') == 'error'


def test_a_record_with_two_faults_reports_the_smaller_reason():
    text = b'h\nACGT\n\nIII\n'                   # no '@', no '+', short quality
    with pytest.raises(ValueError) as e:
        _native.records_split(text, *FORMATS['fastq'])
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (0, rm.REASON_AT)
    assert check_against_model(text, 'fastq') == 'error'


def test_arguments_are_checked():
    for period, phase, flags in ((0, 0, 0), (4, 4, 0), (2, 1, _native.REC_FASTQ_CHECKS), (4, 1, 2)):
        with pytest.raises(ValueError):
            _native.records_split(b'A\n', period, phase, flags)
    starts, ends, packed, info = _native.records_split(b'a\nb\nc\nd\ne\nf\n', 4, 1, 0)     # the parameterised path without the checks
    assert starts.tolist() == [2, 10] and packed == b'bf' and info['n_lines'] == 6


def test_scan_items_is_exported():
    assert _native.scan_items() >= 64 and _native.scan_items() % 64 == 0


class SeveralDevices(object):
    """Stands in for an engine the batched call does not serve."""
    devices = [0, 1]

    def comm_info(self):
        return 0, 0, False

    def upload_records(self, *a):
        raise AssertionError("an engine of several devices uploads no records")


def test_host_fallback_returns_the_model_s_sequences(tmp_path):
    rnd = rm.rng(7)
    for fmt, gen in (('lines', rm.random_lines_text), ('fastq', rm.random_fastq_text)):
        for _ in range(300):
            text = gen(rnd)
            try:
                starts, reads, _n = rm.model(text, fmt)
            except rm.Malformed as bad:              # (an empty last read: see the test above)
                with pytest.raises(ValueError, match="record %d:" % bad.record):
                    fa.resident_records(text, format=fmt, engine=SeveralDevices())
                continue
            held = fa.resident_records(text, format=fmt, engine=SeveralDevices())
            assert held.handle is None and held.kind is None
            assert list(held.sequences) == reads and len(held) == len(reads)
            assert held.starts.tolist() == starts and held.lengths.tolist() == [len(r) for r in reads]
    text = rm.fastq([b'ACGT', b'', b'GG'])
    path = tmp_path / "reads.fastq"
    path.write_bytes(text)
    held = fa.resident_records(str(path), engine=SeveralDevices())
    assert list(held.sequences) == [b'ACGT', b'', b'GG'] and held[2] == b'GG'
    empty = tmp_path / "empty.fastq"
    empty.write_bytes(b'')
    assert len(fa.resident_records(empty, engine=SeveralDevices())) == 0
    with pytest.raises(ValueError, match="record 1"):
        fa.resident_records(fastq_with({1: rm.REASON_QUAL}), engine=SeveralDevices())


def test_resident_records_refuses_text_and_unknown_formats():
    with pytest.raises(TypeError):
        fa.resident_records('@a\nACGT\n+\nIIII\n', engine=SeveralDevices())
    with pytest.raises(ValueError, match="fasta"):
        fa.resident_records(b'>a\nACGT\n', format='fasta', engine=SeveralDevices())
    with pytest.raises(TypeError):
        fa.resident_records(12, engine=SeveralDevices())
    assert 'resident_records' in fa.__all__


def test_record_sequences_view_is_lazy_and_indexable():
    text = rm.fastq([b'ACGT', b'', b'GGA', b'T'], eol=b'\r\n')
    starts, reads, _n = rm.model(text, 'fastq')
    view = records.RecordSequences(text, np.array(starts, np.uint64), np.array([len(r) for r in reads], np.uint64))
    assert len(view) == 4 and bool(view) and list(view) == reads
    assert view[0] == b'ACGT' and view[-1] == b'T' and view[1:3] == reads[1:3] and view[::-1] == reads[::-1]
    assert type(view[2]) is bytes
    with pytest.raises(IndexError):
        view[4]
    assert not records.RecordSequences(b'', np.zeros(0, np.uint64), np.zeros(0, np.uint64))


# one minimal malformed text per reason of the library's table: FASTQ 1-4, FASTA 5-7
MINIMAL = [(1, 'fastq', b'@h\nAC\n'), (2, 'fastq', b'h\nAC\n+\nII\n'), (3, 'fastq', b'@h\nAC\n-\nII\n'), (4, 'fastq', b'@h\nAC\n+\nI\n'),
           (5, 'fasta', b'AC\n'), (6, 'fasta', b'>a\nAC\n\nAC\n'), (7, 'fasta', b'>a\nAC\nA\nAC\n')]


@pytest.mark.parametrize("reason,fmt,text", MINIMAL)
def test_the_python_splitters_refuse_in_the_library_s_words(reason, fmt, text):
    """records._REASONS restates the library's table: the host twin's message and the plain-Python splitter's are one text."""
    from fuzzysearch_amd import fasta
    with pytest.raises(ValueError) as native:
        _native.fasta_split(text) if fmt == 'fasta' else _native.records_split(text, *FORMATS[fmt])
    with pytest.raises(ValueError) as plain:
        fasta.split_fasta(text) if fmt == 'fasta' else records.split_records(text, fmt)
    assert (native.value.info['bad_record'], native.value.info['bad_reason']) == (0, reason)
    assert str(plain.value) == str(native.value) == '%s: record 0: %s' % (fmt, records._REASONS[reason])
    assert sorted(records._REASONS) == [r for r, _f, _t in MINIMAL] and not hasattr(fasta, '_REASONS')


@pytest.mark.parametrize("text", [b'a\nbc\n', b'a\r\nbc\r\n', b'a\nbc', b'a\r\nbc\r', b'a\n\nbc\n\n\r\n\n', b'\n', b''])
def test_line_spans_against_bytes_split(text):
    lines = text.split(b'\n')
    if lines[-1] == b'':                             # the text ended with a terminator (or is empty): no line behind it
        lines.pop()
    spans = records._line_spans(text, trim=False)
    assert len(spans) == len(lines)
    assert [text[s:s + n] for s, n, _w in spans] == [ln[:-1] if ln.endswith(b'\r') else ln for ln in lines]
    assert b''.join(text[s:s + w] for s, _n, w in spans) == text
    assert [s for s, _n, _w in spans] == [sum(len(ln) + 1 for ln in lines[:i]) for i in range(len(lines))]
    kept = len(lines)
    while kept and lines[kept - 1] in (b'', b'\r'):
        kept -= 1
    assert records._line_spans(text) == spans[:kept]
