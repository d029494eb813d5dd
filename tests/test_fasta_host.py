"""FASTA, the parts that need no GPU: the split of fz_batch_upload_fasta run on the host through the functions its kernels
run (fz_debug_fasta_split: fz_fa_measure, fz_fa_line_check, fz_fa_src, fz_fa_upper4 of fz_device.h) against the model of
tests/fasta_model.py, the error order, and the Python surface of resident_fasta over a recording fake engine."""
import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, fasta
from tests import fasta_model as fm

N_TEXTS = 2400


def rows_as_tuples(rows):
    return [tuple(int(r[f]) for f in fm.FIELDS) for r in rows]


def check_against_model(text, upper):
    """One text through both -> 'ok' or the (record, reason) both refuse it with; asserts they agree."""
    flags = _native.FA_UPPER if upper else 0
    try:
        rows, seqs = fm.model(text, upper)
    except fm.Malformed as bad:
        with pytest.raises(ValueError) as e:
            _native.fasta_split(text, flags)
        assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (bad.record, bad.reason), text
        assert 'record %d:' % bad.record in str(e.value) and 'fasta' in str(e.value)
        return bad.record, bad.reason
    g_rows, g_ends, g_packed, info = _native.fasta_split(text, flags)
    assert info['n_seqs'] == len(rows) and info['bad_reason'] == 0 and info['packed_bytes'] == sum(map(len, seqs)), text
    assert rows_as_tuples(g_rows) == rows, text
    assert g_ends.tolist() == fm.ends_of(seqs) and g_packed == b''.join(seqs), text
    return 'ok'


def test_split_matches_the_model_on_random_texts():
    rnd = fm.rng(20271)
    seen, reasons = set(), set()
    outcomes = {'ok': 0, 'error': 0}
    kinds = sorted(fm.DAMAGES)
    for i in range(N_TEXTS):
        upper = bool(i & 1)
        if i % 3 == 2:                               # a third malformed: every damage at the first, a middle and the last record
            what, where = kinds[(i // 3) % len(kinds)], ('first', 'middle', 'last')[(i // 3 // len(kinds)) % 3]
            text, done = fm.random_text(rnd, damage=[what], where=where)
            got = check_against_model(text, upper)
            if done:
                (record, what), = done.items()
                assert got == (record, fm.DAMAGES[what]), (text, done)
                reasons.add((fm.DAMAGES[what], where))
                outcomes['error'] += 1
            continue
        text, _ = fm.random_text(rnd)
        assert check_against_model(text, upper) == 'ok', text
        outcomes['ok'] += 1
        rows, seqs = fm.model(text)
        seen.add(('crlf', b'\r\n' in text))
        seen.add(('final newline', text.endswith(b'\n')))
        seen.add(('empty contig first', rows[0][2] == 0))
        seen.add(('empty contig last', rows[-1][2] == 0))
        seen.add(('empty contig in the middle', any(r[2] == 0 for r in rows[1:-1])))
        seen.add(('consecutive headers', any(a[2] == 0 and b[2] == 0 for a, b in zip(rows, rows[1:]))))
        seen.add(('lower case', any(s != s.upper() for s in seqs)))
    assert outcomes['ok'] >= N_TEXTS // 2 and outcomes['error'] >= N_TEXTS // 5, outcomes
    assert seen >= {(k, v) for k in ('crlf', 'final newline', 'empty contig first', 'empty contig last', 'empty contig in the middle',
                                     'consecutive headers') for v in (False, True)} | {('lower case', True)}, seen
    assert reasons >= {(why, where) for why in (fm.REASON_EMPTY, fm.REASON_WIDTH) for where in ('first', 'middle', 'last')} | \
        {(fm.REASON_START, 'first')}, reasons


def test_two_errors_in_one_text_report_the_smallest_record_and_reason():
    rnd = fm.rng(20272)
    n = 0
    for i in range(600):
        a, b = rnd.sample(sorted(set(fm.DAMAGES) - {'no_start'}), 2)
        text, done = fm.random_text(rnd, damage=[a, b], where=[2, 1] if i & 1 else [0, 2])
        got = check_against_model(text, False)
        if len(done) == 2:
            first = min(done)
            assert got == (first, fm.DAMAGES[done[first]]), (text, done)
            n += 1
    assert n >= 300
    # ... and the smaller reason of one record: an empty line is also a line of another length
    assert check_against_model(b'>a\nAC\n\nGT\n', False) == (0, fm.REASON_EMPTY)
    assert check_against_model(b'>a\nAC\nA\nGT\n>b\nAC\n\nGT\n', False) == (0, fm.REASON_WIDTH)
    assert check_against_model(b'x\n>a\nAC\n\nGT\n', False) == (0, fm.REASON_START)


@pytest.mark.parametrize("text", [
    b'', b'\n', b'\r\n\n', b'>', b'>\n', b'>a', b'>a\n', b'>a\r\n', b'>a\nA', b'>a\nA\r', b'>a\nA\r\n', b'>a\n>b\n', b'>a\n>b\nAC\n>c',
    b'>a\nACGT\nAC\n', b'>a\nACGT\nACGT\n', b'>a\r\nACGT\r\nAC', b'>a\nAC\n\n\n', b'>a\nA>C\n>b x\ty\nAC\rGT\nA\n', b'>a\nAC\r\r\nAC\r\r\n',
])
def test_corner_texts_that_are_well_formed(text):
    assert check_against_model(text, False) == 'ok' and check_against_model(text, True) == 'ok'


@pytest.mark.parametrize("text,first", fm.MALFORMED)
def test_corner_texts_that_are_malformed(text, first):
    assert check_against_model(text, False) == first


def test_upper4_on_every_byte_in_every_lane():
    for lane in range(4):
        for other in (0x00, 0x61, 0x7a, 0xff):
            for v in range(256):
                word = bytes(v if i == lane else other for i in range(4))
                got = _native.fasta_upper4(int.from_bytes(word, 'little')).to_bytes(4, 'little')
                assert got == word.upper(), (word, got)


@pytest.mark.parametrize("width", [1, 15, 16, 17, 60, 61])
@pytest.mark.parametrize("eol", [b'\n', b'\r\n'])
def test_src_against_the_model_s_position_map(width, eol):
    rnd = fm.rng(width)
    contigs = [fm.random_contig(rnd, n) for n in (3 * width + 1, 0, 4 * width, 1, 2 * width - 1 if width > 1 else 1)]
    text = fm.fasta(contigs, width=width, eol=eol, final_eol=bool(width & 1))
    rows, seqs = fm.model(text)
    assert seqs == contigs
    for (_hs, _hl, length, offset, lb, lw), where in zip(rows, fm.position_map(text)):
        assert len(where) == length
        assert [_native.fasta_src(offset, lb, lw, q) for q in range(length)] == where
    big = 1 << 33                                    # past 32 bits: the 64-bit division
    assert _native.fasta_src(7, 60, 61, big) == 7 + big // 60 * 61 + big % 60
    assert _native.fasta_src(7, big + 1, big + 2, big + 5) == 7 + big + 2 + 4


def test_arguments_are_checked():
    with pytest.raises(ValueError):
        _native.fasta_split(b'>a\nA\n', 2)
    assert {"fz_batch_upload_fasta", "fz_batch_fasta_index", "fz_debug_fasta_split"} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.fasta_dtype().itemsize == 48 and _native.fasta_dtype().names == fm.FIELDS


class Recording(object):
    """Stands in for an engine of one device: upload_fasta and fasta_index answer from the host split and are recorded."""
    devices = [0]

    def __init__(self):
        self.log = []

    def comm_info(self):
        return 0, 0, False

    def upload_fasta(self, text, flags=0):
        self.log.append(('upload_fasta', flags))
        rows, _ends, _packed, info = _native.fasta_split(text, flags)
        handle = type('Handle', (), {})()
        handle.n_seqs, handle.info, handle.rows, handle.release = info['n_seqs'], info, rows, lambda: None
        return handle

    def fasta_index(self, handle):
        self.log.append(('fasta_index',))
        return handle.rows


class SeveralDevices(object):
    """Stands in for an engine the batched call does not serve."""
    devices = [0, 1]

    def comm_info(self):
        return 0, 0, False

    def upload_fasta(self, *a):
        raise AssertionError("an engine of several devices uploads no FASTA")


TEXT = fm.fasta([b'ACGTacgtNNryAC', b'', b'acgtACG', b'T' * 300], width=7, eol=b'\r\n',
                heads=[b'>chr1 first contig', b'>empty', b'>chr3\ttabbed', b'>chrLong'])


def test_the_surface_over_a_recording_engine(tmp_path):
    path = tmp_path / "small.fa"
    path.write_bytes(TEXT)
    for upper in (False, True):
        rows, seqs = fm.model(TEXT, upper)
        for source in (TEXT, str(path), path, bytearray(TEXT), memoryview(TEXT)):
            eng = Recording()
            held = fa.resident_fasta(source, upper=upper, engine=eng)
            assert isinstance(held, fa.FastaBatch) and isinstance(held, fa.batch.BatchSequences) and held.kind == 'bytes'
            assert eng.log == [('upload_fasta', _native.FA_UPPER if upper else 0)] and len(held) == 4
            assert eng.log == [('upload_fasta', _native.FA_UPPER if upper else 0)]          # the index has not come back yet
            assert held.lengths.tolist() == [r[2] for r in rows] and held.offsets.tolist() == [r[3] for r in rows]
            assert held.linebases.tolist() == [r[4] for r in rows] and held.linewidths.tolist() == [r[5] for r in rows]
            assert held.starts.tolist() == held.offsets.tolist() and held.lengths.dtype == np.uint64
            assert eng.log.count(('fasta_index',)) == 1                                     # ... and comes back once
            assert list(held.names) == [b'chr1', b'empty', b'chr3', b'chrLong'] and held.names[-1] == b'chrLong'
            assert list(held.headers) == [b'chr1 first contig', b'empty', b'chr3\ttabbed', b'chrLong']
            assert held.fai() == fm.fai(TEXT) and held.fai().startswith(b'chr1\t14\t20\t7\t9\n')
            for c, where in enumerate(fm.position_map(TEXT)):
                assert [held.locate(c, q) for q in range(len(where))] == where
                with pytest.raises(IndexError):
                    held.locate(c, len(where))
            assert list(held.sequences) == seqs and [bytes(s) for s in held.sequences[1:3]] == seqs[1:3]
            assert [len(held[c]) for c in range(4)] == [len(s) for s in seqs] and bytes(held.sequences[-1]) == seqs[-1]


def test_the_lazy_view_cuts_what_the_model_s_bytes_hold():
    rnd = fm.rng(5)
    contig = fm.random_contig(rnd, 64 * 70 + 13)     # (more lines than the line-by-line cut takes)
    for width, eol in ((60, b'\n'), (61, b'\r\n'), (1, b'\n'), (16, b'\n')):
        text = fm.fasta([b'AC', contig, b''], width=width, eol=eol)
        for upper in (False, True):
            held = fa.resident_fasta(text, upper=upper, engine=Recording())
            want = fm.model(text, upper)[1]
            view = held.sequences[1]
            assert len(view) == len(contig) and bytes(view) == want[1] and type(view[3:9]) is bytes
            n = len(contig)
            cuts = [(0, 0), (0, 1), (0, n), (n - 1, n), (59, 61), (60, 120), (5, 4), (-20, None), (None, -n - 5), (n - 3, n + 50),
                    (-n - 7, 9), (n, n + 1), (100, 100 + 65 * width), (width - 1, 66 * width + 1)]
            cuts += [(a, a + rnd.randint(0, 200)) for a in (rnd.randrange(n) for _ in range(200))]
            for a, b in cuts:
                assert view[a:b] == want[1][a:b], (width, a, b)
            for sl in (slice(None, None, -1), slice(70, 3, -7), slice(1, 500, 61), slice(None, None, 997)):
                assert view[sl] == want[1][sl]
            for q in (0, 59, 60, -1, -n, n - 1):
                assert view[q] == want[1][q]
            for q in (n, -n - 1):
                with pytest.raises(IndexError):
                    view[q]
            assert held.sequences[2][0:5] == b'' and len(held.sequences[2]) == 0 and bytes(held.sequences[2]) == b''
            with pytest.raises(IndexError):
                held.sequences[3]


def test_several_devices_take_the_plain_python_split(tmp_path):
    rnd = fm.rng(11)
    for i in range(400):
        text, _ = fm.random_text(rnd, damage=[sorted(fm.DAMAGES)[i % len(fm.DAMAGES)]] if i % 4 == 3 else (), where='middle')
        upper = bool(i & 1)
        try:
            rows, seqs = fm.model(text, upper)
        except fm.Malformed as bad:
            with pytest.raises(ValueError, match="fasta: record %d:" % bad.record):
                fa.resident_fasta(text, upper=upper, engine=SeveralDevices())
            continue
        held = fa.resident_fasta(text, upper=upper, engine=SeveralDevices())
        assert held.handle is None and held.kind is None and isinstance(held.sequences, list)
        assert held.sequences == seqs and len(held) == len(seqs) and rows_as_tuples(held.index) == rows
        assert held.fai() == fm.fai(text)
    path = tmp_path / "two.fa"
    path.write_bytes(b'>a\nACGT\nAC\n>b\nGG\n')
    held = fa.resident_fasta(str(path), engine=SeveralDevices())
    assert held.sequences == [b'ACGTAC', b'GG'] and held[1] == b'GG' and list(held.names) == [b'a', b'b']
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b'')
    assert len(fa.resident_fasta(empty, engine=SeveralDevices())) == 0


def test_refusals_and_exports():
    for eng in (SeveralDevices(), Recording()):
        with pytest.raises(TypeError):
            fa.resident_fasta('>a\nACGT\n', engine=eng)
        with pytest.raises(TypeError):
            fa.resident_fasta(12, engine=eng)
        with pytest.raises(ValueError, match="fasta: record 0:"):
            fa.resident_fasta(b'ACGT\n', engine=eng)
        with pytest.raises(ValueError, match="fasta: record 1:"):
            fa.resident_fasta(b'>a\nAC\n>b\nAC\nA\nAC\n', engine=eng)
    with pytest.raises(ValueError, match="fasta"):              # resident_records goes on refusing the format
        fa.resident_records(b'>a\nACGT\n', format='fasta', engine=SeveralDevices())
    assert 'resident_fasta' in fa.__all__ and fa.resident_fasta is fasta.resident_fasta
    assert {'upload_fasta', 'fasta_index'} <= set(dir(_native.Engine))
