"""-m gpu: a FASTA text split on the device (fz_batch_upload_fasta / Engine.upload_fasta / resident_fasta) against the model
of tests/fasta_model.py: the index, the tables and the packed bytes exactly, at every seam of the tiles, of the scan and of
the gather's 16-byte pieces; the errors; and the three batch searches over the handle against resident_batch of the
model's contigs."""
import random

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import fasta_model as fm

pytestmark = pytest.mark.gpu

TILE = 16384
WIDTHS = [1, 15, 16, 17, 60, 61, 64, 80]


def check(engine, text, upper=False):
    """upload_fasta(text) against the model -> the number of contigs."""
    rows, seqs = fm.model(text, upper)
    h = engine.upload_fasta(text, _native.FA_UPPER if upper else 0)
    try:
        packed = b''.join(seqs)
        assert h.n_seqs == len(rows) and h.info['packed_bytes'] == len(packed) == len(h), len(text)
        starts, ends = engine.batch_tables(h)
        assert starts.tolist() == [r[3] for r in rows], ("offsets", len(text))
        assert ends.tolist() == fm.ends_of(seqs), ("ends", len(text))
        index = engine.fasta_index(h)
        assert [tuple(int(r[f]) for f in fm.FIELDS) for r in index] == rows, ("index", len(text))
        got = engine.batch_bytes(h)
        if got != packed:
            at = next(i for i, (a, b) in enumerate(zip(got, packed)) if a != b)
            raise AssertionError("packed bytes differ from byte %d of %d (text of %d bytes)" % (at, len(packed), len(text)))
    finally:
        h.release()
    return len(rows)


def dna(rnd, n, alphabet=b'ACGT'):
    return bytes(rnd.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("eol", [b'\n', b'\r\n'])
def test_tile_seams(engine, eol):
    """The first header grows byte by byte, so a contig's last lines, the next record's header and its first lines pass over
    the seam between tile 0 and tile 1.  What lay on the seam is tallied from the text and asserted."""
    rnd = random.Random(16384)
    lw = 60 + len(eol)
    contigs = [dna(rnd, 60 * ((TILE - 40) // lw)), dna(rnd, 200), b'', dna(rnd, 47)]
    seen = set()
    for pad in range(lw + 70):
        heads = [b'>' + b'h' * pad, b'>second contig header', b'>e', b'>last']
        text = fm.fasta(contigs, eol=eol, heads=heads)
        check(engine, text)
        second = text.index(b'>second')
        for side, at in (('last byte of tile 0', TILE - 1), ('first byte of tile 1', TILE)):
            if text[at:at + 1] == b'\n':
                seen.add(('newline', side))
            if text[at:at + 2] == b'\r\n':
                seen.add(('CR of a CRLF', side))
            if at == second:
                seen.add(('>', side))
        if second < TILE - 1 and second + len(heads[1]) > TILE:
            seen.add('seam inside a header')
    sides = ('last byte of tile 0', 'first byte of tile 1')
    what = ['newline', '>'] + (['CR of a CRLF'] if eol == b'\r\n' else [])
    assert seen >= {(w, s) for w in what for s in sides} | {'seam inside a header'}, seen


def test_scan_seams(engine):
    """More records, and more lines in one record, than one workgroup of the scan takes."""
    b = _native.scan_items()
    for n in (b - 1, b, b + 1, 2 * b + 1):
        assert check(engine, b'>a\nA\n' * n) == n
        assert check(engine, b'>a\n' * n + b'>b\nAC\n') == n + 1             # (headers only: empty contigs)
    rnd = random.Random(b)
    for width, lines in ((1, 2 * b + 7), (15, b + 1), (16, b)):
        assert check(engine, fm.fasta([b'AC', dna(rnd, width * (lines - 1) + 1), b'G'], width=width)) == 3


@pytest.mark.parametrize("width", WIDTHS)
def test_line_widths_and_piece_ends(engine, width):
    """Per width: a last line of 1 byte and of `width` bytes; contigs that end on a 16-byte boundary of the packed bytes and
    in the middle of a piece; LF and CRLF; with and without the final newline."""
    rnd = random.Random(width)
    alphabet = b'ACGTacgtNn'
    contigs = [dna(rnd, 16 * width, alphabet),                # last line full; ends on a piece boundary (packed offset 16 w)
               dna(rnd, 16 * width + 1, alphabet),            # last line of 1 byte; ends one byte into a piece
               dna(rnd, 15, alphabet),                        # ends on a boundary again (16 w + 1 + 15)
               dna(rnd, 5 * width, alphabet), b'', dna(rnd, 1, alphabet), dna(rnd, 3 * width + width // 2 + 1, alphabet)]
    assert (len(contigs[0]) + len(contigs[1]) + len(contigs[2])) % 16 == 0
    for eol in (b'\n', b'\r\n'):
        for final_eol in (True, False):
            for upper in (False, True):
                assert check(engine, fm.fasta(contigs, width=width, eol=eol, final_eol=final_eol), upper) == len(contigs)
    assert check(engine, fm.fasta(contigs[::-1], width=width)) == len(contigs)


def test_a_contig_over_three_tiles_and_short_ones_behind_it(engine):
    rnd = random.Random(3)
    contigs = [dna(rnd, 2 * TILE + 9000), b'', dna(rnd, 1), dna(rnd, 15), dna(rnd, TILE), dna(rnd, 16)]
    for width in (60, 61, 80):
        assert check(engine, fm.fasta(contigs, width=width)) == 6
        assert check(engine, fm.fasta(contigs, width=width, eol=b'\r\n', final_eol=False), upper=True) == 6


@pytest.mark.parametrize("final_eol", [True, False])
def test_text_of_whole_tiles_with_a_full_last_line(engine, final_eol):
    """The over-read guard: the text fills its last tile to the last byte, and that byte belongs to (or ends) a full line."""
    rnd = random.Random(2)
    body = dna(rnd, 536 * 60)
    pad = 2 * TILE - 536 * 61 - 2 + (0 if final_eol else 1)
    text = fm.fasta([body], heads=[b'>' + b'h' * pad], final_eol=final_eol)
    assert len(text) == 2 * TILE and (text.endswith(b'\n') == final_eol)
    assert check(engine, text) == 1 and check(engine, text, upper=True) == 1
    for width in (16, 64):                                   # ... and the last piece's source is the buffer's last 16 bytes
        lines = (TILE - 64) // (width + 1)
        pad = TILE - lines * (width + 1) - 2 + 1
        text = fm.fasta([dna(rnd, lines * width)], width=width, heads=[b'>' + b'h' * pad], final_eol=False)
        assert len(text) == TILE
        assert check(engine, text) == 1


def test_upper_is_bytes_upper(engine):
    rnd = random.Random(7)
    alphabet = bytes(c for c in range(256) if c not in b'\n\r')
    contigs = [dna(rnd, 1000, alphabet).replace(b'>', b'<'), dna(rnd, 333, b'acgtnryswkmbdhvACGTN*-.[`{@')]
    for width in (60, 17):
        text = fm.fasta(contigs, width=width)
        assert check(engine, text, upper=True) == 2 and check(engine, text, upper=False) == 2
    assert check(engine, b'') == 0 and check(engine, b'\n\r\n') == 0 and check(engine, b'>only a header') == 1


def searches(engine):
    held = fa.resident_batch([b'ACGTACGTACGTACGTTTGA' * 3])
    try:
        return len(fa.find_near_matches_batch(b'ACGTACGTACGTACGTTTGA', held, max_l_dist=1)[0])
    finally:
        held.release()


@pytest.mark.parametrize("text,first", fm.MALFORMED)
def test_errors_of_the_reason_table(engine, text, first):
    with pytest.raises(fm.Malformed) as m:
        fm.model(text)
    assert (m.value.record, m.value.reason) == first
    with pytest.raises(ValueError) as e:
        engine.upload_fasta(text)
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == first
    assert 'fasta: record %d:' % first[0] in str(e.value)
    with pytest.raises(ValueError, match='fasta: record %d:' % first[0]):
        fa.resident_fasta(text)
    assert searches(engine) == 3                              # nothing was left allocated or in flight


@pytest.mark.parametrize("what", sorted(fm.DAMAGES))
def test_errors_far_into_the_text(engine, what):
    """600 records of 3 lines (tile 2 and beyond): the damaged record and, with a second damage behind it, the smaller one."""
    rnd = random.Random(len(what))
    records = [fm.record_lines(rnd, c, 60, 3, 17) for c in range(600)]
    eols = [[b'\n'] * 4 for _ in records]
    if what == 'no_start':
        records[0][0] = b'h'
        want = 0
    else:
        assert fm.damaged(rnd, records[411], eols[411], what, 60) and fm.damaged(rnd, records[500], eols[500], 'long_middle', 60)
        want = 411
    text = b''.join(l + e for lines, es in zip(records, eols) for l, e in zip(lines, es))
    with pytest.raises(fm.Malformed) as m:
        fm.model(text)
    assert (m.value.record, m.value.reason) == (want, fm.DAMAGES[what])
    with pytest.raises(ValueError) as e:
        engine.upload_fasta(text)
    assert (e.value.info['bad_record'], e.value.info['bad_reason']) == (want, fm.DAMAGES[what])
    assert searches(engine) == 3


def same_matches(a, b):
    return [[(m.start, m.end, m.dist, bytes(m.matched)) for m in per] for per in a] == \
           [[(m.start, m.end, m.dist, bytes(m.matched)) for m in per] for per in b]


@pytest.fixture(scope="module")
def genome():
    """Four contigs (one of more than three tiles), 30 % lower case, and patterns planted flush with a contig's start and
    end, across a line end of the source, and across the seam between two contigs."""
    rnd = random.Random(2027)
    pats = [dna(rnd, 20) for _ in range(5)]
    contigs = [bytearray(dna(rnd, 200)), bytearray(dna(rnd, 3 * TILE + 1234)), bytearray(), bytearray(dna(rnd, 90))]
    contigs[1][:20] = pats[0]                                 # flush with the start
    contigs[1][-20:] = pats[1]                                # flush with the end
    contigs[1][60 * 100 + 50:60 * 100 + 70] = pats[2]         # across a line end of the source (60-column lines)
    contigs[0][-10:] = pats[3][:10]                           # across the seam of contigs 0 and 1 ...
    contigs[1][20:30] = pats[3][10:]
    contigs[3][30:50] = pats[4]
    contigs[3][35] ^= 0x20                                    # one planted base in lower case
    for c in contigs:
        for i in range(len(c)):
            if rnd.random() < 0.3 and not (c is contigs[1] and (i < 20 or i >= len(c) - 20 or 6050 <= i < 6070)):
                c[i] |= 0x20
    heads = [b'>chr1 the first', b'>chr2', b'>empty', b'>chr4\tlast']
    return fm.fasta([bytes(c) for c in contigs], heads=heads), pats


@pytest.mark.parametrize("upper", [False, True])
def test_searches_over_the_handle(engine, genome, upper):
    text, pats = genome
    rows, seqs = fm.model(text, upper)
    held, listed = fa.resident_fasta(text, upper=upper), fa.resident_batch(seqs)
    try:
        assert isinstance(held, fa.batch.BatchSequences) and held.kind == 'bytes' and len(held) == 4
        assert list(held.names) == [b'chr1', b'chr2', b'empty', b'chr4'] and held.lengths.tolist() == [len(s) for s in seqs]
        assert held.fai() == fm.fai(text)
        found = 0
        for p in pats:
            got, want = fa.find_near_matches_batch(p, held, max_l_dist=2), fa.find_near_matches_batch(p, listed, max_l_dist=2)
            assert same_matches(got, want)
            assert all(m.matched == seqs[c][m.start:m.end] and type(m.matched) is bytes for c, per in enumerate(got) for m in per)
            found += sum(map(len, got))
        one = fa.find_near_matches_batch(pats[0], held, max_l_dist=0)
        assert [(m.start, m.end) for m in one[1]] == [(0, 20)] and not one[0]
        assert [(m.start, m.end) for m in fa.find_near_matches_batch(pats[1], held, max_l_dist=0)[1]] == [(len(seqs[1]) - 20, len(seqs[1]))]
        assert [(m.start, m.end) for m in fa.find_near_matches_batch(pats[2], held, max_l_dist=0)[1]] == [(6050, 6070)]
        assert fa.find_near_matches_batch(pats[3], held, max_l_dist=2) == [[], [], [], []]        # the seam one is not found
        if upper:
            assert [(m.start, m.dist) for m in fa.find_near_matches_batch(pats[4], held, max_l_dist=0)[3]] == [(30, 0)]
        assert found >= (4 if upper else 3)                       # (the pattern of contig 3 lies in mixed case)
        for limits in (dict(max_l_dist=1), dict(max_substitutions=2, max_insertions=0, max_deletions=0)):
            multi, want = fa.find_near_matches_multi_batch(pats, held, **limits), fa.find_near_matches_multi_batch(pats, listed, **limits)
            assert len(multi) == len(pats) and all(same_matches(a, b) for a, b in zip(multi, want))
        best, want = fa.find_best_matches_batch(pats, held, max_l_dist=2), fa.find_best_matches_batch(pats, listed, max_l_dist=2)
        for name in ('pattern', 'dist', 'start', 'end', 'tied'):
            assert np.array_equal(getattr(best, name), getattr(want, name)), name
        assert best.pattern[2] == -1 and best.pattern[1] >= 0
        # separate limits: the per-sequence loop, over the contigs' bytes one at a time
        limits = dict(max_substitutions=1, max_insertions=1, max_deletions=0, max_l_dist=1)
        assert same_matches(fa.find_near_matches_batch(pats[2], held, **limits), fa.find_near_matches_batch(pats[2], seqs, **limits))
    finally:
        held.release()
        listed.release()


def test_a_path_is_mapped_and_the_index_comes_on_demand(engine, genome, tmp_path):
    text, pats = genome
    path = tmp_path / "genome.fa"
    path.write_bytes(text)
    rows, seqs = fm.model(text)
    for source in (str(path), path, bytearray(text), memoryview(text)):
        held = fa.resident_fasta(source)
        assert held._rows is None                                 # nothing but ends[] came back with the upload
        assert bytes(held.sequences[3]) == seqs[3] and held.sequences[1][6050:6070] == seqs[1][6050:6070]
        assert held.locate(1, 6060) == fm.position_map(text)[1][6060] and text[held.locate(3, 31)] == seqs[3][31]
        held.release()
    other = fa.resident_batch(seqs)
    with pytest.raises(ValueError):
        engine.fasta_index(other.handle)                          # not a handle of upload_fasta
    other.release()
