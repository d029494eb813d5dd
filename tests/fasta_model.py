"""The model the FASTA split is held to (fz_batch_upload_fasta, fz_debug_fasta_split, resident_fasta): plain Python written
from the rule of `samtools faidx` as include/fzhip.h states it, independent of fuzzysearch_amd/fasta.py.  Plus the generators
of the texts the tests feed both."""
import random

REASON_START, REASON_EMPTY, REASON_WIDTH = 5, 6, 7
FIELDS = ('header_start', 'header_len', 'length', 'offset', 'linebases', 'linewidth')


class Malformed(Exception):
    def __init__(self, record, reason):
        Exception.__init__(self, "record %d reason %d" % (record, reason))
        self.record, self.reason = record, reason


def split_lines(text):
    """-> [(offset of the line's first byte, its content, its width)]: a final line needs no terminator, one CR in front of
    the LF (or ending an unterminated last line) is not content, trailing empty lines are no lines.  The width reaches to
    the next line's first byte, or to the end of the text."""
    lines = text.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    out, pos = [], 0
    for ln in lines:
        out.append((pos, ln[:-1] if ln.endswith(b'\r') else ln, min(len(ln) + 1, len(text) - pos)))
        pos += len(ln) + 1
    while out and out[-1][1] == b'':
        out.pop()
    return out


def model(text, upper=False):
    """-> (rows, sequences): rows = one tuple in the order of FIELDS per record.  Raises Malformed with the smallest
    (record, reason)."""
    text = bytes(text)
    lines = split_lines(text)
    errors = []
    if lines and not text.startswith(b'>'):
        errors.append((0, REASON_START))
    records = []
    for line in lines:
        if line[1].startswith(b'>'):
            records.append((line, []))
        elif records:
            records[-1][1].append(line)
    rows, sequences = [], []
    for r, ((hpos, head, hwidth), body) in enumerate(records):
        if body:
            offset, linebases, linewidth = body[0][0], len(body[0][1]), body[0][2]
        else:
            offset, linebases, linewidth = hpos + hwidth, 0, 0
        for i, (_pos, content, width) in enumerate(body):
            if content == b'':
                errors.append((r, REASON_EMPTY))
            if i < len(body) - 1:
                if len(content) != linebases or width != linewidth:
                    errors.append((r, REASON_WIDTH))
            elif len(content) > linebases:
                errors.append((r, REASON_WIDTH))
        seq = b''.join(content for _pos, content, _width in body)
        rows.append((hpos + 1, len(head) - 1, len(seq), offset, linebases, linewidth))
        sequences.append(seq.upper() if upper else seq)
    if errors:
        raise Malformed(*min(errors))
    return rows, sequences


def position_map(text):
    """-> per record the list of every base's offset in the text (from the lines, no arithmetic)."""
    out = []
    for pos, content, _width in split_lines(bytes(text)):
        if content.startswith(b'>'):
            out.append([])
        elif out:
            out[-1] += range(pos, pos + len(content))
    return out


def ends_of(sequences):
    out, at = [], 0
    for s in sequences:
        at += len(s)
        out.append(at)
    return out


def fai(text):
    rows, _ = model(text)
    heads = [bytes(text)[r[0]:r[0] + r[1]] for r in rows]
    return b''.join(b'%s\t%d\t%d\t%d\t%d\n' % ((h.replace(b'\t', b' ').split(b' ')[0],) + r[2:]) for h, r in zip(heads, rows))


def fasta(contigs, width=60, eol=b'\n', final_eol=True, heads=None):
    """A FASTA text: contigs[c] on lines of `width` bases; heads[c] = the header line of record c (default b'>c<c>')."""
    out = []
    for c, seq in enumerate(contigs):
        out.append(heads[c] if heads else b'>c%d' % c)
        out += [seq[i:i + width] for i in range(0, len(seq), width)]
    text = b''.join(l + eol for l in out)
    if not final_eol and text:
        text = text[:-len(eol)]
    return text


ALPHABET = b'ACGTacgtNnRYKMryk*-'

# damage -> the reason the model must find for the damaged record (when nothing smaller hides it)
DAMAGES = {'no_start': REASON_START, 'empty_line': REASON_EMPTY, 'short_middle': REASON_WIDTH, 'long_middle': REASON_WIDTH,
           'long_last': REASON_WIDTH, 'other_eol': REASON_WIDTH}


def random_contig(rnd, n):
    return bytes(rnd.choice(ALPHABET) for _ in range(n))


def record_lines(rnd, c, width, n_lines, last_len):
    """[header, sequence lines...] of a record with n_lines sequence lines, the last of last_len bases."""
    head = b'>' + rnd.choice([b'c%d' % c, b'c%d some words' % c, b'c%d\ttab' % c, b'', b' x'])
    body = [random_contig(rnd, width) for _ in range(max(0, n_lines - 1))]
    if n_lines:
        body.append(random_contig(rnd, last_len))
    return [head] + body


def damaged(rnd, lines, eols, what, width):
    """One record's lines and terminators damaged in place -> True when the damage applies to this record."""
    n_seq = len(lines) - 1
    if what == 'empty_line' and n_seq >= 2:
        lines[rnd.randrange(1, n_seq)] = b''          # never the text's last line: that one would be a trailing empty line
    elif what == 'short_middle' and n_seq >= 2 and width >= 2:
        i = rnd.randrange(1, n_seq)
        lines[i] = lines[i][:-1]
    elif what == 'long_middle' and n_seq >= 2:
        i = rnd.randrange(1, n_seq)
        lines[i] += b'A'
    elif what == 'long_last' and n_seq >= 2:
        lines[n_seq] = lines[1] + b'A'
    elif what == 'other_eol' and n_seq >= 3:
        i = rnd.randrange(2, n_seq)                   # not the first sequence line (that one defines the width)
        eols[i] = b'\r\n' if eols[i] == b'\n' else b'\n'
    else:
        return False
    return True


def random_text(rnd, damage=(), where=None):
    """A small FASTA text: line widths 1 .. 80, LF or CRLF, with and without a final newline, empty contigs (first, in the
    middle, last, consecutive headers), 0-2 trailing blank lines.  damage: names of DAMAGES applied to the record(s) `where`
    ('first' / 'middle' / 'last', or a list of record numbers) -> (text, the records damaged as {record: damage})."""
    n = rnd.choice([1, 2, 3, 3, 5, 8])
    if damage:
        n = max(n, 3)
    eol = rnd.choice([b'\n', b'\n', b'\r\n'])
    records, all_eols = [], []
    for c in range(n):
        width = rnd.randint(1, 80) if rnd.random() < 0.7 else rnd.choice([1, 15, 16, 17, 60, 61])
        n_lines = rnd.choice([0, 1, 1, 2, 3, 4, 7])
        if damage:
            n_lines = max(n_lines, 3)
        last_len = rnd.choice([1, width, rnd.randint(1, width)])
        lines = record_lines(rnd, c, width, n_lines, last_len)
        records.append((lines, [eol] * len(lines), width))
    done = {}
    if damage:
        if where == 'first':
            targets = [0]
        elif where == 'middle':
            targets = [rnd.randrange(1, n - 1)]
        elif where == 'last':
            targets = [n - 1]
        else:
            targets = list(where)
        for t, what in zip(targets, damage):
            if what == 'no_start':
                records[0][0][0] = records[0][0][0][1:] or b'x'
                done[0] = what
            elif damaged(rnd, records[t][0], records[t][1], what, records[t][2]):
                done[t] = what
    text = b''.join(l + e for lines, eols, _w in records for l, e in zip(lines, eols))
    tail = rnd.random()
    if tail < 0.3:
        text = text[:-len(eol)]
    elif tail < 0.5:
        text += b''.join(rnd.choice([b'\n', b'\r\n']) for _ in range(rnd.randint(1, 2)))
    return text, done


# the reason table: a malformed text, the (record, reason) it is refused with
MALFORMED = [
    (b'A', (0, REASON_START)), (b'\n>a\nA\n', (0, REASON_START)), (b';c\n>a\nA\n', (0, REASON_START)),
    (b'>a\n\nAC\n', (0, REASON_EMPTY)), (b'>a\nAC\n\n>b\nA\n', (0, REASON_EMPTY)), (b'>a\nAC\n\r\nAC\n', (0, REASON_EMPTY)),
    (b'>a\nAC\nACG\n', (0, REASON_WIDTH)), (b'>a\nA\n>b\nAC\nA\nAC\n', (1, REASON_WIDTH)), (b'>a\nAC\r\nAC\nAC\n', (0, REASON_WIDTH)),
    (b'>a\nAC\nAC\r\nAC\n', (0, REASON_WIDTH)),
]


def rng(seed):
    return random.Random(seed)
