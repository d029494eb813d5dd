"""The model the record split is held to (fz_batch_upload_records, fz_debug_records_split, resident_records): plain Python,
independent of fuzzysearch_amd/records.py.  Plus the generators of the texts the tests feed both."""
import random

import numpy as np

REASON_COUNT, REASON_AT, REASON_PLUS, REASON_QUAL = 1, 2, 3, 4


class Malformed(Exception):
    def __init__(self, record, reason):
        Exception.__init__(self, "record %d reason %d" % (record, reason))
        self.record, self.reason = record, reason


def split_lines(text):
    """-> [(offset of the line's first byte, its content)]: a final line needs no terminator, "" has no lines, one CR in
    front of the LF (or ending an unterminated last line) is not content."""
    lines = text.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    out, pos = [], 0
    for ln in lines:
        out.append((pos, ln[:-1] if ln.endswith(b'\r') else ln))
        pos += len(ln) + 1
    return out


def model(text, fmt):
    """-> (starts, reads, n_lines) or raises Malformed with the smallest (record, reason)."""
    lines = split_lines(bytes(text))
    if fmt == 'lines':
        return [s for s, _ in lines], [l for _, l in lines], len(lines)
    assert fmt == 'fastq'
    while lines and lines[-1][1] == b'':
        lines.pop()
    errors = []
    if len(lines) % 4:
        errors.append((len(lines) // 4, REASON_COUNT))
    for r in range(len(lines) // 4):
        head, seq, plus, qual = (lines[4 * r + i][1] for i in range(4))
        if not head.startswith(b'@'):
            errors.append((r, REASON_AT))
        elif not plus.startswith(b'+'):
            errors.append((r, REASON_PLUS))
        elif len(qual) != len(seq):
            errors.append((r, REASON_QUAL))
    if errors:
        raise Malformed(*min(errors))
    kept = lines[1::4]
    return [s for s, _ in kept], [l for _, l in kept], len(lines)


def tables(text, fmt):
    """-> (starts u64, ends u64, packed bytes, n_lines) of the model."""
    starts, reads, n_lines = model(text, fmt)
    ends = np.cumsum([len(r) for r in reads], dtype=np.uint64) if reads else np.zeros(0, np.uint64)
    return np.array(starts, dtype=np.uint64), ends, b''.join(reads), n_lines


def fastq(reads, heads=None, eol=b'\n', final_eol=True, quals=None):
    """A FASTQ text of `reads`; heads[r] = the header line of record r (default b'@r<r>'); eol = a terminator or one per line."""
    out = []
    for r, read in enumerate(reads):
        out += [heads[r] if heads else b'@r%d' % r, read, b'+', quals[r] if quals else b'I' * len(read)]
    eols = eol if isinstance(eol, list) else [eol] * len(out)
    text = b''.join(l + e for l, e in zip(out, eols))
    if not final_eol and text:
        text = text[:-len(eols[len(out) - 1])]
    return text


def random_line(rnd, alphabet, max_len):
    return bytes(rnd.choice(alphabet) for _ in range(rnd.randint(0, max_len)))


def random_lines_text(rnd):
    """Small 'lines' text: LF / CRLF mixed per line, empty lines, a lone CR in content, a missing final terminator."""
    n = rnd.choice([0, 0, 1, 1, 2, 3, 5, 8, 13])
    parts = []
    for _ in range(n):
        parts.append(random_line(rnd, b'ACGT\r@+', rnd.choice([0, 1, 4, 9])) + rnd.choice([b'\n', b'\n', b'\r\n']))
    text = b''.join(parts)
    if parts and rnd.random() < 0.4:
        text = text[:-1]                            # no final LF (a CRLF's CR then ends the unterminated line)
        if text.endswith(b'\r') and rnd.random() < 0.5:
            text = text[:-1]
    return text


def random_fastq_text(rnd, break_it=False):
    """Small valid FASTQ: LF / CRLF mixed per line, empty reads, '@' / '+' as first quality characters, a lone CR in the
    read, a missing final terminator, 0-3 trailing blank lines.  break_it: a random selection of damages instead."""
    n = rnd.choice([0, 1, 1, 2, 3, 5])
    lines = []
    for r in range(n):
        read = random_line(rnd, b'ACGT', rnd.choice([0, 1, 5, 12]))
        if read and rnd.random() < 0.2:
            read = read[:1] + b'\r' + read[1:]
        qual = bytes(rnd.choice(b'@+I5') for _ in range(len(read)))
        lines += [b'@' + random_line(rnd, b'abc 1', 6), read, b'+' + rnd.choice([b'', b'x']), qual]
    if break_it and lines:
        for _ in range(rnd.randint(1, 2)):
            i = rnd.randrange(len(lines))
            kind = rnd.randrange(4)
            if kind == 0:
                del lines[i]
            elif kind == 1:
                lines[i] = b'x' + lines[i]
            elif kind == 2:
                lines[i] = lines[i][1:]
            else:
                lines.insert(i, b'')
    text = b''.join(l + rnd.choice([b'\n', b'\n', b'\r\n']) for l in lines)
    if lines and rnd.random() < 0.3:
        text = text[:-1]
        if text.endswith(b'\r') and rnd.random() < 0.5:
            text = text[:-1]
    else:
        text += b''.join(rnd.choice([b'\n', b'\r\n']) for _ in range(rnd.randint(0, 3)))
    return text


def rng(seed):
    return random.Random(seed)
