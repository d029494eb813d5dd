"""The model of format_records: three lines of Python, the verdict beside them, and the builders of the tests' cases."""
import random

PRESETS = {'lines': ((b'', b'\n'), None),
           'fastq': ((b'', b'\n', b'\n+\n', b'\n'), (1, 2)),
           'fasta': ((b'>', b'\n', b'\n'), None)}


def model(cols, lits):
    """text = join over the records of lit[0] + col[0][j] + lit[1] + ... + col[C-1][j] + lit[C]."""
    return b''.join(lits[0] + b''.join(bytes(col[j]) + lits[c + 1] for c, col in enumerate(cols))
                    for j in range(len(cols[0])))


def starts(cols, lits):
    """at[]: where every record starts in the text, the text's length last."""
    at = [0]
    for j in range(len(cols[0])):
        at.append(at[-1] + sum(map(len, lits)) + sum(len(col[j]) for col in cols))
    return at


def first_bad(cols, equal):
    """-> (record, 1) of the smallest record in which the two checked columns differ in length, or None."""
    if equal is None:
        return None
    a, b = equal
    for j in range(len(cols[0])):
        if len(cols[a][j]) != len(cols[b][j]):
            return j, 1
    return None


def offsets(seqs):
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    return offs


def rnd_bytes(rnd, n, alphabet=None):
    if alphabet is None:
        return rnd.randbytes(n)
    return bytes(rnd.choice(alphabet) for _ in range(n))


def random_columns(rnd, n_cols, n, max_len=33, alphabet=None):
    """n_cols columns of n sequences with lengths 0 .. max_len in shuffled order."""
    cols = []
    for _ in range(n_cols):
        lens = [i % (max_len + 1) for i in range(n)]
        rnd.shuffle(lens)
        cols.append([rnd_bytes(rnd, k, alphabet) for k in lens])
    return cols


def fastq_columns(rnd, n, max_len=40):
    """-> (heads with their '@', reads, quals) of n valid FASTQ records; no '\\n' or '\\r' in any of them."""
    heads = [b'@r%d %s' % (j, rnd_bytes(rnd, rnd.randint(0, 9), b'abc:/1')) for j in range(n)]
    reads = [rnd_bytes(rnd, rnd.randint(0, max_len), b'ACGTN') for _ in range(n)]
    quals = [rnd_bytes(rnd, len(r), b'!#5?I@+') for r in reads]
    return heads, reads, quals


def rng(seed):
    return random.Random(seed)
