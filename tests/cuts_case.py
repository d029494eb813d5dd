"""Case builders for the score-cut tests (tests/test_cuts_host.py, tests/test_gpu_cuts.py): seeded reads with good and bad
ends, tables over small alphabets, the layouts around the reads, and the case file of tests/cuts_emul.cpp.  Nothing here
knows an answer: every expectation comes from tests/cuts_model.py."""
import random
import struct

import numpy as np

ALPHABETS = (b"ACGT", bytes([0x00, 0xff]), bytes([0x00, 0xff, 0x41, 0x43]))
STOP3, STOP5, RATE = 1, 2, 4                                # fz_batch_score_cuts' flags
PIECE = 64                                                  # bytes of a lane's piece (csrc/fz_device.h: FZ_CUT_PIECE_DWORDS)


def rng_of(*seed):
    return random.Random(repr(seed))


def rand_bytes(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def rand_table(rng, alphabet, top=None, lo=-3, hi=3):
    """A table of small scores over `alphabet` (every other byte: -1); `top`: a byte that gets the highest score of all"""
    w = [-1] * 256
    for c in alphabet:
        w[c] = rng.randrange(lo, hi + 1)
    if top is not None:
        w[top] = max(w) + 1 if max(w) >= 0 else 1
    return w


def ended_read(rng, n, w, alphabet):
    """n bytes whose two ends are runs of mostly well-scored bytes of random lengths (they may meet or cross the middle),
    with a share of other bytes in them: peaks at every depth, equal peaks, runs that the rate refuses"""
    if n == 0:
        return b""
    good = [c for c in alphabet if w[c] > 0] or list(alphabet)
    r = bytearray(rand_bytes(rng, n, alphabet))
    for side in (0, 1):
        run = rng.randrange(0, n + 1) if rng.random() < 0.7 else 0
        noise = rng.choice((0.0, 0.1, 0.3))
        for q in range(run):
            if rng.random() >= noise:
                r[q if side else n - 1 - q] = rng.choice(good)
    return bytes(r)


def aligned_reads(rng, lengths, w, alphabet, filler):
    """For every length and every start alignment 0 .. 3 of the packed bytes one ended_read, steered there by a read of
    0 .. 3 bytes of `filler` in front of it: every read's neighbours end and begin with the filler byte."""
    reads, at = [], 0
    for n in lengths:
        for a in range(4):
            fill = bytes([filler]) * ((a - at) % 4)
            read = ended_read(rng, n, w, alphabet)
            reads += [fill, read]
            at += len(fill) + len(read)
    return reads


def pack(reads):
    return b"".join(reads), [len(r) for r in reads]


def offsets(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return offs


def flags_of(stop3, stop5, rate):
    return (STOP3 if stop3 else 0) | (STOP5 if stop5 else 0) | (RATE if rate is not None else 0)


def emul_group(w3, w5, flags, rate, reads, pad):
    """one group of the emulator's case file"""
    blob, lens = pack(reads)
    num, den = rate if rate is not None else (0, 1)
    sides = (1 if w3 is not None else 0) | (2 if w5 is not None else 0)
    out = [struct.pack("<6I", sides, flags, num, den, len(reads), pad)]
    for w in (w3, w5):
        if w is not None:
            out.append(struct.pack("<256h", *w))
    out.append(struct.pack("<%dI" % len(lens), *lens))
    out.append(blob)
    return b"".join(out)


def groups(lengths, seed="groups"):
    """(w3, w5, stop, rate, reads, pad byte): each side alone and both; stop on and off; the rate on and off; behind the data
    and around every read 0x00 or 0xff, which the tables give their highest score"""
    out = []
    for sides in (1, 2, 3):
        for stop in (True, False):
            for rate in (None, (1, 5), (1, 3)):
                if rate == (1, 3) and stop:
                    continue
                for pad in (0x00, 0xff):
                    rng = rng_of(seed, sides, stop, rate, pad)
                    alphabet = ALPHABETS[2] if rng.random() < 0.5 else ALPHABETS[1]
                    w3 = rand_table(rng, alphabet, top=pad) if sides & 1 else None
                    w5 = rand_table(rng, alphabet, top=pad) if sides & 2 else None
                    reads = aligned_reads(rng, lengths, w3 if w3 is not None else w5, alphabet, pad)
                    out.append((w3, w5, stop, rate, reads, pad))
    return out


def twin_batch(rng, n_seqs, w, alphabet, top, long_at=None, long_len=70000):
    """n_seqs reads of 0 .. 20 bytes whose first and last bytes are often `top` (the highest score: what a neighbour would
    add); `long_at`: the position of one read of long_len bytes that ends in a long well-scored run"""
    reads = []
    for j in range(n_seqs):
        if j == long_at:
            good = [c for c in alphabet if w[c] > 0] or [top]
            body = bytearray(rand_bytes(rng, long_len, alphabet))
            for q in range(long_len // 2, long_len):
                if rng.random() < 0.97:
                    body[q] = rng.choice(good)
            reads.append(bytes(body))
            continue
        r = bytearray(ended_read(rng, rng.randrange(0, 21), w, alphabet))
        if r and rng.random() < 0.6:
            r[0] = top
        if r and rng.random() < 0.6:
            r[-1] = top
        reads.append(bytes(r))
    return reads


def rows_arrays(rows):
    """fz_cut rows -> (start, end) as the public call and the model give them"""
    return rows["start"].astype(np.int64), rows["end"].astype(np.int64)
