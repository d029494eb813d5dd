"""Case builders for the end-overlap tests (tests/test_overlap_host.py, tests/test_gpu_overlap.py): reads that end in an
edited prefix of a pattern, the layouts around them, and the case file of tests/overlap_emul.cpp.  Nothing here knows an
answer: every expectation comes from tests/overlap_model.py."""
import random
import struct

ALPHABETS = (b"ACGT", bytes([0x00, 0xff]), bytes([0x00, 0xff, 0x41, 0x43]))


def rand_bytes(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def edited(rng, s, edits, alphabet=b"ACGT", kinds="sid"):
    """s with `edits` random edits: s(ubstitution), i(nsertion), d(eletion)"""
    s = bytearray(s)
    for _ in range(edits):
        kind = rng.choice(kinds)
        if kind == "i" or not s:
            s.insert(rng.randrange(len(s) + 1), rng.choice(alphabet))
        elif kind == "d":
            del s[rng.randrange(len(s))]
        else:
            q = rng.randrange(len(s))
            s[q] = rng.choice([c for c in alphabet if c != s[q]] or list(alphabet))
    return bytes(s)


def planted_read(rng, pattern, i, edits, body, alphabet=b"ACGT", kinds="sid"):
    """`body` random bytes, then pattern[:i] with `edits` edits: the read breaks off inside the pattern"""
    return rand_bytes(rng, body, alphabet) + edited(rng, pattern[:i], edits, alphabet, kinds)


def mixed_reads(rng, patterns, k, count, alphabet=b"ACGT", longest=100):
    """count reads: planted prefixes within and just over their budget, random ends, and reads shorter than the tail"""
    reads = []
    for _ in range(count):
        p = rng.choice(patterns)
        m, roll = len(p), rng.random()
        if roll < 0.5 and m > 1:
            i = rng.randrange(1, m)
            reads.append(planted_read(rng, p, i, rng.randrange(0, k * i // m + 2), rng.randrange(0, longest - m + 1 if longest > m else 1), alphabet))
        elif roll < 0.7:
            reads.append(rand_bytes(rng, rng.randrange(0, min(m + k, longest) + 1), alphabet))   # shorter than the tail
        elif roll < 0.8 and m > 1:
            i = rng.randrange(1, m)                          # the read is nothing but (part of) a prefix
            reads.append(edited(rng, p[:i], rng.randrange(0, 2), alphabet)[rng.randrange(0, i):])
        else:
            reads.append(rand_bytes(rng, rng.randrange(0, longest + 1), alphabet))
    return reads


def adversarial_neighbours(pattern, o, filler=b"T"):
    """Reads whose NEIGHBOURS hold what would complete an overlap, packed back to back (m >= 8 and o <= 4 assumed):
    a prefix that the next read continues; a prefix at the end of a read in front of an empty read and of reads shorter
    than o; a read shorter than its prefix whose predecessor ends with the missing head."""
    p, f = bytes(pattern), bytes(filler)
    half = len(p) // 2
    reads = [f * 9 + p[:half], p[half:] + f * 5,             # the next read begins with the bytes that continue the prefix
             f * 7 + p[:half + 1], b"", f * 3,               # ... while this read is empty
             f * 6 + p[:6], p[6:5 + o], f * 4,               # ... or shorter than o and itself a continuation
             f * 5 + p[:3], p[3:7], f * 2,                   # the previous read ends in the head of this read's "prefix"
             p[:half], p[:1], p[:2], b"", p[:len(p) - 1]]
    return reads


def pack(reads):
    return b"".join(reads), [len(r) for r in reads]


def emul_group(mode, k, o, patterns, reads, pad=0):
    """one group of the emulator's case file"""
    blob, lens = pack(reads)
    out = [struct.pack("<6I", mode, k, o, len(patterns), len(reads), pad)]
    for p in patterns:
        out.append(struct.pack("<I", len(p)) + bytes(p))
    out.append(struct.pack("<%dI" % len(lens), *lens))
    out.append(blob)
    return b"".join(out)


def rng_of(*seed):
    return random.Random(repr(seed))


def offsets(reads):
    import numpy as np
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return offs


def rows_arrays(rows):
    """fz_overlap rows -> (pattern, overlap, dist, start) as the public call and the model give them"""
    import numpy as np
    none = rows["pattern"] == 0xffff
    return (np.where(none, -1, rows["pattern"].astype(np.int32)), rows["overlap"].astype(np.int32),
            np.where(none, -1, rows["dist"].astype(np.int32)), rows["start"].astype(np.int64))


def result_arrays(res):
    return res.pattern, res.overlap, res.dist, res.start


# Two patterns of 20 that tie on the matched characters at the end of TIE_READ but not on the distance (k = 2): X's first 10
# bytes end the read exactly (10 matched, 0 edits), Y's first 11 are those 10 with one byte inserted (10 matched, 1 edit).
TIE_X = b"ACGTTGCAAGCCTAGGATCC"
TIE_Y = TIE_X[:4] + b"T" + TIE_X[4:10] + b"GGGGGGGGG"
TIE_READ = b"TTTTTTTTTTTTTTTTTTTTT" + TIE_X[:10]
