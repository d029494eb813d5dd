"""Symbol classes: pattern positions that accept a SET of sequence bytes (IUPAC guides, degenerate primers, UMI runs).

``classes`` maps a pattern byte to the sequence bytes it accepts.  Pattern byte ``c`` matches sequence byte ``t`` iff
``t == c`` or ``c`` is a key and ``t`` is in its set; the class distance of a pattern and a window of its length is the
number of positions that do not match.  Sequence bytes are never classes: an ``N`` in the sequence matches a pattern ``N``
by equality and a pattern ``A`` not at all.  All sets together may name at most 8 distinct bytes, the base symbols; a key
may itself be one (``{ord('A'): b'Aa', ...}`` asks for case-insensitive matching).

The keyword lives on the three multi-pattern calls (find_near_matches_multi, find_near_matches_multi_batch,
find_best_matches_batch) and is answered by the multi-pattern pass alone, by verification kernels of its own: mismatch-only
limits (``max_insertions=0, max_deletions=0``, at least one substitution), bytes-like sequences, and every subsequence inside
the pass's domain (k <= 8, length <= 128, length // (k + 1) >= 4) — a list of one included.  Everything else raises
UnsupportedSearch before anything is searched; there is no class-aware single-pattern route and no CPU fallback.
"""
from . import _native
from .common import LevenshteinSearchParams
from .engine import is_byteslike

__all__ = ['IUPAC_DNA', 'class_tables', 'class_call']

# the IUPAC nucleotide codes, upper case
IUPAC_DNA = {ord(code): bases for code, bases in (
    ('R', b'AG'), ('Y', b'CT'), ('S', b'CG'), ('W', b'AT'), ('K', b'GT'), ('M', b'AC'),
    ('B', b'CGT'), ('D', b'AGT'), ('H', b'ACT'), ('V', b'ACG'),
    ('N', b'ACGT'))}

MAX_BASE_SYMBOLS = 8
MAX_K, MAX_M, MIN_L = 8, 128, 4                      # the multi-pattern domain (csrc/fz_device.h: FZ_MP_MAX_K, _MAX_M, _MIN_L)


def class_tables(classes):
    """The mapping -> (pmask, tmask), two bytes objects of 256 as the C-ABI's class entries take them: tmask[t] = the
    one-hot bit of base symbol t, pmask[c] = the bits of key c's set.  ValueError for a key outside 0..255, an empty set or
    more than 8 base symbols; TypeError for a key that is neither an int nor one byte."""
    sets = {}
    for key, members in classes.items():
        if isinstance(key, (bytes, bytearray)):
            if len(key) != 1:
                raise ValueError('a class key must be one byte, not %r' % (key,))
            key = key[0]
        elif isinstance(key, bool) or not isinstance(key, int):
            raise TypeError('a class key must be an int or a bytes object of length 1, not %r' % (key,))
        if not 0 <= key <= 255:
            raise ValueError('class key %d is not a byte value (0..255)' % key)
        members = bytes(memoryview(members))
        if not members:
            raise ValueError('the set of class key %d is empty' % key)
        sets[key] = sets.get(key, b'') + members
    base = sorted(set(b''.join(sets.values())))
    if len(base) > MAX_BASE_SYMBOLS:
        raise ValueError('the classes name %d distinct sequence bytes; at most %d base symbols fit one mask byte'
                         % (len(base), MAX_BASE_SYMBOLS))
    tmask, pmask = bytearray(256), bytearray(256)
    for bit, t in enumerate(base):
        tmask[t] = 1 << bit
    for key, members in sets.items():
        for t in members:
            pmask[key] |= tmask[t]
    return bytes(pmask), bytes(tmask)


def class_call(subsequences, limits, classes, byteslike_sequences):
    """Everything a class call checks before anything is searched, no device needed: -> (pattern bytes per subsequence,
    k, tables).  ValueError / TypeError for the mapping and the limits as above and as LevenshteinSearchParams raises them;
    UnsupportedSearch, naming the list position where one is at fault, for everything outside the scope."""
    tables = class_tables(classes)
    search_params = LevenshteinSearchParams(*limits)
    max_subs, max_ins, max_dels, max_l = search_params.unpacked
    if max_ins != 0 or max_dels != 0:
        raise _native.UnsupportedSearch('classes are searched under mismatch-only limits (max_insertions=0, max_deletions=0); '
                                        'Levenshtein and generic limits with classes are not supported')
    k = min(max_subs, max_l)
    if k < 1:
        raise _native.UnsupportedSearch('classes need a budget of at least one substitution: an exact search knows no classes')
    if not byteslike_sequences:
        raise _native.UnsupportedSearch('classes are searched in bytes-like sequences only (not str, not mixed kinds)')
    patterns = []
    for i, p in enumerate(subsequences):
        if not is_byteslike(p):
            raise _native.UnsupportedSearch('subsequence %d is not bytes-like: classes are sets of bytes' % i)
        pb = p if isinstance(p, bytes) else bytes(memoryview(p))
        m = len(pb)
        if k > MAX_K or m > MAX_M or m // (k + 1) < MIN_L:
            raise _native.UnsupportedSearch(
                'subsequence %d (length %d, %d substitutions) is outside the multi-pattern domain k <= %d, length <= %d, '
                'length // (k + 1) >= %d, the only place classes are searched' % (i, m, k, MAX_K, MAX_M, MIN_L))
        patterns.append(pb)
    if patterns:
        _native.multi_plan_classes(patterns, k, tables)  # a subsequence whose spellings do not fit the filter's table: refused by position
    return patterns, k, tables
