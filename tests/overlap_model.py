"""The definition of find_end_overlaps_batch in Python: a strictly partial PREFIX of a subsequence at the END of a sequence.

Per sequence r (n items), subsequence p (m items), budget k and min_overlap o, over the prefix lengths o <= i <= m - 1 with
the scaled budget k_i = k * i // m:
  Levenshtein     E(i) = min over a of ed(p[:i], r[a:]), j(i) = the longest suffix of r at that distance.  That is the
                  reference's own expansion of the reversed prefix over the reversed end of the sequence (oracle.expand: the
                  last arg-min of the bottom row), which answers (None, None) when E(i) > k_i
  substitutions   E(i) = Hamming(p[:i], r[n - i:]) for i <= n, j(i) = i
A length qualifies when E(i) <= k_i; the subsequence answers with the most matched items i - E(i), then the smaller E(i);
the sequence answers with the subsequence of the largest i - d, then the smaller d, then the lower list position, as
(pattern, overlap = i, dist = d, start = n - j(i)), or (-1, 0, -1, n).  brute_* restate E and j by a textbook DP over every
suffix; tests/test_overlap_host.py holds the model against them."""
import numpy as np

import oracle

LEV, SUBS = 1, 2


def overlap_one(mode, p, r, k, o):
    """one subsequence, one sequence -> (i, d, j) or None"""
    p, r = bytes(p), bytes(r)
    m, n, best = len(p), len(r), None
    for i in range(o, m):
        ki = k * i // m
        if mode == LEV:
            d, j = oracle.expand(p[:i][::-1], r[::-1][:i + ki], ki)
            if d is None:
                continue
        else:
            if i > n:
                continue
            d, j = sum(a != b for a, b in zip(p[:i], r[n - i:])), i
            if d > ki:
                continue
        if best is None or (i - d, -d) > (best[0] - best[1], -best[1]):
            best = (i, d, j)
    return best


def per_pattern(mode, patterns, reads, k, o):
    """-> ones[read][pattern] = overlap_one"""
    return [[overlap_one(mode, p, r, k, o) for p in patterns] for r in reads]


def choose(ones, reads, n_pats=None):
    """per_pattern's answers (of the first n_pats patterns) -> (pattern int32, overlap int32, dist int32, start int64), one
    entry per read: the largest i - d, then the smaller d, then the lower list position"""
    n = len(reads)
    pattern, overlap = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    dist, start = np.full(n, -1, dtype=np.int32), np.array([len(r) for r in reads], dtype=np.int64)
    for s, r in enumerate(reads):
        best = None
        for q, one in enumerate(ones[s][:n_pats]):
            if one is not None and (best is None or (one[0] - one[1], -one[1]) > (best[1] - best[2], -best[2])):
                best = (q,) + one
        if best is not None:
            pattern[s], overlap[s], dist[s], start[s] = best[0], best[1], best[2], len(r) - best[3]
    return pattern, overlap, dist, start


def end_overlaps(mode, patterns, reads, k, o):
    return choose(per_pattern(mode, patterns, reads, k, o), reads)


def edit_distance(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(prev + (x != y), row[j] + 1, row[j - 1] + 1)
    return row[len(b)]


def brute_one(mode, p, r, k, o):
    """overlap_one from the definition alone: every suffix, a textbook DP"""
    p, r = bytes(p), bytes(r)
    m, n, best = len(p), len(r), None
    for i in range(o, m):
        if mode == LEV:
            per_suffix = [edit_distance(p[:i], r[n - j:]) for j in range(n + 1)]
            d = min(per_suffix)
            j = max(j for j in range(n + 1) if per_suffix[j] == d)
        else:
            if i > n:
                continue
            d, j = sum(a != b for a, b in zip(p[:i], r[n - i:])), i
        if d <= k * i // m and (best is None or (i - d, -d) > (best[0] - best[1], -best[1])):
            best = (i, d, j)
    return best
