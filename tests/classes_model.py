"""Brute-force model of the class distance (fuzzysearch_amd/classes.py), shared by the host and the GPU tests of symbol
classes.  Nothing here knows about hashes, blocks' tables or dwords: a 256 x 256 acceptance table and numpy."""
import numpy as np

from fuzzysearch_amd import _native


def accept_table(classes):
    """A[c, t]: does pattern byte c match sequence byte t?  t == c, or c is a key and t is in its set."""
    A = np.eye(256, dtype=bool)
    for key, members in (classes or {}).items():
        c = key if isinstance(key, int) else key[0]
        for t in bytes(members):
            A[c, t] = True
    return A


def window_matches(p, text, A):
    """-> bool array [number of windows, len(p)]: position q of the window at i matches (no windows: shape (0, m))."""
    m, n = len(p), len(text)
    if m == 0 or n < m:
        return np.zeros((0, m), dtype=bool)
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(t, m)
    return A[np.frombuffer(bytes(p), dtype=np.uint8)[None, :], win]


def windows_within(p, text, k, A):
    """W: [(start, dist)] of every window of len(p) bytes whose class distance is <= k, by start."""
    acc = window_matches(p, text, A)
    dist = len(p) - acc.sum(axis=1)
    return [(int(i), int(dist[i])) for i in np.nonzero(dist <= k)[0]]


def raw_rows(p, text, k, A):
    """The raw stream of one pattern: (start, end, dist, block) for every window within k and every n-gram block
    [g * L, g * L + L) of the pattern (L = len(p) // (k + 1)) that the window class-matches exactly; by (block, start).
    (window_matches() column by column - does text byte i + q match pattern position q? - summed and and-ed as vectors over
    the windows, without the [windows, len(p)] array: the seam sweeps run this over texts of megabytes.)"""
    p = bytes(p)
    m, n = len(p), len(text)
    if m == 0 or n < m:
        return []
    L = m // (k + 1)
    nw = n - m + 1
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    accepted = {c: A[c][t] for c in set(p)}                 # per pattern symbol: which text bytes it matches
    matches = np.zeros(nw, dtype=np.int32)
    for q, c in enumerate(p):
        matches += accepted[c][q:q + nw]
    dist = m - matches
    within = dist <= k
    rows = []
    for g in range(m // L):
        ok = within.copy()
        for q in range(g * L, g * L + L):
            ok &= accepted[p[q]][q:q + nw]
        rows += [(int(i), int(i) + m, int(dist[i]), g) for i in np.nonzero(ok)[0]]
    return rows


def best_of_groups(p, text, k, A):
    """The public value: the raw stream through the library's host function fz_group_best -> [(start, end, dist)], in the
    group-list order that function gives the stream (the order of the substitutions-only calls without classes)."""
    raw = raw_rows(p, text, k, A)
    return [tuple(r)[:3] for r in _native.group_best(raw)] if raw else []


def best_of_windows(p, text, k, A):
    """The same from W itself, every window once, by start: the same matches (the overlap groups and the best of each do
    not depend on the order or on a window appearing once per block), possibly in another order -> sorted."""
    w = [(s, s + len(p), d, -1) for s, d in windows_within(p, text, k, A)]
    return sorted(tuple(r)[:3] for r in _native.group_best(w)) if w else []


def assignment(patterns, reads, k, A):
    """The reduction find_best_matches_batch documents, over W of every (pattern, read): per read (pattern, dist, tied,
    start, end) — the smallest distance, the lowest list position that reaches it, whether another position reaches it
    too, and that pattern's window at that distance with the smallest start; (-1, -1, False, -1, -1) when none matches."""
    out = []
    for r in reads:
        best = []                                         # per pattern that matches: (dist, position, start)
        for i, p in enumerate(patterns):
            w = windows_within(p, r, k, A)
            if w:
                d = min(x[1] for x in w)
                best.append((d, i, min(s for s, dd in w if dd == d)))
        if not best:
            out.append((-1, -1, False, -1, -1))
            continue
        d, i, s = min(best)
        out.append((i, d, sum(1 for b in best if b[0] == d) > 1, s, s + len(patterns[i])))
    return out
