"""The definition of find_score_cuts_batch in plain Python: where the running sum of a table of scores, taken from a read's
end, peaks.

For a read r of n bytes, a table w of 256 signed scores, a flag `stop` and an optional miss rate (num, den) — a miss is a
byte with w < 0 —

    cut3(r):  s = best = miss = 0; cut = n
              for i = n - 1 down to 0:
                  s += w[r[i]]; miss += (w[r[i]] < 0)
                  if stop and s < 0: break
                  if s > best and (no rate or miss * den <= num * (n - i)): best = s; cut = i
              return cut                       # in [0, n]; n = nothing cut
    cut5(r) = n - cut3(reversed r)             # in [0, n]; 0 = nothing cut

The comparison is strict, so of equal peaks the one nearest the end wins; a read of length 0 gives (0, 0); when both sides
are asked for and start >= end, both are 0.  The rate applies to the sides that do not stop.  This model is the definition:
the integer rate test is the project's own.  brute_cut3 restates it as an arg-max over prefix sums in numpy;
tests/test_cuts_host.py holds the model against it."""
import numpy as np


def cut3(r, w, stop, rate=None):
    r = bytes(r)
    n = len(r)
    s = best = miss = 0
    cut = n
    for i in range(n - 1, -1, -1):
        s += w[r[i]]
        miss += w[r[i]] < 0
        if stop and s < 0:
            break
        if s > best and (rate is None or miss * rate[1] <= rate[0] * (n - i)):
            best, cut = s, i
    return cut


def cut5(r, w, stop, rate=None):
    r = bytes(r)
    return len(r) - cut3(r[::-1], w, stop, rate)


def cuts_one(r, w3, w5, stop3=True, stop5=True, rate=None):
    """-> (start, end) of one read; w3 / w5: a table or None for a side not asked for; the rate is in force on the sides that
    do not stop"""
    n = len(r)
    start = 0 if w5 is None else cut5(r, w5, stop5, None if stop5 else rate)
    end = n if w3 is None else cut3(r, w3, stop3, None if stop3 else rate)
    if w3 is not None and w5 is not None and start >= end:
        start = end = 0
    return start, end


def score_cuts(reads, w3, w5, stop3=True, stop5=True, rate=None):
    """-> (start int64, end int64), one entry per read"""
    rows = [cuts_one(r, w3, w5, stop3, stop5, rate) for r in reads]
    return (np.array([a for a, _ in rows], dtype=np.int64), np.array([b for _, b in rows], dtype=np.int64))


def quality_table(cutoff, base=33):
    return [cutoff - (b - base) for b in range(256)]


def poly_table(base=b"A", hit=1, miss=-2):
    w = [miss] * 256
    w[base[0]] = hit
    return w


def brute_cut3(r, w, stop, rate=None):
    """cut3 from the definition written as prefix sums of the reversed read: S[t] = the sum of the last t + 1 scores, M[t]
    the misses among them.  With `stop` only the t in front of the first negative S count.  The cut is n - 1 - t for the
    FIRST t (nearest the end) whose S[t] is the maximum over the allowed t, if that maximum is above 0."""
    r = np.frombuffer(bytes(r), dtype=np.uint8)
    n = len(r)
    if n == 0:
        return 0
    wv = np.asarray(w, dtype=np.int64)[r[::-1]]
    S, M = np.cumsum(wv), np.cumsum(wv < 0)
    ok = np.ones(n, dtype=bool)
    if stop:
        neg = np.flatnonzero(S < 0)
        if neg.size:
            ok[neg[0]:] = False
    if rate is not None:
        # (the loop's `best` moves on accepted positions only, so the answer is the arg-max over them)
        ok &= M * rate[1] <= rate[0] * np.arange(1, n + 1)
    if not ok.any():
        return n
    masked = np.where(ok, S, np.iinfo(np.int64).min)
    t = int(np.argmax(masked))                               # (argmax: the first of equal maxima)
    return n - 1 - t if masked[t] > 0 else n
