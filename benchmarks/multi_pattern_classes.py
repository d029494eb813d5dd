"""IUPAC pattern lists on the multi-pattern pass: the class call against what a caller had to do without it, the same list
expanded into all its concrete spellings (the table of profiles/r16_multi_pattern_classes.txt).

    python benchmarks/multi_pattern_classes.py [--mib 1024] [--reps 5] [--plants 32]

Workload: `--mib` MiB of workloads.dna, resident; two lists of 16 patterns, every pattern planted `--plants` times in one of
its spellings (exact and with one substitution; the planted deletions and insertions do not match).
  (a) guides   16 x (20 random bases + NGG), k = 3: L = 5, the NGG tail lies behind the last n-gram block and costs no table
               entry.  Expanded: AGG, CGG, GGG, TGG, 64 patterns.
  (b) primers  16 x 24 bases with two two-base letters (R, Y, S, W, K, M) inside hashed block bytes, k = 2: L = 8, 7 table
               entries per pattern instead of 3.  Expanded: 64 patterns.
Per cell, at the C-ABI:
  classes   ONE fz_subs_ngrams_multi_best_cls call over the 16 patterns
  expanded  ONE fz_subs_ngrams_multi_best call over the 64 spellings, planned as the library plans it
Before anything is timed the RAW streams of the two routes are compared: per source pattern the windows (start, dist) of the
class call against the windows of its spellings merged (the smallest distance per start: on a text of bases alone that is the
class distance), and the reduced rows of the class call against fz_group_best of those merged windows.  Then `--reps` rounds,
alternating, after one round of warm-up: the median and the min-max spread of the whole-call host clock and of the kernels'
own hipEvent spans (fz_stats: filter + verify).
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fuzzysearch_amd as fa                  # noqa: E402
from fuzzysearch_amd import _native, classes  # noqa: E402
from tests import workloads                   # noqa: E402

IUPAC = fa.IUPAC_DNA
TWO_BASE = b"RYSWKM"


def spellings(p):
    return [bytes(s) for s in itertools.product(*[IUPAC.get(c, bytes([c])) for c in p])]


def guides(rng):
    return [workloads.dna(20, int(rng.integers(1 << 30))).tobytes() + b"NGG" for _ in range(16)]


def primers(rng):
    out = []
    for _ in range(16):
        p = bytearray(workloads.dna(24, int(rng.integers(1 << 30))).tobytes())
        p[int(rng.integers(0, 4))] = TWO_BASE[int(rng.integers(6))]              # block 0, bytes 0 .. 3
        p[8 + int(rng.integers(5, 8))] = TWO_BASE[int(rng.integers(6))]          # block 1, bytes 5 .. 7
        out.append(bytes(p))
    return out


def windows(rows):
    """Raw rows (one per window and matching block) -> {start: dist}."""
    return dict(zip(rows["start"].tolist(), rows["dist"].tolist()))


def timed(fn, eng):
    t0 = time.perf_counter()
    fn()
    ms = (time.perf_counter() - t0) * 1e3
    f, v, _ = eng.kernel_ms()
    return ms, f + v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plants", type=int, default=32)
    a = ap.parse_args()
    n = a.mib << 20
    rng = np.random.default_rng(20261019)
    cells = [("guides 20+NGG", 3, guides(rng)), ("primers 24, 2 letters", 2, primers(rng))]
    seq = workloads.dna(n, 20251018)
    for ci, (_, _, pats) in enumerate(cells):
        for i, p in enumerate(pats):
            sp = spellings(p)
            workloads.plant_variants(seq, np.frombuffer(sp[i % len(sp)], dtype=np.uint8), a.plants, 9000 + 100 * ci + i)
    tables = classes.class_tables(IUPAC)
    eng = _native.default_engine()
    eng.set_timing(True)
    h = eng.upload(seq)
    del seq
    print("IUPAC lists on the multi-pattern pass: %d MiB of DNA resident, %d planted variants per pattern, median [min, max] of %d rounds "
          "after 1 of warm-up, classes and expanded alternating; host clock of the whole call, ms (kernels: hipEvent spans)" % (a.mib, a.plants, a.reps))
    print("%-22s %2s | %3s %7s %6s | %9s %21s %9s | %3s %6s | %9s %21s %9s | %6s | %6s" % (
        "cell", "k", "P", "entries", "passes", "classes", "[min, max]", "kernels", "P", "passes", "expanded", "[min, max]", "kernels", "ratio", "rows"))
    for name, k, pats in cells:
        exp, source = [], []
        for i, p in enumerate(pats):
            for s in spellings(p):
                exp.append(s)
                source.append(i)
        _, per_pat, _ = _native.multi_plan_classes(pats, k, tables)
        raw_c = eng.subs_ngrams_multi_classes(h, pats, k, tables, as_array=True)
        raw_e = eng.subs_ngrams_multi(h, exp, k, as_array=True)
        best_c = eng.subs_ngrams_multi_classes(h, pats, k, tables, best=True, as_array=True)
        passes_c = eng.stats()["filter_launches"]
        eng.subs_ngrams_multi_best(h, exp, k, as_array=True)
        passes_e = eng.stats()["filter_launches"]
        n_rows = 0
        for i in range(len(pats)):
            merged = {}
            for j, rows in enumerate(raw_e):
                if source[j] == i:
                    for s, d in windows(rows).items():
                        merged[s] = min(d, merged.get(s, d))
            assert windows(raw_c[i]) == merged, "pattern %d: the class call and its expansion disagree" % i
            m = len(pats[i])
            want = _native.group_best([(s, s + m, d, -1) for s, d in sorted(merged.items())]) if merged else []
            assert sorted(tuple(r)[:3] for r in best_c[i].tolist()) == sorted(tuple(r)[:3] for r in want), "pattern %d: reduced rows differ" % i
            n_rows += len(merged)
        run_c = lambda: eng._multi_call("fz_subs_ngrams_multi_best", h, pats, k, tables)
        run_e = lambda: eng._multi_call("fz_subs_ngrams_multi_best", h, exp, k)

        def once(run):
            box = []
            ms, kern = timed(lambda: box.append(run()), eng)
            eng._lib.fz_free(box[0][0])
            return ms, kern
        once(run_c), once(run_e)
        tc, te = [], []
        for _ in range(a.reps):
            tc.append(once(run_c))
            te.append(once(run_e))
        mc, me = float(np.median([x[0] for x in tc])), float(np.median([x[0] for x in te]))
        print("%-22s %2d | %3d %7d %6d | %9.3f [%9.3f, %9.3f] %9.3f | %3d %6d | %9.3f [%9.3f, %9.3f] %9.3f | %6.3f | %6d" % (
            name, k, len(pats), sum(per_pat), passes_c, mc, min(x[0] for x in tc), max(x[0] for x in tc), float(np.median([x[1] for x in tc])),
            len(exp), passes_e, me, min(x[0] for x in te), max(x[0] for x in te), float(np.median([x[1] for x in te])), mc / me, n_rows))
        sys.stdout.flush()
    h.release()


if __name__ == "__main__":
    main()
