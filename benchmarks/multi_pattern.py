"""Multi-pattern search against the parent's best form for the same job.

    python benchmarks/multi_pattern.py [--mib 1024] [--reps 30] [--mode lev|subs] [--force-pass]

Workload: `--mib` MiB of workloads.dna, resident.  P in {1, 4, 16, 64} random DNA patterns with a few planted variants
each, two regimes: m = 20, k = 2 (dense: 3 P / 4^6 of the offsets are n-gram hits) and m = 32, k = 2 (filter-bound).
  loop   the P patterns through the two-in-flight pipeline (lev_ngrams_begin / lev_ngrams_end), one search each
  multi  ONE lev_ngrams_multi call
in the same process, alternating, after a settle phase; row streams are compared before anything is timed.  Medians over
`--reps` repetitions and the min-max spread of each; the multi call's own kernel spans come from its hipEvents
(stats()["filter_ms"] / ["verify_ms"]: the group's two launches), to be held against a `rocprofv3 --kernel-trace --stats`
run of this script.  The hit list's cost is printed per case: every hit is 8 bytes written by the filter and read by the
verification.

--mode subs: the substitutions-only search (k substitutions, no insertions or deletions), regimes 20:2, 20:3, 23:3, 32:2 by
default.  loop = subs_ngrams per pattern, one synchronous call each, on the same handle (what the list cost before
subs_ngrams_multi); multi = ONE subs_ngrams_multi call.
--force-pass: every group of two or more patterns rides a pass whatever the planner's cost rule expects (FZ_MP_FORCE_PASS),
which is how the cells the rule gives to the loop are measured; the `rule` column says what the rule would have done.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuzzysearch_amd import _native           # noqa: E402
from tests import workloads                   # noqa: E402


def loop(eng, h, pats, k):
    out = []
    eng.lev_ngrams_begin(h, pats[0], k)
    for p in pats[1:]:
        eng.lev_ngrams_begin(h, p, k)
        out.append(eng.lev_ngrams_end(as_array=True))
    out.append(eng.lev_ngrams_end(as_array=True))
    return out


def loop_subs(eng, h, pats, k):
    return [eng.subs_ngrams(h, p, k, as_array=True) for p in pats]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--plants", type=int, default=8)
    ap.add_argument("--regimes", default=None, help="m:k,m:k,... (default 20:2,32:2; --mode subs: 20:2,20:3,23:3,32:2)")
    ap.add_argument("--mode", choices=("lev", "subs"), default="lev")
    ap.add_argument("--force-pass", action="store_true")
    ap.add_argument("--counts", default="1,4,16,64", help="numbers of patterns")
    a = ap.parse_args()
    subs = a.mode == "subs"
    if a.regimes is None:
        a.regimes = "20:2,20:3,23:3,32:2" if subs else "20:2,32:2"
    if a.force_pass:
        os.environ["FZ_MP_FORCE_PASS"] = "1"                           # (read when the library loads its switches)
    n = a.mib << 20
    regimes = [tuple(int(x) for x in r.split(":")) for r in a.regimes.split(",")]
    counts = [int(x) for x in a.counts.split(",")]
    seq = workloads.dna(n, 20250925)
    pats = {}
    for (m, k) in regimes:
        pats[(m, k)] = [workloads.dna(m, 5000 + 100 * m + i) for i in range(max(counts))]
        for i, p in enumerate(pats[(m, k)]):
            workloads.plant_variants(seq, p, a.plants, 900 + 64 * m + i)
        pats[(m, k)] = [p.tobytes() for p in pats[(m, k)]]
    eng = _native.default_engine()
    run_loop = loop_subs if subs else loop
    run_multi = eng.subs_ngrams_multi if subs else eng.lev_ngrams_multi
    mode = _native.MODE_SUBS if subs else _native.MODE_LEV
    h = eng.upload(seq)
    gib = n / float(1 << 30)
    print("multi-pattern search (%s%s): %d MiB of DNA resident, %d planted variants per pattern, %d repetitions per case, alternating"
          % ("substitutions only" if subs else "Levenshtein", ", every group forced onto a pass" if a.force_pass else "",
             a.mib, a.plants, a.reps))
    t_end = time.perf_counter() + 0.3                              # settle: clocks up, buffers grown
    while time.perf_counter() < t_end:
        (eng.subs_ngrams if subs else eng.lev_ngrams)(h, pats[regimes[0]][0], regimes[0][1])
    hdr = "%3s %3s %3s | %9s %19s | %9s %19s %8s | %7s | %10s %8s | %9s %9s | %s" % (
        "m", "k", "P", "loop ms", "[min, max]", "multi ms", "[min, max]", "ms/pat", "ratio", "hits", "rows", "filter ms", "verify ms",
        "hit list MB/GiB (written + read)")
    print(hdr)
    for (m, k) in regimes:
        for P in counts:
            ps = pats[(m, k)][:P]
            ref = run_loop(eng, h, ps, k)
            got = run_multi(h, ps, k, as_array=True)
            assert len(got) == P and all(np.array_equal(x, y) for x, y in zip(got, ref)), "row streams differ"
            st = eng.stats()
            for _ in range(3):
                run_loop(eng, h, ps, k)
                run_multi(h, ps, k, as_array=True)
            tl, tm, fms, vms = [], [], [], []
            for _ in range(a.reps):
                tl += timed(lambda: run_loop(eng, h, ps, k), 1)
                tm += timed(lambda: run_multi(h, ps, k, as_array=True), 1)
                s2 = eng.stats()
                fms.append(s2["filter_ms"])
                vms.append(s2["verify_ms"])
            ml, mm = float(np.median(tl)), float(np.median(tm))
            hits = st["ngram_hits"]
            rule = ""
            if a.force_pass:                                           # what the planner's rule does with this list
                os.environ.pop("FZ_MP_FORCE_PASS")
                eng._lib.fz_debug_reload_switches()
                rule = "   rule: pass" if _native.multi_plan(ps, k, mode)[1] else "   rule: loop"
                os.environ["FZ_MP_FORCE_PASS"] = "1"
                eng._lib.fz_debug_reload_switches()
            print("%3d %3d %3d | %9.3f [%8.3f, %8.3f] | %9.3f [%8.3f, %8.3f] %8.4f | %7.3f | %10d %8d | %9.3f %9.3f | %.1f%s%s" % (
                m, k, P, ml, min(tl), max(tl), mm, min(tm), max(tm), mm / P, mm / ml, hits, st["raw_matches"],
                float(np.median(fms)), float(np.median(vms)), 2 * 8 * hits / 1e6 / gib,
                "" if st["verify_form"] == 5 else "   (single route)", rule))
    h.release()


if __name__ == "__main__":
    main()
