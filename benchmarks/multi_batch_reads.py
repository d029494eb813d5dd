"""A pattern list against millions of short reads: fz_batch_search_multi against the loop of fz_batch_search per pattern
(the table of profiles/r11_multi_batch.txt).

    python benchmarks/multi_batch_reads.py [--reads 4000000] [--read-len 150] [--reps 10] [--plants 64]
                                           [--counts 8,24,64] [--lengths 20,32] [--budgets lev:2,subs:2,subs:3]

Workload: `--reads` reads of `--read-len` bytes of workloads.dna (4 M x 150 = 600 MB), resident as one batch; per cell P
random DNA patterns of m characters, each planted `--plants` times (exact, 1 substitution, 1 deletion, 1 insertion in turn)
somewhere in the packed bytes — most copies inside one read, a few across a seam, as a real read set has them.
  pass   ONE fz_batch_search_multi call with FZ_MP_FORCE_PASS: every group of two or more patterns rides a pass
  loop   fz_batch_search once per pattern on the same handle (what the list cost before this call)
both raw, in the same process, alternating, after 3 rounds of warm-up; row streams are compared before anything is timed.
Per cell: the median and the min-max spread of the whole-call host clock (synchronous calls: each ends in the completion of
its kernels and the ordering of its rows) over `--reps` rounds, the kernels' own hipEvent spans (fz_stats: filter + verify,
summed over the loop's calls), and the host share = whole call - kernels (ordering P x rows by sequence).  The `rule` column
says what mp_worth_a_pass does with the list when nothing forces it.
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

MODES = {"lev": _native.MODE_LEV, "subs": _native.MODE_SUBS}


def run_loop(eng, h, mode, pats, k):
    out, kern = [], 0.0
    for p in pats:
        out.append(eng.batch_search(h, mode, p, k, reduced=False))
        f, v, _ = eng.kernel_ms()
        kern += f + v
    return out, kern


def run_pass(eng, h, mode, pats, k):
    out = eng.batch_search_multi(h, mode, pats, k, reduced=False)
    f, v, _ = eng.kernel_ms()
    return out, f + v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--plants", type=int, default=64)
    ap.add_argument("--counts", default="8,24,64")
    ap.add_argument("--lengths", default="20,32")
    ap.add_argument("--budgets", default="lev:2,subs:2,subs:3")
    a = ap.parse_args()
    counts = [int(x) for x in a.counts.split(",")]
    lengths = [int(x) for x in a.lengths.split(",")]
    budgets = [(b.split(":")[0], int(b.split(":")[1])) for b in a.budgets.split(",")]
    n = a.reads * a.read_len
    seq = workloads.dna(n, 20251018)
    pats = {}
    for m in lengths:
        arrs = [workloads.dna(m, 7000 + 100 * m + i) for i in range(max(counts))]
        for i, p in enumerate(arrs):
            workloads.plant_variants(seq, p, a.plants, 1100 + 64 * m + i)
        pats[m] = [p.tobytes() for p in arrs]
    blob = seq.tobytes()
    offs = np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.read_len)
    os.environ["FZ_MP_FORCE_PASS"] = "1"                               # (read when the library loads its switches)
    eng = _native.default_engine()
    lib = eng._lib
    eng.set_timing(True)
    h = eng.upload_batch(blob, offs)
    print("pattern lists over a batch of reads: %d reads x %d bytes of DNA (%.0f MB) resident, %d planted variants per pattern, "
          "raw rows, %d rounds per cell after 3 of warm-up, pass and loop alternating" % (a.reads, a.read_len, n / 1e6, a.plants, a.reps))
    t_end = time.perf_counter() + 0.3                                  # settle: clocks up, buffers grown
    while time.perf_counter() < t_end:
        eng.batch_search(h, _native.MODE_LEV, pats[lengths[0]][0], 2)
    print("%4s %3s %3s %3s | %9s %19s %9s %8s | %9s %19s %9s %8s | %7s %7s | %8s %6s | %s" % (
        "mode", "m", "k", "P", "pass ms", "[min, max]", "kernels", "host", "loop ms", "[min, max]", "kernels", "host",
        "ratio", "k-ratio", "rows", "passes", "rule"))
    for name, k in budgets:
        mode = MODES[name]
        for m in lengths:
            for P in counts:
                ps = pats[m][:P]
                ref, _ = run_loop(eng, h, mode, ps, k)
                got, _ = run_pass(eng, h, mode, ps, k)
                st = eng.stats()
                assert len(got) == P and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(got, ref)), "rows differ"
                assert st["verify_form"] == 5, "the list was meant to ride a pass"
                for _ in range(3):
                    run_loop(eng, h, mode, ps, k)
                    run_pass(eng, h, mode, ps, k)
                tl, tp, kl, kp = [], [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    _, kern = run_loop(eng, h, mode, ps, k)
                    tl.append((time.perf_counter() - t0) * 1e3)
                    kl.append(kern)
                    t0 = time.perf_counter()
                    _, kern = run_pass(eng, h, mode, ps, k)
                    tp.append((time.perf_counter() - t0) * 1e3)
                    kp.append(kern)
                os.environ.pop("FZ_MP_FORCE_PASS")                     # what the planner's rule does with this list
                lib.fz_debug_reload_switches()
                rule = "pass" if _native.multi_plan(ps, k, mode)[1] else "loop"
                os.environ["FZ_MP_FORCE_PASS"] = "1"
                lib.fz_debug_reload_switches()
                ml, mp, mkl, mkp = (float(np.median(x)) for x in (tl, tp, kl, kp))
                print("%4s %3d %3d %3d | %9.3f [%8.3f, %8.3f] %9.3f %8.3f | %9.3f [%8.3f, %8.3f] %9.3f %8.3f | %7.3f %7.3f | %8d %6d | %s" % (
                    name, m, k, P, mp, min(tp), max(tp), mkp, mp - mkp, ml, min(tl), max(tl), mkl, ml - mkl, mp / ml, mkp / mkl,
                    st["raw_matches"], st["filter_launches"], rule))
                sys.stdout.flush()
    h.release()


if __name__ == "__main__":
    main()
