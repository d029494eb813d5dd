"""Demultiplexing millions of short reads: fz_batch_assign against the route to the same answer without it
(the table of profiles/r12_assign.txt).

    python benchmarks/assign_reads.py [--reads 4000000] [--read-len 150] [--reps 10] [--plants 64] [--counts 8,64]
                                      [--cells lev:32:2,subs:32:2,subs:20:3] [--public-counts 8] [--public-reps 3]

Workload: the cells of benchmarks/multi_batch_reads.py — `--reads` reads of `--read-len` bytes of workloads.dna (4 M x 150 =
600 MB), resident as one batch; per cell P random DNA patterns of m characters, each planted `--plants` times (exact, 1
substitution, 1 deletion, 1 insertion in turn) somewhere in the packed bytes.  FZ_MP_FORCE_PASS for both routes: every list
rides passes.
  assign  ONE fz_batch_assign call: five arrays of one entry per read
  rows    ONE fz_batch_search_multi(reduced = 1) call plus a numpy reduction of its rows to the same five arrays (a lexsort
          by (read, dist, pattern, start, -end), the first row per read, a count of the other patterns at that distance)
in the same process, alternating, after 3 rounds of warm-up.  Before anything is timed pattern, dist and tied of the two
routes are compared, and (start, end) of `assign` against the same reduction of the RAW rows (reduced = 0: the position is
defined on the raw stream).  Per cell: the median and the min-max spread of the whole-call host clock over `--reps` rounds and
the kernels' own hipEvent spans (fz_stats: filter + verify; for `assign` the fold is part of verify).
The public calls, for the list sizes of `--public-counts` (P x reads lists of Match: 64 patterns over 4 M reads would be
256 M lists): find_best_matches_batch against find_near_matches_multi_batch plus the same reduction in Python over its lists.
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


def reduce_rows(rows, seq_of, bounds, n_seqs):
    """Rows of fz_batch_search_multi (all patterns' rows, pattern i at bounds[i] .. bounds[i + 1]) -> the five arrays."""
    pattern = np.full(n_seqs, -1, dtype=np.int32)
    dist = np.full(n_seqs, -1, dtype=np.int32)
    start = np.full(n_seqs, -1, dtype=np.int64)
    end = np.full(n_seqs, -1, dtype=np.int64)
    tied = np.zeros(n_seqs, dtype=bool)
    if len(rows):
        pat = np.repeat(np.arange(len(bounds) - 1, dtype=np.int32), np.diff(np.asarray(bounds, dtype=np.int64)))
        order = np.lexsort((-rows["end"], rows["start"], pat, rows["dist"], seq_of))
        which, first = np.unique(seq_of[order], return_index=True)
        best = order[first]
        pattern[which], dist[which], start[which], end[which] = pat[best], rows["dist"][best], rows["start"][best], rows["end"][best]
        other = (rows["dist"] == dist[seq_of]) & (pat != pattern[seq_of])
        tied[seq_of[other]] = True
    return pattern, dist, start, end, tied


def run_assign(eng, h, mode, pats, k):
    rows = eng.batch_assign(h, mode, pats, k)
    f, v, _ = eng.kernel_ms()
    have = rows["pattern"] >= 0
    out = (rows["pattern"], np.where(have, rows["dist"].astype(np.int32), -1), np.where(have, rows["start"].astype(np.int64), -1),
           np.where(have, rows["end"].astype(np.int64), -1), rows["tied"] != 0)
    return out, f + v


def run_rows(eng, h, mode, pats, k, n_seqs, reduced=True):
    ptr, seq_of, bounds = eng._batch_multi_call(h, mode, pats, k, reduced)
    f, v, _ = eng.kernel_ms()
    rows = _native._take_matches_array(eng._lib, ptr, bounds[-1])
    return reduce_rows(rows, seq_of, bounds, n_seqs), f + v


def public_rows(fa, pats, held, limits):
    """The parent's public route: find_near_matches_multi_batch, then the reduction over its lists of Match."""
    nested = fa.find_near_matches_multi_batch(pats, held, **limits)
    n = len(held)
    pattern, dist, tied = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=bool)
    for i, per in enumerate(nested):
        for j, ms in enumerate(per):
            if ms:
                d = min(x.dist for x in ms)
                if pattern[j] < 0 or d < dist[j]:
                    pattern[j], dist[j], tied[j] = i, d, False
                elif d == dist[j]:
                    tied[j] = True
    return pattern, dist, tied


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--plants", type=int, default=64)
    ap.add_argument("--counts", default="8,64")
    ap.add_argument("--cells", default="lev:32:2,subs:32:2,subs:20:3")
    ap.add_argument("--public-counts", default="8")
    ap.add_argument("--public-reps", type=int, default=3)
    a = ap.parse_args()
    counts = [int(x) for x in a.counts.split(",")]
    public_counts = [int(x) for x in a.public_counts.split(",") if x]
    cells = [(c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in a.cells.split(",")]
    n = a.reads * a.read_len
    seq = workloads.dna(n, 20251018)
    pats = {}
    for m in sorted(set(c[1] for c in cells)):
        arrs = [workloads.dna(m, 7000 + 100 * m + i) for i in range(max(counts))]
        for i, p in enumerate(arrs):
            workloads.plant_variants(seq, p, a.plants, 1100 + 64 * m + i)
        pats[m] = [p.tobytes() for p in arrs]
    blob = seq.tobytes()
    offs = np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.read_len)
    os.environ["FZ_MP_FORCE_PASS"] = "1"                               # (read when the library loads its switches)
    eng = _native.default_engine()
    eng.set_timing(True)
    h = eng.upload_batch(blob, offs)
    print("best pattern per read: %d reads x %d bytes of DNA (%.0f MB) resident, %d planted variants per pattern, %d rounds per cell "
          "after 3 of warm-up, assign and rows alternating" % (a.reads, a.read_len, n / 1e6, a.plants, a.reps))
    t_end = time.perf_counter() + 0.3                                  # settle: clocks up, buffers grown
    while time.perf_counter() < t_end:
        eng.batch_search(h, _native.MODE_LEV, pats[cells[0][1]][0], 2)
    print("C-ABI  %4s %3s %3s %3s | %9s %19s %9s | %9s %19s %9s | %7s | %8s %8s %6s" % (
        "mode", "m", "k", "P", "assign ms", "[min, max]", "kernels", "rows ms", "[min, max]", "kernels", "ratio", "assigned", "tied", "passes"))
    for name, m, k in cells:
        mode = MODES[name]
        for P in counts:
            ps = pats[m][:P]
            got, _ = run_assign(eng, h, mode, ps, k)
            st = eng.stats()
            assert st["verify_form"] == 5, "the list was meant to ride a pass"
            red, _ = run_rows(eng, h, mode, ps, k, a.reads)
            raw, _ = run_rows(eng, h, mode, ps, k, a.reads, reduced=False)
            for x in (0, 1, 4):
                assert np.array_equal(got[x], red[x]) and np.array_equal(got[x], raw[x]), "pattern, dist or tied differ"
            assert np.array_equal(got[2], raw[2]) and np.array_equal(got[3], raw[3]), "positions differ from the raw rows' reduction"
            for _ in range(3):
                run_assign(eng, h, mode, ps, k)
                run_rows(eng, h, mode, ps, k, a.reads)
            ta, tr, ka, kr = [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, kern = run_assign(eng, h, mode, ps, k)
                ta.append((time.perf_counter() - t0) * 1e3)
                ka.append(kern)
                t0 = time.perf_counter()
                _, kern = run_rows(eng, h, mode, ps, k, a.reads)
                tr.append((time.perf_counter() - t0) * 1e3)
                kr.append(kern)
            ma, mr, mka, mkr = (float(np.median(x)) for x in (ta, tr, ka, kr))
            print("C-ABI  %4s %3d %3d %3d | %9.3f [%8.3f, %8.3f] %9.3f | %9.3f [%8.3f, %8.3f] %9.3f | %7.3f | %8d %8d %6d" % (
                name, m, k, P, ma, min(ta), max(ta), mka, mr, min(tr), max(tr), mkr, ma / mr,
                int((got[0] >= 0).sum()), int(got[4].sum()), st["filter_launches"]))
            sys.stdout.flush()
    h.release()
    if public_counts:
        import fuzzysearch_amd as fa
        reads = [blob[i:i + a.read_len] for i in range(0, n, a.read_len)]
        held = fa.resident_batch(reads)
        print("public %4s %3s %3s %3s | %9s %19s | %9s %19s | %7s   (%d rounds after 1 of warm-up)" % (
            "mode", "m", "k", "P", "best ms", "[min, max]", "lists ms", "[min, max]", "ratio", a.public_reps))
        for name, m, k in cells:
            limits = dict(max_l_dist=k) if name == "lev" else dict(max_substitutions=k, max_insertions=0, max_deletions=0)
            for P in public_counts:
                ps = pats[m][:P]
                best = fa.find_best_matches_batch(ps, held, **limits)
                want = public_rows(fa, ps, held, limits)
                assert np.array_equal(best.pattern, want[0]) and np.array_equal(best.dist, want[1]) and np.array_equal(best.tied, want[2])
                tb, tl = [], []
                for _ in range(a.public_reps):
                    t0 = time.perf_counter()
                    fa.find_best_matches_batch(ps, held, **limits)
                    tb.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    public_rows(fa, ps, held, limits)
                    tl.append((time.perf_counter() - t0) * 1e3)
                print("public %4s %3d %3d %3d | %9.3f [%8.3f, %8.3f] | %9.1f [%8.1f, %8.1f] | %7.4f" % (
                    name, m, k, P, float(np.median(tb)), min(tb), max(tb), float(np.median(tl)), min(tl), max(tl),
                    float(np.median(tb)) / float(np.median(tl))))
                sys.stdout.flush()
        held.release()


if __name__ == "__main__":
    main()
