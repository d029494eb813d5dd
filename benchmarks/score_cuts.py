"""What quality trimming and poly-A trimming positions cost: quality_cuts and poly_tail_cuts on the device (DESIGN.md
section 4; profiles/r24_score_cuts.txt).

    python benchmarks/score_cuts.py [--reads 4000000] [--read-len 150] [--reps 5] [--sample 20000]

Input: `--reads` synthetic reads of `--read-len` bytes with a quality column as a FASTQ text made resident once
(resident_records, lines 1 and 3).
  (a) quality_cuts, 3' at cutoff 20: qualities of 30 .. 40 whose last 0 .. 40 bytes degrade to 2 .. 19;
  (b) poly_tail_cuts: about 30 % of the reads end in a poly-A tail of 5 .. 60 bytes with 10 % other bases.
Both are compared with the model (tests/cuts_model.py) on the first `--sample` reads before anything is timed.  Per cell:
  the kernel's span (Engine.cuts_ms: hipEvents around the launch), the four parts of fz_debug_cuts_ms (tables up, kernel,
  rows back, the whole C-ABI call), the public call (host clock), and the per-read Python route — the model's loop over
  the sample's sequences, scaled to `--reads` and marked as scaled.
Next to each kernel time: the gather kernel of a plain fz_batch_derive over the same batch in the same run (every byte read
once and written once), the yardstick.  1 round of warm-up, then the median and the min-max spread over `--reps` rounds.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fuzzysearch_amd import _native           # noqa: E402
from tests import cuts_model as cm            # noqa: E402
from tests import workloads                   # noqa: E402


def stat(v):
    return float(np.median(v)), min(v), max(v)


def make_fastq(dna, quals):
    """reads x read_len bases and qualities -> the FASTQ text: records of one width, '@r' + 8 digits as header."""
    reads, read_len = dna.shape
    width = 11 + read_len + 3 + read_len + 1
    rec = np.empty((reads, width), dtype=np.uint8)
    rec[:, 0], rec[:, 1] = ord('@'), ord('r')
    idx = np.arange(reads, dtype=np.int64)
    for d in range(8):
        rec[:, 9 - d] = ord('0') + (idx // 10 ** d) % 10
    rec[:, 10] = 10
    rec[:, 11:11 + read_len] = dna
    at = 11 + read_len
    rec[:, at], rec[:, at + 1], rec[:, at + 2] = 10, ord('+'), 10
    rec[:, at + 3:at + 3 + read_len] = quals
    rec[:, width - 1] = 10
    return rec.tobytes()


def degrading_quals(reads, read_len, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(30, 41, size=(reads, read_len), dtype=np.uint8)
    low = rng.integers(2, 20, size=(reads, read_len), dtype=np.uint8)
    tail = rng.integers(0, 41, size=reads)
    bad = np.arange(read_len)[None, :] >= (read_len - tail)[:, None]
    q[bad] = low[bad]
    return q + 33, tail


def plant_tails(dna, share, seed):
    """Overwrite the ends of about `share` of the reads (in place) with 5 .. 60 'A' of which 10 % are another base -> their rows"""
    rng = np.random.default_rng(seed)
    reads, width = dna.shape
    which = np.flatnonzero(rng.random(reads) < share)
    lens = rng.integers(5, 61, size=len(which))
    tail = np.arange(width)[None, :] >= (width - lens)[:, None]
    other = rng.random((len(which), width)) < 0.10
    rows = dna[which]
    rows[tail & ~other] = ord('A')
    rows[tail & other] = np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, size=int((tail & other).sum()))]
    dna[which] = rows
    return which


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=20000)
    a = ap.parse_args()
    import fuzzysearch_amd as fa
    dna = workloads.dna(a.reads * a.read_len, 20251021).reshape(a.reads, a.read_len)
    tails = plant_tails(dna, 0.30, 24)
    quals, low = degrading_quals(a.reads, a.read_len, 25)
    eng = _native.default_engine()
    eng.set_timing(True)
    bases, qual = fa.resident_records(make_fastq(dna, quals), engine=eng, lines=(1, 3))
    n_check = min(a.sample, a.reads)
    print("score cuts: %d reads x %d bytes with qualities; the last 0 .. 40 qualities of every read degrade (mean %.1f); %d reads (%.1f %%) "
          "end in a poly-A tail of 5 .. 60 bytes with 10 %% other bases; %d rounds after 1 of warm-up"
          % (a.reads, a.read_len, float(low.mean()), len(tails), 100.0 * len(tails) / a.reads, a.reps))
    cells = (("(a) quality_cuts, 3' at cutoff 20", qual, quals, lambda h: fa.quality_cuts(h, 20), lambda r: cm.cut3(r, cm.quality_table(20), True)),
             ("(b) poly_tail_cuts, 1 / -2, miss rate 1 / 5", bases, dna, lambda h: fa.poly_tail_cuts(h), lambda r: cm.cut3(r, cm.poly_table(), False, (1, 5))))
    for name, held, raw, call, model in cells:
        res = call(held)                                     # (the warm-up)
        sample = [raw[j].tobytes() for j in range(n_check)]
        t0 = time.perf_counter()
        want = np.array([model(r) for r in sample], dtype=np.int64)
        cpu_ms = (time.perf_counter() - t0) * 1e3 * a.reads / max(n_check, 1)
        assert np.array_equal(res.end[:n_check], want) and not res.start[:n_check].any(), name
        parts, wall = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = call(held)
            wall.append((time.perf_counter() - t0) * 1e3)
            parts.append(eng.cuts_ms())
        gather = []
        held.derive().release()
        for _ in range(a.reps):
            held.derive().release()
            gather.append(eng.derive_ms()["gather"])
        cut = int((res.end < a.read_len).sum())
        print("%s: %d reads cut, %.1f bytes a read (equal to the model on the first %d reads)" % (name, cut, float((a.read_len - res.end).mean()), n_check))
        print("    kernel (1 launch)                 %9.3f ms [%9.3f, %9.3f]" % stat([p["kernels"] for p in parts]))
        print("    fz_batch_derive's gather kernel   %9.3f ms [%9.3f, %9.3f]   the same batch, every byte read and written once" % stat(gather))
        print("    tables to the device              %9.3f ms [%9.3f, %9.3f]" % stat([p["tables_h2d"] for p in parts]))
        print("    rows to the host                  %9.3f ms [%9.3f, %9.3f]" % stat([p["rows_d2h"] for p in parts]))
        print("    fz_batch_score_cuts               %9.3f ms [%9.3f, %9.3f]" % stat([p["call"] for p in parts]))
        print("    the public call                   %9.3f ms [%9.3f, %9.3f]" % stat(wall))
        print("    the model's loop on the CPU       %9.0f ms for %d reads SCALED from %d reads" % (cpu_ms, a.reads, n_check))
        sys.stdout.flush()
    bases.release()
    qual.release()


if __name__ == "__main__":
    main()
