"""What finding adapter prefixes at read ends costs: find_end_overlaps_batch on the device (DESIGN.md section 4;
profiles/r22_overlap.txt).

    python benchmarks/overlap_reads.py [--reads 4000000] [--read-len 150] [--reps 5] [--sample 20000]

Input: `--reads` synthetic reads of `--read-len` bytes as a FASTQ text made resident once (resident_records); about 30 % of
them end in a prefix of 3 .. 32 bytes of a 33-byte adapter with 0 .. 2 edits (substitutions, and for every eighth of them
one insertion or deletion).  For one adapter at k = 3 and for a panel of 8, in both modes:
  the kernels' span (Engine.overlap_ms: hipEvents around the launches of the list and the finish kernel), the C-ABI call
  (its own clock, the copy of the 8-byte rows included) and the public call (host clock around find_end_overlaps_batch).
Next to them
  (a) the kernels' span of fz_batch_search for the same adapter over the same batch: one streaming pass, the yardstick;
  (b) the per-read CPU route, oracle.expand in the model's loop (tests/overlap_model.py) over the first `--sample` reads,
      scaled to `--reads` and marked as scaled.
The device's arrays are compared with the model's on the sample (a tenth of it for the panel) before anything is timed.
1 round of warm-up, then the median and the min-max spread over `--reps` rounds.
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
from tests import overlap_model as om         # noqa: E402
from tests import workloads                   # noqa: E402
from ingest_reads import make_fastq           # noqa: E402

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
NEXT_BASE = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    NEXT_BASE[_a] = _b


def stat(v):
    return float(np.median(v)), min(v), max(v)


def plant(dna, adapter, share, seed):
    """Overwrite the ends of about `share` of the reads (in place) with adapter[:3 .. 32] carrying 0 .. 2 edits -> their rows."""
    rng = np.random.default_rng(seed)
    reads, width = dna.shape
    ad = np.frombuffer(adapter, dtype=np.uint8)
    which = np.flatnonzero(rng.random(reads) < share)
    lens = rng.integers(3, len(adapter), size=len(which))
    edits = rng.integers(0, 3, size=len(which))
    for n in range(3, len(adapter)):
        dna[which[lens == n], width - n:] = ad[:n]
    for e in (1, 2):                                        # substitutions: another base at a random place of the prefix
        rows, span = which[edits >= e], lens[edits >= e]
        cols = width - 1 - rng.integers(0, span)
        dna[rows, cols] = NEXT_BASE[dna[rows, cols]]
    for row, n in zip(which[::8].tolist(), lens[::8].tolist()):    # one insertion or deletion instead
        at = int(rng.integers(0, n))
        if (row ^ n) & 1:
            tail = np.concatenate([ad[:at], ad[at + 1:n + 1]])
        else:
            tail = np.concatenate([ad[:at], [ad[(at + 7) % len(ad)]], ad[at:n - 1]])
        dna[row, width - n:] = tail[:n]
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
    planted = plant(dna, ADAPTER, 0.30, 22)
    rng = np.random.default_rng(23)
    panel = [ADAPTER] + [workloads.dna(int(m), 100 + i).tobytes() for i, m in enumerate(rng.integers(20, 41, size=7))]
    eng = _native.default_engine()
    eng.set_timing(True)
    held = fa.resident_records(make_fastq(dna), engine=eng)
    sample = [dna[j].tobytes() for j in range(min(a.sample, a.reads))]
    print("end overlaps: %d reads x %d bytes, %d of them (%.1f %%) end in a prefix of 3 .. %d bytes of the %d-byte adapter with 0 .. 2 edits; "
          "%d rounds after 1 of warm-up" % (a.reads, a.read_len, len(planted), 100.0 * len(planted) / a.reads, len(ADAPTER) - 1, len(ADAPTER), a.reps))
    limits = {om.LEV: dict(max_l_dist=3), om.SUBS: dict(max_substitutions=3, max_insertions=0, max_deletions=0)}
    names = {om.LEV: "Levenshtein, k = 3", om.SUBS: "substitutions only, k = 3"}
    cpu_ms = {}
    for mode in (om.LEV, om.SUBS):
        for what, patterns, n_check in (("one adapter of 33", [ADAPTER], len(sample)), ("a panel of 8 (20 .. 40 bytes)", panel, len(sample) // 10)):
            res = fa.find_end_overlaps_batch(patterns, held, min_overlap=3, **limits[mode])       # (the warm-up)
            t0 = time.perf_counter()
            want = om.end_overlaps(mode, patterns, sample[:n_check], 3, 3)
            model_ms = (time.perf_counter() - t0) * 1e3
            for name, w in zip(("pattern", "overlap", "dist", "start"), want):
                assert np.array_equal(getattr(res, name)[:n_check], w), (names[mode], what, name)
            if len(patterns) == 1:
                cpu_ms[mode] = model_ms * a.reads / max(n_check, 1)
            kern, call, wall = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = fa.find_end_overlaps_batch(patterns, held, min_overlap=3, **limits[mode])
                wall.append((time.perf_counter() - t0) * 1e3)
                ms = eng.overlap_ms()
                kern.append(ms["kernels"])
                call.append(ms["call"])
            found = int((res.pattern >= 0).sum())
            print("%s, %s: %d reads with an overlap (equal to the model on the first %d reads)" % (names[mode], what, found, n_check))
            print("    kernels (%d launch%s + finish)   %9.3f ms [%9.3f, %9.3f]   %.3f ms per pattern"
                  % ((eng.stats()["filter_launches"], "" if eng.stats()["filter_launches"] == 1 else "es") + stat(kern) + (stat(kern)[0] / len(patterns),)))
            print("    fz_batch_end_overlaps             %9.3f ms [%9.3f, %9.3f]" % stat(call))
            print("    find_end_overlaps_batch           %9.3f ms [%9.3f, %9.3f]" % stat(wall))
            sys.stdout.flush()
    # (a) one streaming pass over the same batch
    for mode, native in ((om.LEV, _native.MODE_LEV), (om.SUBS, _native.MODE_SUBS)):
        eng.batch_search(held.handle, native, ADAPTER, 3)
        spans = []
        for _ in range(a.reps):
            eng.batch_search(held.handle, native, ADAPTER, 3)
            f, v, _d = eng.kernel_ms()
            spans.append(f + v)
        print("(a) fz_batch_search, the whole adapter, %s: kernels %9.3f ms [%9.3f, %9.3f] over %.0f MB"
              % ((names[mode],) + stat(spans) + (len(held.handle) / 1e6,)))
    # (b) the CPU route
    for mode in (om.LEV, om.SUBS):
        print("(b) the model's loop on the CPU, %s: %.0f ms for %d reads SCALED from %d reads"
              % (names[mode], cpu_ms[mode], a.reads, len(sample)))
    held.release()


if __name__ == "__main__":
    main()
