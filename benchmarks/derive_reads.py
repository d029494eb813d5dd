"""What acting on a search result costs: derive_batch on the device against cutting the reads in Python and uploading them
again (the table of profiles/r18_derive.txt).

    python benchmarks/derive_reads.py [--reads 4000000] [--read-len 150] [--reps 5] [--base-reps 2]

Input: the ingest benchmark's, `--reads` synthetic reads of `--read-len` bytes held by resident_records.
  1. the plain gather next to the ingest's: resident_records' own spans (Engine.records_ms) and the identity derive, whose
     gather is the same kernel, fz_rec_gather_kernel, over the packed bytes instead of the FASTQ text;
  2. the C-ABI call (Engine.derive_batch) split by the engine's own spans (Engine.derive_ms: hipEvents on the stream around
     the tables' copies, measure + scan, the gather; the host clock around the D2H of ends[], started once the gather has
     finished, so the four spans do not overlap and what is left of the call is the host's) for a trim (ends only), a
     1-in-8 selection and the reverse complement;
  3. the four gather instances over the same identity tables, GB/s of bytes read + written against the 8 TB/s peak, and the
     ratio of each to the plain one of the same run;
  4. the public calls against the Python route they replace: resident_batch([s[a:b] ...]) over a list of the reads that
     already exists, s[::-1].translate(t) for the reverse complement.
Every derived batch is compared with the Python route's (packed bytes and ends) before anything is timed.  1 round of
warm-up, then the median and the min-max spread over `--reps` rounds (`--base-reps` for the Python route).
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
from tests import workloads                   # noqa: E402
from ingest_reads import make_fastq           # noqa: E402

PEAK_GBS = 8000.0


def stat(v):
    return float(np.median(v)), min(v), max(v)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stat(out)


def abi_rounds(eng, handle, reps, **kw):
    """-> (walls, spans, packed bytes) of `reps` Engine.derive_batch calls after one of warm-up, each handle released."""
    eng.derive_batch(handle, **kw).release()
    walls, spans, packed = [], [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        h = eng.derive_batch(handle, **kw)
        walls.append((time.perf_counter() - t0) * 1e3)
        spans.append(eng.derive_ms())
        packed = len(h)
        h.release()
    return walls, spans, packed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2)
    a = ap.parse_args()
    import fuzzysearch_amd as fa
    dna = workloads.dna(a.reads * a.read_len, 20251019).reshape(a.reads, a.read_len)
    data = make_fastq(dna)
    eng = _native.default_engine()
    eng.set_timing(True)
    rnd = np.random.RandomState(18)
    ends = rnd.randint(a.read_len * 2 // 3, a.read_len + 1, size=a.reads).astype(np.uint64)
    mask = np.zeros(a.reads, dtype=bool)
    mask[::8] = True
    index = np.flatnonzero(mask).astype(np.uint32)
    table = fa.DNA_COMPLEMENT
    print("derive: %d reads x %d bytes held by resident_records (%.0f MB of reads); %d rounds after 1 of warm-up (%d for the Python route)"
          % (a.reads, a.read_len, dna.size / 1e6, a.reps, a.base_reps))

    # -- 1. the ingest's spans, for the same session's comparison
    fa.resident_records(data).release()
    rec = []
    for _ in range(a.reps):
        fa.resident_records(data).release()
        rec.append(eng.records_ms())
    held = fa.resident_records(data)
    reads = list(held.sequences)
    print("resident_records in this session: call %.1f ms [%.1f, %.1f], its splitting kernels (count, scan, lines, measure, scan, gather) summed %.3f ms [%.3f, %.3f]"
          % (stat([r["call"] for r in rec]) + stat([r["kernels"] for r in rec])))

    # -- before anything is timed: the three derived batches against the Python route's
    routes = {
        "trim": (dict(ends=ends), lambda: [s[:e] for s, e in zip(reads, ends.tolist())]),
        "select 1 in 8": (dict(index=index), lambda: [s for s, m in zip(reads, mask.tolist()) if m]),
        "reverse complement": (dict(reverse=True, translate=table), lambda: [s[::-1].translate(table) for s in reads]),
    }
    for name, (kw, python) in routes.items():
        want = fa.resident_batch(python())
        got = eng.derive_batch(held.handle, **kw)
        assert eng.batch_bytes(got) == eng.batch_bytes(want.handle), name
        assert np.array_equal(eng.batch_tables(got)[1], eng.batch_tables(want.handle)[1]), name
        got.release()
        want.release()
    print("the three derived batches equal the Python route's (packed bytes and ends)")
    sys.stdout.flush()

    # -- 2. the C-ABI call, split
    for name, (kw, _python) in routes.items():
        walls, spans, packed = abi_rounds(eng, held.handle, a.reps, **kw)
        print("Engine.derive_batch, %s (%.0f MB packed)  %10.2f ms [%9.2f, %9.2f]" % ((name, packed / 1e6) + stat(walls)))
        for key, label in (("tables_h2d", "tables up (H2D)"), ("measure_scan", "measure + scan"), ("gather", "gather"),
                           ("ends_d2h", "ends[] back (D2H, host clock)"), ("call", "the C-ABI call, whole")):
            print("      %-32s %10.3f ms [%9.3f, %9.3f]" % ((label,) + stat([s[key] for s in spans])))
        rest = [s["call"] - s["tables_h2d"] - s["measure_scan"] - s["gather"] - s["ends_d2h"] for s in spans]
        print("      %-32s %10.3f ms [%9.3f, %9.3f]" % (("host remainder of the call",) + stat(rest)))
        g = float(np.median([s["gather"] for s in spans]))
        print("      gather: %.0f GB/s of bytes read + written = %.1f %% of %.0f GB/s" % (2 * packed / g / 1e6, 2 * packed / g / 1e6 / PEAK_GBS * 100, PEAK_GBS))
        sys.stdout.flush()

    # -- 3. the four gather instances over the identity tables
    plain = None
    for name, kw in (("plain (fz_rec_gather_kernel)", dict()), ("REV", dict(reverse=True)), ("XLAT", dict(translate=table)),
                     ("REV + XLAT", dict(reverse=True, translate=table))):
        _walls, spans, packed = abi_rounds(eng, held.handle, a.reps, **kw)
        g = stat([s["gather"] for s in spans])
        plain = plain or g[0]
        print("gather, identity tables, %-30s %8.3f ms [%8.3f, %8.3f]  %6.0f GB/s = %4.1f %% of peak   x %.2f of plain"
              % ((name,) + g + (2 * packed / g[0] / 1e6, 2 * packed / g[0] / 1e6 / PEAK_GBS * 100, g[0] / plain)))
    sys.stdout.flush()

    # -- 4. the public calls against what they replace
    for name, (kw, python) in routes.items():
        if "index" in kw:
            kw = dict(index=mask)

        def device():
            held.derive(**kw).release()

        def host():
            fa.resident_batch(python()).release()

        device()
        d = timed(device, a.reps)
        h = timed(host, a.base_reps)
        print("%-20s reads.derive(...) %9.2f ms [%9.2f, %9.2f]   resident_batch([...]) %9.1f ms [%9.1f, %9.1f]   ratio %.0f"
              % ((name,) + d + h + (h[0] / d[0],)))
        sys.stdout.flush()
    held.release()


if __name__ == "__main__":
    main()
