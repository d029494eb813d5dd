"""How millions of short reads get to the device: resident_records against splitting the file in Python
(the table of profiles/r13_ingest.txt).

    python benchmarks/ingest_reads.py [--reads 4000000] [--read-len 150] [--reps 5] [--base-reps 3] [--patterns 8] [--plants 64]

Input: `--reads` synthetic reads of `--read-len` bytes of workloads.dna as a FASTQ text made here (4 M x 150: 1.3 GB).
  (a) split   the route without resident_records: data.split(b'\\n')[1::4], then resident_batch(list)
  (b) bytes   resident_records(data)
  (c) path    resident_records(path) of the same text in a file that was just written (page cache)
Each is one call that ends with the batch resident and its handle released again; 1 round of warm-up, then the median and
the min-max spread of the host clock over the rounds.  (b) is split, from the engine's own spans of the call
(Engine.records_ms: hipEvents around the copy and the kernels, the host clock around the D2H of ends[]), into the H2D copy,
the sum of the splitting kernels, the D2H of ends[] and the rest (allocations, frees, first[], the tables to numpy).
Before anything is timed the batch of (b) is compared with the batch of (a): the same packed bytes and ends.
Then find_best_matches_batch over the handle of (b), `--patterns` patterns of 32 characters planted `--plants` times each,
max_l_dist = 2: the public call, the fz_batch_assign call inside it, its kernels.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuzzysearch_amd import _native           # noqa: E402
from tests import workloads                   # noqa: E402


def make_fastq(dna):
    """reads x read_len bytes -> the FASTQ text: records of one width, '@r' + 8 digits as header."""
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
    rec[:, at + 3:at + 3 + read_len] = ord('I')
    rec[:, width - 1] = 10
    return rec.tobytes()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--patterns", type=int, default=8)
    ap.add_argument("--plants", type=int, default=64)
    a = ap.parse_args()
    os.environ["FZ_MP_FORCE_PASS"] = "1"                               # (as benchmarks/assign_reads.py: the list rides a pass)
    import fuzzysearch_amd as fa
    flat = workloads.dna(a.reads * a.read_len, 20251019)
    pats = [workloads.dna(32, 9100 + i) for i in range(a.patterns)]
    for i, p in enumerate(pats):                                       # (as benchmarks/assign_reads.py: exact, 1 substitution, 1 deletion, 1 insertion in turn)
        workloads.plant_variants(flat, p, a.plants, 3100 + i)
    dna = flat.reshape(a.reads, a.read_len)
    data = make_fastq(dna)
    eng = _native.default_engine()
    eng.set_timing(True)
    print("ingest: %d reads x %d bytes as FASTQ (%.0f MB of text, %.0f MB of reads); %d rounds after 1 of warm-up (%d for the split route)"
          % (a.reads, a.read_len, len(data) / 1e6, dna.size / 1e6, a.reps, a.base_reps))

    def route_split():
        held = fa.resident_batch(data.split(b'\n')[1::4])
        held.release()

    def route_bytes():
        held = fa.resident_records(data)
        held.release()

    held = fa.resident_records(data)
    listed = fa.resident_batch(data.split(b'\n')[1::4])
    assert len(held) == len(listed) == a.reads
    assert eng.batch_bytes(held.handle) == eng.batch_bytes(listed.handle) == dna.tobytes(), "the two batches differ"
    assert np.array_equal(eng.batch_tables(held.handle)[1], eng.batch_tables(listed.handle)[1])
    assert held[a.reads - 1] == listed[a.reads - 1]
    listed.release()
    held.release()

    route_split()
    s_med, s_lo, s_hi = timed(route_split, a.base_reps)
    print("(a) split + [1::4] + resident_batch(list)  %10.1f ms [%9.1f, %9.1f]" % (s_med, s_lo, s_hi))
    sys.stdout.flush()
    route_bytes()
    walls, spans = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        route_bytes()
        walls.append((time.perf_counter() - t0) * 1e3)
        spans.append(eng.records_ms())
    b_med = float(np.median(walls))
    print("(b) resident_records(bytes)                %10.1f ms [%9.1f, %9.1f]   (a) / (b) = %.1f" % (b_med, min(walls), max(walls), s_med / b_med))
    for key, label in (("h2d", "H2D copy of the text"), ("kernels", "splitting kernels, summed"), ("ends_d2h", "D2H of ends[]"),
                       ("call", "the C-ABI call, whole")):
        v = [s[key] for s in spans]
        print("      %-28s %10.2f ms [%9.2f, %9.2f]" % (label, float(np.median(v)), min(v), max(v)))
    rest = [w - s["h2d"] - s["kernels"] - s["ends_d2h"] for w, s in zip(walls, spans)]
    print("      %-28s %10.2f ms [%9.2f, %9.2f]" % ("host remainder", float(np.median(rest)), min(rest), max(rest)))
    k_med, h_med = float(np.median([s["kernels"] for s in spans])), float(np.median([s["h2d"] for s in spans]))
    print("      kernels / H2D = %.3f (%.0f GB/s of text through the kernels, %.1f GB/s over PCIe)"
          % (k_med / h_med, len(data) / k_med / 1e6, len(data) / h_med / 1e6))
    sys.stdout.flush()

    tmp = tempfile.NamedTemporaryFile(suffix=".fastq", delete=False)
    try:
        tmp.write(data)
        tmp.close()

        def route_path():
            h = fa.resident_records(tmp.name)
            h.release()

        route_path()
        p_med, p_lo, p_hi = timed(route_path, a.reps)
        print("(c) resident_records(path), page cache     %10.1f ms [%9.1f, %9.1f]" % (p_med, p_lo, p_hi))
    finally:
        os.unlink(tmp.name)
    sys.stdout.flush()

    held = fa.resident_records(data)
    ps = [p.tobytes() for p in pats]
    best = fa.find_best_matches_batch(ps, held, max_l_dist=2)
    pub, abi, kern = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fa.find_best_matches_batch(ps, held, max_l_dist=2)
        pub.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.batch_assign(held.handle, _native.MODE_LEV, ps, 2)
        abi.append((time.perf_counter() - t0) * 1e3)
        f, v, _ = eng.kernel_ms()
        kern.append(f + v)
    print("find_best_matches_batch over the handle, %d patterns of 32, max_l_dist=2 (%d reads assigned):" % (len(ps), int((best.pattern >= 0).sum())))
    for label, v in (("public call", pub), ("Engine.batch_assign inside it", abi), ("its kernels (filter + verify)", kern)):
        print("      %-28s %10.2f ms [%9.2f, %9.2f]" % (label, float(np.median(v)), min(v), max(v)))
    held.release()


if __name__ == "__main__":
    main()
