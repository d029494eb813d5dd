"""The gathers of the ingest and of derive_batch under one kernel trace (profiles/r18_derive.txt, second part).

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python benchmarks/derive_trace.py            # the workload
    python benchmarks/derive_trace.py --summarize <dir>                                                   # the table

(benchmarks/derive_trace.sh runs both.)  The workload: 4 x resident_records of the ingest benchmark's FASTQ (4 M reads of 150
bytes), then Engine.derive_batch over its handle, 3 calls per form: identity plain / REV / XLAT / REV + XLAT, then a trim (ends
only).  The table: every fz_rec_* and fz_derive_* kernel with its durations in microseconds in dispatch order — of
fz_rec_gather_kernel the first 4 run inside resident_records (source: the FASTQ text), the next 3 are the plain identity
derive (source: the packed bytes), the last 3 the trim.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def workload(reads=4_000_000, read_len=150):
    import numpy as np
    import fuzzysearch_amd as fa
    from fuzzysearch_amd import _native
    from tests import workloads
    from ingest_reads import make_fastq
    data = make_fastq(workloads.dna(reads * read_len, 20251019).reshape(reads, read_len))
    eng = _native.default_engine()
    for _ in range(3):
        fa.resident_records(data).release()
    held = fa.resident_records(data)
    ends = np.random.RandomState(18).randint(read_len * 2 // 3, read_len + 1, size=reads).astype(np.uint64)
    for kw in (dict(), dict(reverse=True), dict(translate=fa.DNA_COMPLEMENT), dict(reverse=True, translate=fa.DNA_COMPLEMENT), dict(ends=ends)):
        for _ in range(3):
            eng.derive_batch(held.handle, **kw).release()
    held.release()


def summarize(directory):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    by = {}
    for _t, name, us in rows:
        by.setdefault(name.split("(")[0], []).append(us)
    for name, v in by.items():
        if "fz_rec_gather" in name or "fz_derive" in name:
            print("%-50s calls %3d  us in dispatch order: %s" % (name, len(v), " ".join("%.1f" % x for x in v)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        workload()
