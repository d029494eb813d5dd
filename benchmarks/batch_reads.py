"""One adapter against millions of short reads: fz_batch_search / find_near_matches_batch.

    python benchmarks/batch_reads.py [reads = 4000000] [read length = 150] [repeats = 30]

Workload: `reads` reads of `read length` bytes of workloads.dna (4 M x 150 = 600 MB), an adapter of 33 characters planted
with at most 2 edits in 1 % of the reads, max_l_dist = 2.
 (a) the batch search at the C-ABI (raw and reduced rows) on reads held by fz_batch_upload, against the yardstick measured in
     the same run, alternating: the unsegmented fz_lev_ngrams of the same adapter over the same packed bytes as ONE
     sequence.  Host clock around synchronous calls (each ends in the completion of its kernels), median / min / max of
     `repeats` calls after 5 of warm-up, plus the filter kernels' own hipEvent span (fz_stats).
 (b) find_near_matches_batch end to end (packing, upload, search, Match objects), on a list of bytes and on a
     resident_batch handle, against the Python loop over the first 20 000 reads scaled by reads / 20 000 (the loop's cost
     is per read: one upload, one launch, one C-ABI round trip each).
Prints one JSON line.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import workloads

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
read_len = int(sys.argv[2]) if len(sys.argv) > 2 else 150
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 30
loop_reads = min(20_000, n_reads)
K = 2

data = workloads.dna(n_reads * read_len, 20251017)
adapter = workloads.dna(33, 3)
rng = np.random.default_rng(11)
planted = np.sort(rng.choice(n_reads, size=max(1, n_reads // 100), replace=False))
for j in planted.tolist():
    v = bytearray(adapter.tobytes())
    for _ in range(int(rng.integers(0, K + 1))):
        q = int(rng.integers(1, len(v) - 1))
        op = int(rng.integers(0, 3))
        if op == 0:
            v[q] = int(workloads.DNA[int(rng.integers(0, 4))])
        elif op == 1:
            del v[q]
        else:
            v.insert(q, int(workloads.DNA[int(rng.integers(0, 4))]))
    at = j * read_len + int(rng.integers(0, read_len - len(v) + 1))
    data[at:at + len(v)] = np.frombuffer(bytes(v), dtype=np.uint8)
blob = data.tobytes()
p = adapter.tobytes()
offs = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)

eng = _native.default_engine()
hb = eng.upload_batch(blob, offs)
hs = eng.upload(blob)


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


calls = {
    "yardstick_lev_ngrams": lambda: eng.lev_ngrams(hs, p, K, as_array=True),
    "batch_raw": lambda: eng.batch_search(hb, _native.MODE_LEV, p, K, reduced=False),
    "batch_reduced": lambda: eng.batch_search(hb, _native.MODE_LEV, p, K, reduced=True),
}
wall = {k: [] for k in calls}
kern = {k: [] for k in calls}
rows = {}
for it in range(5 + repeats):                       # alternating: the three share whatever else the machine is doing
    for name, fn in calls.items():
        ms, r = timed(fn)
        st = eng.stats()
        if it >= 5:
            wall[name].append(ms)
            kern[name].append(st["filter_ms"])
        rows[name] = len(r[0]) if isinstance(r, tuple) else len(r)
        form = st["verify_form"]
        launches = st["filter_launches"]
out = {"case": "%d reads x %d bytes of DNA, adapter of 33, max_l_dist=2, 1 %% planted" % (n_reads, read_len),
       "packed_MB": round(len(blob) / 1e6, 1), "repeats": repeats, "verify_form": form, "filter_launches": launches, "rows": rows,
       "c_abi_wall": {k: spread(v) for k, v in wall.items()}, "c_abi_filter_kernel": {k: spread(v) for k, v in kern.items()}}
y = statistics.median(wall["yardstick_lev_ngrams"])
out["batch_raw_over_yardstick"] = round(statistics.median(wall["batch_raw"]) / y, 3)
out["batch_reduced_over_yardstick"] = round(statistics.median(wall["batch_reduced"]) / y, 3)
out["kernel_batch_over_yardstick"] = round(statistics.median(kern["batch_raw"]) / statistics.median(kern["yardstick_lev_ngrams"]), 3)
out["yardstick_GBps"] = round(len(blob) / (y * 1e-3) / 1e9, 1)
out["batch_raw_GBps"] = round(len(blob) / (statistics.median(wall["batch_raw"]) * 1e-3) / 1e9, 1)
hb.release()
hs.release()

# (b) the public call, end to end
view = memoryview(blob)
reads = [bytes(view[i * read_len:(i + 1) * read_len]) for i in range(n_reads)]
api = []
for _ in range(3):
    ms, res = timed(lambda: fa.find_near_matches_batch(p, reads, max_l_dist=K))
    api.append(ms)
out["find_near_matches_batch_ms"] = spread(api)
out["reads_with_matches"] = sum(1 for r in res if r)
held = fa.resident_batch(reads)
api_held = []
for _ in range(3):
    ms, res2 = timed(lambda: fa.find_near_matches_batch(p, held, max_l_dist=K))
    api_held.append(ms)
assert res2 == res
held.release()
out["find_near_matches_batch_resident_ms"] = spread(api_held)
with fa.residency_cache().bypass():
    ms, loop = timed(lambda: [fa.find_near_matches(p, s, max_l_dist=K) for s in reads[:loop_reads]])
assert loop == res[:loop_reads]
out["loop_first_reads"] = {"reads": loop_reads, "ms": round(ms, 1), "scaled_to_all_reads_ms": round(ms * n_reads / loop_reads, 1),
                           "scaling": "x %g (cost per read)" % (n_reads / loop_reads)}
out["loop_over_batch"] = round(ms * n_reads / loop_reads / statistics.median(api), 1)
print(json.dumps(out))
