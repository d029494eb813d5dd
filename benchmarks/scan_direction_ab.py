"""Scan direction, A/B inside one process (kernel time repeats to 0.1 % inside a process and moves ~3 % between processes,
profiles/r23_headline_lean.txt §6): blocks of `reps` synchronous calls and `reps` pipelined steps (two searches in flight),
alternating set_scan_direction(1) - always forward - and (0) - every scan starts where the last one ended - on one resident
sequence.  Per block one JSON line: the mean kernel span of the synchronous calls, ms per call, ms per pipelined step.  Then
the medians per mode and the ratio.  Cases: the headline (DNA, m = 20, k = 2), the candidate-free regime (k = 1, a pattern
the text does not hold), configs[2] (ASCII, m = 32, 3 substitutions) and configs[3a] (UTF-8, m = 64, k = 5).
    python benchmarks/scan_direction_ab.py [MiB] [reps] [rounds] [headline]     (headline: that case alone)
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fuzzysearch_amd import _native  # noqa: E402
from tests import workloads  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n = mib << 20
eng = _native.Engine([0])
MODES = ((1, "forward"), (0, "alternating"))


def block(call, begin):
    spans = []
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
        spans.append(eng.kernel_ms()[0])
    sync = (time.perf_counter() - t0) / reps
    begin()
    for _ in range(10):
        begin(); eng.search_end(as_array=True)
    t0 = time.perf_counter()
    for _ in range(reps):
        begin(); eng.search_end(as_array=True)
    pipe = (time.perf_counter() - t0) / reps
    eng.search_end(as_array=True)
    return float(np.mean(spans)), sync * 1e3, pipe * 1e3


def case(name, seq, call, begin):
    h = eng.upload(seq)
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:
        call(h)
    got = {label: [] for _m, label in MODES}
    rows = None
    for rnd in range(rounds):
        for mode, label in MODES:
            eng.set_scan_direction(mode)
            res = block(lambda: call(h), lambda: begin(h))
            got[label].append(res)
            print(json.dumps({"case": name, "MiB": mib, "round": rnd, "mode": label, "kernel_ms": round(res[0], 4),
                              "sync_ms_per_call": round(res[1], 4), "pipelined_ms_per_step": round(res[2], 4)}), flush=True)
            r = call(h)
            assert rows is None or np.array_equal(rows, r), "the rows depend on the direction"
            rows = r
    med = {label: [statistics.median(x[i] for x in v) for i in range(3)] for label, v in got.items()}
    print(json.dumps({"case": name, "MiB": mib, "rows": len(rows), "median": {k: [round(x, 4) for x in v] for k, v in med.items()},
                      "alternating_over_forward": [round(a / f, 4) for a, f in zip(med["alternating"], med["forward"])],
                      "columns": ["kernel_ms", "sync_ms_per_call", "pipelined_ms_per_step"]}), flush=True)
    eng.set_scan_direction(0)
    h.release()


seq, pat = workloads.cfg2(n, mib or 64)[:2]
p = pat.tobytes()
case("headline DNA m=20 k=2", seq, lambda h: eng.lev_ngrams(h, p, 2, as_array=True), lambda h: eng.lev_ngrams_begin(h, p, 2))
if len(sys.argv) > 4 and sys.argv[4] == "headline":
    sys.exit(0)
q = b"NNNNNNNNNNRRRRRRRRRR"                                  # no n-gram of it in the text: the filter alone
case("candidate-free m=20 k=1", seq, lambda h: eng.lev_ngrams(h, q, 1, as_array=True), lambda h: eng.lev_ngrams_begin(h, q, 1))
del seq
seq, pat, _ = workloads.cfg3(n, mib or 64)
p3 = pat.tobytes()
case("configs[2] ASCII m=32 subs<=3", seq, lambda h: eng.subs_ngrams(h, p3, 3, as_array=True), lambda h: eng.subs_ngrams_begin(h, p3, 3))
del seq
seq, pat, _ = workloads.cfg4(n, mib or 64)
p4 = pat.tobytes()
case("configs[3a] UTF-8 m=64 k=5", seq, lambda h: eng.lev_ngrams(h, p4, 5, as_array=True), lambda h: eng.lev_ngrams_begin(h, p4, 5))
