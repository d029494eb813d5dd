"""-m gpu: the two-deep pipeline of a default engine (no set_streams call) overlaps consecutive fused scans on two streams.
Its ordered raw streams are the synchronous calls', the oracle's and those of the one-stream pipeline (fz_set_streams(1))."""
import random

import numpy as np
import pytest

import oracle
from tests import workloads

pytestmark = pytest.mark.gpu


def _rows(arr):
    return [tuple(int(x) for x in r) for r in arr.tolist()]


def test_default_engine_runs_the_bench_loop_like_the_synchronous_call():
    """bench.py's timed loop (two searches in flight, |p| = 20, k = 2) on 1 GiB of workloads.cfg2, default engine: every
    step returns the synchronous call's stream, and that is the oracle's."""
    from fuzzysearch_amd import _native
    eng = _native.Engine([0])
    try:
        seq, pat, _planted = workloads.cfg2()
        p = pat.tobytes()
        h = eng.upload(seq)
        want = eng.lev_ngrams(h, p, 2, as_array=True)
        steps = 40
        eng.lev_ngrams_begin(h, p, 2)
        for i in range(steps):
            if i + 1 < steps:
                eng.lev_ngrams_begin(h, p, 2)
            got = eng.lev_ngrams_end(as_array=True)
            assert np.array_equal(got, want), i
        # a synchronous call after an odd number of pipelined ones (the younger slot is then the current one) is unchanged
        assert np.array_equal(eng.lev_ngrams(h, p, 2, as_array=True), want)
        h.release()
        assert _rows(want) == oracle.lev_ngrams_raw(p, seq.tobytes(), 2)
    finally:
        eng.close()


def test_mixed_pipeline_equals_the_one_stream_pipeline():
    """Levenshtein / substitutions-only searches in flight two at a time on a default engine, step by step equal to the same
    sequence of calls after fz_set_streams(1) and to the oracle — including a result set too large for the pinned slot (the
    search falls back to the device buffer and one stream) and the overlapped searches after it."""
    from fuzzysearch_amd import _native
    t = workloads.dna(8 << 20, 71).tobytes()
    pats = [(t[5000:5020], 2), (t[70000:70024], 3), (t[123456:123470], 1)]
    for q, (p, k) in enumerate(pats):
        t = t[:300000 * (q + 1)] + p + t[300000 * (q + 1) + len(p):]
    dense_t, dense_p = b"ACGT" * 30000, b"ACGTACGTACGTAC"
    want = {}
    for p, k in pats:
        want[("lev", p, k)] = oracle.lev_ngrams_raw(p, t, k)
        want[("subs", p, k)] = oracle.subs_ngrams_raw(p, t, k)
    want[("dense", dense_p, 2)] = oracle.lev_ngrams_raw(dense_p, dense_t, 2)
    assert len(want[("dense", dense_p, 2)]) > 20000
    rnd = random.Random(9)
    calls = [("lev",) + rnd.choice(pats) if rnd.random() < 0.5 else ("subs",) + rnd.choice(pats) for _ in range(40)]
    calls[17] = ("dense", dense_p, 2)

    def run(streams):
        eng = _native.Engine([0])
        try:
            if streams:
                eng.set_streams(streams)
            h, hd = eng.upload(t), eng.upload(dense_t)
            out, inflight = [], []
            for kind, p, k in calls:
                if kind == "subs":
                    eng.subs_ngrams_begin(h, p, k)
                else:
                    eng.lev_ngrams_begin(hd if kind == "dense" else h, p, k)
                inflight.append((kind, p, k))
                if len(inflight) == 2:
                    out.append((inflight.pop(0), eng.search_end()))
            while inflight:
                out.append((inflight.pop(0), eng.search_end()))
            return out
        finally:
            eng.close()

    default, one = run(None), run(1)
    assert len(default) == len(one) == len(calls)
    for i, ((c, got), (c1, got1)) in enumerate(zip(default, one)):
        assert c == c1 == calls[i]
        assert got == got1 == want[c], (i, c[0])
