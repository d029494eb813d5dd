"""-m gpu: the RAW stream of a file search - what fz_stream_finish returns: every row (start, end, dist, block) and the chunk
number of every row - against the model of the reference's chunk loop (tests/file_model.py over the oracle, raw=True),
exactly and in order.  No tie-aware comparison on this level: ties only arise in consolidation, which is not involved.

The stream is driven directly (_native.FileStream: buffer / submit / read_fd / finish) so that the batch size is the test's:
the default (one batch), about eight chunks, three chunks (the planted chunk seams are its batch seams) and the smallest (two).  Inputs:
tests/file_seam_case.py - a copy of the pattern at every offset across both seams of a chunk boundary, the file ends around
the existence rule of the last chunk - for every kernel a file search can take; then what the host state machine adds: feeds
of any granularity, reuse of the previous stream's buffers, re-runs inside a stream (more records than direct mode holds,
more hits than the hit list), several default batches.  A third of the cases also go through find_near_matches_in_file under
the rules of tests/test_gpu_file_api.py.  Each case prints the coverage it asserted (pytest -s / -rP)."""
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import fuzzysearch_amd as fa
from tests import file_model, golden_io, gpu_cases, workloads
from tests import file_seam_case as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- every route x geometry x batch size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [r for r in fc.ROUTES if not r.env], ids=lambda r: r.name)
def test_chunk_and_batch_seams(engine, r):
    t0 = time.time()
    lines, n_streams, n_rows = gpu_cases.run_file_route(engine, r, public=True)
    print("\n".join(lines))
    print("%s: %d streams, %d rows compared, %.1f s" % (r.name, n_streams, n_rows, time.time() - t0))
    assert n_streams >= 12 and n_rows > 0


@pytest.mark.parametrize("r", [r for r in fc.ROUTES if r.env], ids=lambda r: r.name)
def test_chunk_and_batch_seams_under_a_switch(r):
    """FZ_FORCE_BIG_VERIFY=1 is read once per process: a fresh interpreter (tests/gpu_cases.py: file)."""
    e = dict(os.environ)
    e.update(r.env)
    res = subprocess.run([sys.executable, "-m", "tests.gpu_cases", "file", r.name], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    out = res.stdout.decode()
    assert res.returncode == 0 and "OK " in out, out[-3000:]
    print(out.strip())


# -- the host state machine ----------------------------------------------------------------------------------------------------
FEED_ROUTES = ("seg-band-20-2", "seg-dense-20-4", "seg-wf-54-8", "file-subs-24-3", "file-subs-dense-12-3", "file-exact-8",
               "file-exact-1", "file-generic-20")


def test_feed_invariance(engine, tmp_path):
    """The same file in full buffers, in seeded random submits of 0 .. 64 KiB with a final submit(0, last), and through read_fd
    from a real file with 1 and 4 threads, at every batch size: one stream, the model's - wherever the batches end."""
    fn = tmp_path / "feed.bin"
    n_streams = 0
    for name in FEED_ROUTES:
        r = gpu_cases.file_route(name)
        for (g, text, background) in (("odd", False, "noisy" if r.noisy else "quiet"), ("smallest", True, "quiet"), ("4096", False, "quiet")):
            case = fc.build(r, fc.stride(r, g), text, background, seed=3)
            want = fc.expected(case)
            fn.write_bytes(case.data)
            fd = os.open(str(fn), os.O_RDONLY)
            try:
                for batch in (gpu_cases.DEFAULT_BATCH, gpu_cases.eight_chunk_batch(case.S), fc.small_batch(case.S), 1):
                    what = "%s feed" % g
                    gpu_cases.check_file_stream(engine, case, want, batch, what + " full")
                    for seed in (1, 2):
                        gpu_cases.check_file_stream(engine, case, want, batch, what + " random %d" % seed, feed="random", seed=seed)
                    for threads in (1, 4):
                        gpu_cases.check_file_stream(engine, case, want, batch, what + " read_fd %d" % threads, feed="fd", fd=fd, threads=threads)
                    n_streams += 5
            finally:
                os.close(fd)
    print("feed invariance: %d routes, %d streams" % (len(FEED_ROUTES), n_streams))


def test_buffer_reuse():
    """One engine: a stream with a large staging capacity, then a smaller capacity and a shorter file in the buffers the first
    left behind (stale bytes of the longer file behind the shorter one's end, the allocation larger than the capacity),
    then a larger one again (the buffers have to grow) - each equal to its model, for a segmented and an unsegmented mode."""
    from fuzzysearch_amd import _native
    eng = _native.Engine([0])
    try:
        for name in ("seg-band-20-2", "file-subs-24-3", "file-generic-20", "file-exact-8"):
            r = gpu_cases.file_route(name)
            p = fc.route_pattern(r)
            S = fc.odd_stride(r)
            rnd = random.Random(5)
            alpha = np.frombuffer(bytes(r.alpha), dtype=np.uint8)

            def dense(n, seed):
                """noisy background, a copy (every third one edited) every 64 bytes: stale bytes would be rows"""
                data = alpha[np.random.default_rng(seed).integers(0, len(alpha), n, dtype=np.uint8)].copy()
                for i, at in enumerate(range(7, n - 2 * r.m, 64)):
                    v = p if i % 3 else fc.edited_copy(rnd, p, r.k, bytes(r.alpha), r.kind == "subs", r.limits)
                    data[at:at + len(v)] = np.frombuffer(v, dtype=np.uint8)
                return data.tobytes()
            for text in (False, True):
                for (n, batch) in (((3 << 19) + 11, 2 << 20), (20 * S + 5, 1), (9 * S + S // 2, 3 * S), ((5 << 19) + 3, 3 << 20), (S + 1, 1)):
                    case = gpu_cases.plain_case(r, p, dense(n, n), S, text)
                    rows = gpu_cases.check_file_stream(eng, case, fc.expected(case), batch, "reuse n = %d" % n)
                    assert rows > 0
    finally:
        eng.close()


# -- re-runs inside a stream -----------------------------------------------------------------------------------------------------
def test_reruns_inside_a_stream(engine, tmp_path):
    cache = str(tmp_path / "hit_list_rows.npz")
    t0 = time.time()
    n = gpu_cases.rerun_many_rows(engine)
    t1 = time.time()
    n += gpu_cases.rerun_hit_list(cache)
    print("re-runs: %d rows compared; many rows %.1f s, hit list %.1f s" % (n, t1 - t0, time.time() - t1))
    # the same two where records and counters come back through D2H copies (process-wide switch: a fresh interpreter)
    e = dict(os.environ)
    e["FZ_NO_DIRECT"] = "1"
    res = subprocess.run([sys.executable, "-m", "tests.gpu_cases", "file-reruns", cache], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    out = res.stdout.decode()
    assert res.returncode == 0 and "OK " in out, out[-3000:]
    print(out.strip())


# -- several default batches for what never had them ---------------------------------------------------------------------------
MANY_BATCHES = (("file-generic-20", True), ("seg-dense-20-4", False), ("seg-wf-54-8", True), ("file-subs-dense-20-4", False))
MANY_BYTES = (140 << 20) + 12345


def test_default_chunks_many_batches(engine, tmp_path):
    """140 MiB of DNA with the default 1 MiB chunks at the default batch: three batches, double-buffered staging.  A copy
    across a seam of the batch boundaries, of their neighbours and of some chunk boundaries, variants all over; generic, Levenshtein k = 4 and (54, 8),
    substitutions (dense form); two of them with the text geometry; from a real file through the reader pool."""
    fn = tmp_path / "big.bin"
    seq = workloads.dna(MANY_BYTES, 4242)
    C = 1 << 20
    cases = []
    for q, (name, text) in enumerate(MANY_BATCHES):
        r = gpu_cases.file_route(name)
        pattern = np.frombuffer(fc.route_pattern(r), dtype=np.uint8)
        m = r.m
        workloads.plant_variants(seq, pattern, 200, 5 + q)
        S, pre, post, chunk_size = fc.geometry(r, C if text else C - fc.keep_of(r), text)
        assert chunk_size == C
        seams = fc.batch_seams(MANY_BYTES, S, pre, post, gpu_cases.DEFAULT_BATCH)
        assert len(seams) == 2, seams
        deltas = (-m - r.k - 1, -m, -m // 2, -1, 0, 1, r.k + 1)
        # (the text geometries share their seams: each takes one batch boundary; every route its own chunk boundaries)
        mine = [seams[q // 2]] if text else seams
        js = sorted(set(mine + [j + 1 for j in mine] + [j - 1 for j in mine] + list(range(20 * q + 1, 20 * q + 8)) + [136 + q]))
        for i, j in enumerate(js):                                 # one copy per boundary: side and offset step with it
            B = fc.seam_bytes(j, S, pre, post)[(i + (j in mine)) % 2]
            at = B + deltas[i % len(deltas)]
            seq[at:at + m] = pattern
        cases.append((r, text, S))
    data = seq.tobytes()
    fn.write_bytes(data)
    fd = os.open(str(fn), os.O_RDONLY)
    try:
        for i, (r, text, S) in enumerate(cases):
            case = gpu_cases.plain_case(r, fc.route_pattern(r), data, S, text)
            want = fc.expected(case)
            assert len(want) > 200
            rows = gpu_cases.check_file_stream(engine, case, want, gpu_cases.DEFAULT_BATCH, "many batches", feed="fd", fd=fd, threads=8)
            n_api = 0
            if not text:
                with open(fn, 'rb') as f:
                    got = fa.find_near_matches_in_file(case.pattern, f, **fc.kwargs(r))
                got = [(x.start, x.end, x.dist) for x in got]
                exp, raw = file_model.file_result(case.pattern, data, fc.kwargs(r), C, False)
                if r.kind == "lev":
                    assert got == exp or golden_io.equal_modulo_ties(got, exp, [x[:3] for x in raw]), r.name
                else:
                    assert len(got) == len(exp) and all(g == e or (g[2] == e[2] and g[1] - g[0] == e[1] - e[0]) for g, e in zip(got, exp)), r.name
                n_api = len(got)
            print("many batches: %s %s, %d rows, %d matches through the API" % (r.name, "text" if text else "binary", rows, n_api))
    finally:
        os.close(fd)
