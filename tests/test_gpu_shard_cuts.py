"""-m gpu: every single-pattern route and form of tests/seam_case.py, and the linear-programming routes, across a SHARD CUT
(tests/shard_cut_case.py; the construction is checked on the CPU by tests/test_shard_cut_case.py).  A hit at global index
idx belongs to the one shard with own_lo <= idx < own_hi: fz_hit_in_range / fz_hit_in_range_s, the tiling of fz_lp_kernel
from own_lo, lo / hi of fz_hamming_kernel, check_halo, the host's merge of the shards' streams and the consolidation of a
group across the cut - a copy of the pattern at cut + d for every d in [-(m + k) - 1, k + 1] (long patterns: every block's
index at cut - 1 and at cut, the named offsets), exact and edited, the cut off the 16-byte grid, both shards at the MINIMAL
halo (m + k; m for substitutions, exact search and subs_lp):

  a  a two-device engine on one GPU (fz_seq_new / fz_seq_add_shard): the library's merged stream, ordered, verify_form,
     raw_matches; the consolidated rows, the flag, two searches in flight; cuts at the tile seam, cuts where a buffer
     clamps at an end of the text, the cuts 0 and n
  b  each shard as a handle of its own (fz_seq_upload_shard): both streams together, sorted stably by block
  c  the automatic split of fz_seq_upload on a two-device engine (the wide halo)
  d  the routes a process-wide switch selects: a and b in a fresh interpreter (python -m tests.gpu_cases shardcut NAME)
  e  lev_lp / subs_lp / generic_lp with the cut at EVERY position of a text of 3 x 256 + 77 bytes
  f  the halo rule: one byte short on either side raises, the exact halo does not, the engine still answers afterwards

Each test prints the coverage it asserted (pytest -s / -rP)."""
import os
import subprocess
import sys
import time

import pytest

from fuzzysearch_amd import _native
from tests import gpu_cases
from tests import seam_case as sc
from tests import shard_cut_case as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = dict(ids=lambda r: r.name)
IN_PROCESS = [r for r in cc.ROUTES if not r.env]
SWITCHED = [r for r in cc.ROUTES if r.env]


@pytest.fixture(scope="module")
def eng2():
    """Two device states on one GPU: one shard per device, the host merges."""
    e = _native.Engine([0, 0])
    yield e
    e.close()


@pytest.mark.parametrize("r", IN_PROCESS, **BY_NAME)
def test_two_device_engine_merges(eng2, r):
    """a: the main cut's full sweep, then the secondary cuts and the text with a copy well inside either shard."""
    t0 = time.perf_counter()
    main = list(cc.texts(r))
    n_main, rows, n_flight, all_rows = gpu_cases.run_shardcut_merged(eng2, r, main)
    cover, nb, across = cc.check_coverage(r, main, all_rows)
    assert n_flight == (0 if r.kind == "exact" else 1)
    n_sec, rows_sec, _f, _r = gpu_cases.run_shardcut_merged(eng2, r, list(cc.secondary(r)) + [cc.both_sides(r)], extras=False)
    assert n_sec >= 3 * len(cc.named_offsets(r.m, r.k)) + len(set(cc.end_cuts(r))) + 2 * 2 + 1
    print("%s | %d rows; secondary cuts: %d texts, %d rows; %.2f s" % (
        cc.coverage_line(r, cover, nb, across, n_main), rows, n_sec, rows_sec, time.perf_counter() - t0))


@pytest.mark.parametrize("r", IN_PROCESS, **BY_NAME)
def test_each_shard_alone(engine, r):
    """b: two handles on the shared engine, the main cut's full sweep."""
    t0 = time.perf_counter()
    main = list(cc.texts(r))
    n_two, rows = gpu_cases.run_shardcut_handles(engine, r, main)
    cover, nb, across = cc.check_coverage(r, main, [row for c in main for row in cc.expected(r, c)])
    print("%s | two handles, %d rows, %.2f s" % (cc.coverage_line(r, cover, nb, across, n_two), rows, time.perf_counter() - t0))


@pytest.mark.parametrize("r", IN_PROCESS, **BY_NAME)
def test_automatic_split(eng2, r):
    """c: fz_seq_upload on the two-device engine cuts an even text in its middle: the named offsets there, and a copy well
    inside either half."""
    p = sc.route_pattern(r)
    n_texts = rows = 0
    for c in cc.split_texts(r):
        assert len(c.case.text) % 2 == 0 and c.cut == len(c.case.text) // 2
        want = cc.expected(r, c)
        h = eng2.upload(c.case.text)
        try:
            got = gpu_cases.seam_search(eng2, h, r.kind, p, r.k)
            st = eng2.stats()
        finally:
            h.release()
        gpu_cases.differ(r.name, "automatic split, d = %d" % c.d, got, want)
        assert st["verify_form"] == r.form and st["raw_matches"] == len(want) and st["n_devices"] == 2
        n_texts += 1
        rows += len(want)
    assert n_texts == len(cc.named_offsets(r.m, r.k)) + 1 and rows > 0
    print("shard cut %-22s form %s | automatic split at byte %d: %d texts, %d rows" % (r.name, r.form, (cc.N + 1) // 2, n_texts, rows))


@pytest.mark.parametrize("r", SWITCHED, **BY_NAME)
def test_routes_under_a_switch(r):
    """d: a and b in a fresh interpreter with the route's switch set."""
    e = dict(os.environ)
    e.update(r.env)
    res = subprocess.run([sys.executable, "-m", "tests.gpu_cases", "shardcut", r.name], cwd=ROOT, env=e,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = res.stdout.decode()
    assert res.returncode == 0 and "OK " in out, out[-3000:]
    print(out.strip())


def _lp_search(eng, h, r, p):
    if r.kind == "lev_lp":
        return eng.lev_lp(h, p, r.k)
    if r.kind == "subs_lp":
        return eng.subs_lp(h, p, r.k)
    return eng.generic_lp(h, p, *r.limits)


@pytest.mark.parametrize("r", cc.LP_ROUTES, **BY_NAME)
def test_lp_routes_at_every_cut(eng2, engine, r):
    """e: the ordered list of the two-device engine at every cut 0 .. n; every 16th cut through two handles as well."""
    t0 = time.perf_counter()
    c = cc.lp_case(r)
    across = cc.check_lp_case(c)
    halo = cc.lp_halo(r)
    n_two = 0
    for cut in cc.lp_cuts():
        h = gpu_cases.two_shards(eng2, c.text, cut, halo)
        try:
            gpu_cases.differ(r.name, "two devices, cut %d" % cut, _lp_search(eng2, h, r, c.pattern), c.want)
            assert eng2.stats()["raw_matches"] == len(c.want), (r.name, cut, "raw_matches")
            if r.kind == "subs_lp":
                assert eng2.subs_lp_any(h, c.pattern, r.k) == bool(c.want), (r.name, cut, "subs_lp_any")
        finally:
            h.release()
        if cut % 16 == 0:
            parts = []
            for (buf, off, lo, hi) in cc.buffers(c.text, cut, halo):
                hs = engine.upload_shard(buf, off, lo, hi, len(c.text))
                try:
                    parts += _lp_search(engine, hs, r, c.pattern)
                finally:
                    hs.release()
            gpu_cases.differ(r.name, "two handles, cut %d" % cut, sorted(parts), sorted(c.want))
            n_two += 1
    print("lp shard cut %-20s | %d cuts (%d with a row across them), %d through two handles, %d rows each, %.2f s" % (
        r.name, cc.LP_N + 1, across, n_two, len(c.want), time.perf_counter() - t0))


def _halo_kinds():
    band, subs, exact, gen = (next(r for r in cc.ROUTES if r.name == name) for name in ("band-L6-k2", "subs-L6-k3", "exact-8", "generic-20"))
    lp = {r.kind: r for r in cc.LP_ROUTES}
    return [("lev_ngrams", band), ("subs_ngrams", subs), ("search_exact", exact), ("generic_ngrams", gen),
            ("lev_lp", lp["lev_lp"]), ("subs_lp", lp["subs_lp"]), ("generic_lp", lp["generic_lp"])]


@pytest.mark.parametrize("kind,r", _halo_kinds(), ids=[kind for kind, _r in _halo_kinds()])
def test_halo_rule(eng2, kind, r):
    """f: with the halo one byte short on B's left, and separately on A's right, the call raises and says so; with the exact
    halo it succeeds; after each raise a plain search on the same engine answers correctly."""
    if kind.endswith("_lp"):
        c = cc.lp_case(r)
        p, text, want, halo, cut = c.pattern, c.text, c.want, cc.lp_halo(r), cc.LP_STARTS + 77
        search = lambda h: _lp_search(eng2, h, r, p)
    else:
        p = sc.route_pattern(r)
        c = next(iter(cc.texts(r, offs=[cc.straddling_d(r)])))
        text, want, halo, cut = c.case.text.tobytes(), cc.expected(r, c), cc.halo(r), c.cut
        search = lambda h: gpu_cases.seam_search(eng2, h, r.kind, p, r.k)
    n = len(text)
    assert halo == len(p) + (0 if kind in ("subs_ngrams", "search_exact", "subs_lp") else r.k) and want

    def plain():
        h = eng2.upload(text)
        try:
            gpu_cases.differ(kind, "the whole text after a refused search", search(h), want)
        finally:
            h.release()

    (a, a_off, a_lo, a_hi), (b, b_off, b_lo, b_hi) = cc.buffers(text, cut, halo)
    for what, bufs in (("B's left", ((a, a_off, a_lo, a_hi), (b[1:], b_off + 1, b_lo, b_hi))),
                       ("A's right", ((a[:-1], a_off, a_lo, a_hi), (b, b_off, b_lo, b_hi)))):
        h = eng2.new_sequence(n)
        try:
            for dev, (buf, off, lo, hi) in enumerate(bufs):
                eng2.add_shard(h, dev, buf, off, lo, hi)
            with pytest.raises(_native.HipEngineError, match="halo too small"):
                search(h)
        finally:
            h.release()
        plain()
    h = gpu_cases.two_shards(eng2, text, cut, halo)
    try:
        gpu_cases.differ(kind, "the exact halo", search(h), want)
    finally:
        h.release()
    print("halo rule %-14s | m %d, k %d: %d bytes accepted, %d refused on either side; %d rows" % (kind, len(p), r.k, halo, halo - 1, len(want)))
