"""Random GPU-vs-oracle cases that also run in a SUBPROCESS (`python -m tests.gpu_cases <what> ...`): several switches
of the library are process-wide statics read from the environment (FZ_FORCE_BIG_VERIFY, FZ_NO_SLOT_AND,
FZ_MAX_BLOCKS, FZ_NO_DIRECT), so a test that wants them set starts a fresh interpreter.  Prints "OK <n cases> <n records>".
The seam sweeps of tests/seam_case.py run through here as well (`seams <route> <CUs>`: the route's small texts, then the
text with several tiles per workgroup; in-process from tests/test_gpu_scan_seams.py for the routes that need no switch), and
those of tests/batch_seam_case.py (`batch-seams <route> <CUs>`) and the shard-cut sweep of tests/shard_cut_case.py
(`shardcut <route>`: the route across a shard cut on a two-device engine and through two handles)."""
import io
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def force_pass():
    """A fixture's body (`force_pass = pytest.fixture(gpu_cases.force_pass)`): -> a function that sets / clears
    FZ_MP_FORCE_PASS and has the library read its switches again; cleared afterwards."""
    from fuzzysearch_amd import _native
    lib = _native.load_library()

    def switch(on):
        if on:
            os.environ["FZ_MP_FORCE_PASS"] = "1"
        else:
            os.environ.pop("FZ_MP_FORCE_PASS", None)
        lib.fz_debug_reload_switches()

    yield switch
    switch(False)


def edited(rnd, p, n_edits, alpha):
    v = bytearray(p)
    for _ in range(n_edits):
        q = rnd.randrange(len(v))
        op = rnd.random()
        if op < 0.4:
            v[q] = rnd.choice(alpha)
        elif op < 0.7 and len(v) > 2:
            del v[q]
        else:
            v.insert(q, rnd.choice(alpha))
    return bytes(v)


def random_cases(rnd, n_cases, ks, max_m, max_n):
    """(pattern, text, k) with planted edited copies at ragged positions (both ends included)."""
    out = []
    while len(out) < n_cases:
        alpha = bytes(rnd.sample(range(1, 256), rnd.choice([2, 3, 4, 4, 20, 200])))
        k = rnd.choice(ks)
        m = rnd.randint(k + 1, max(k + 1, min(max_m, rnd.choice([8, 24, 64, max_m]))))
        n = rnd.randint(0, max_n)
        t = bytearray(rnd.choice(alpha) for _ in range(n))
        p = bytes(rnd.choice(alpha) for _ in range(m))
        for _rep in range(3):
            if n > m + 10 and rnd.random() < 0.8:
                v = edited(rnd, p, rnd.randint(0, k), alpha)
                st = rnd.choice([0, 1, n - len(v) - 1, n - len(v), rnd.randint(0, max(0, n - len(v)))])
                st = max(0, min(st, n - len(v)))
                t[st:st + len(v)] = v
        if len(p) // (k + 1) == 0:
            continue
        out.append((p, bytes(t), k))
    return out


def run_lev_subs(engine, cases):
    import oracle
    n_rec = 0
    for (p, t, k) in cases:
        h = engine.upload(t)
        got = engine.lev_ngrams(h, p, k)
        assert got == oracle.lev_ngrams_raw(p, t, k), ("lev", p, t, k)
        n_rec += len(got)
        got = engine.subs_ngrams(h, p, k)
        assert got == oracle.subs_ngrams_raw(p, t, k), ("subs", p, t, k)
        n_rec += len(got)
        h.release()
    return n_rec


def run_pipelined(engine, cases):
    """Two searches in flight (mixed kinds), and the folded generic search, against the oracle."""
    import oracle
    n_rec = 0
    for (p, t, k) in cases:
        h = engine.upload(t)
        exp_s, exp_l = oracle.subs_ngrams_raw(p, t, k), oracle.lev_ngrams_raw(p, t, k)
        engine.subs_ngrams_begin(h, p, k)
        engine.lev_ngrams_begin(h, p, k)
        assert engine.search_end() == exp_s, ("subs, two in flight", p, t, k)
        assert engine.search_end() == exp_l, ("lev, two in flight", p, t, k)
        engine.lev_ngrams_begin(h, p, k)
        engine.lev_ngrams_begin(h, p, k)
        assert engine.search_end() == exp_l and engine.search_end() == exp_l, ("lev twice", p, t, k)
        n_rec += len(exp_s) + len(exp_l)
        if k and len(t) <= 3000 and len(p) // (k + 1) >= 1:
            try:
                want = oracle.generic_ngrams_raw(p, t, k, k, k, k)
                got = engine.generic_ngrams_consolidated(h, p, k, k, k, k)
            except NotImplementedError:
                pass
            else:
                assert [r[:3] for r in got] == oracle.consolidate(want), ("generic consolidated", p, t, k)
                engine.generic_ngrams_begin(h, p, k, k, k, k, consolidated=True)
                engine.generic_ngrams_begin(h, p, k, k, k, k)
                assert engine.search_end() == got and engine.search_end() == want, ("generic, two in flight", p, t, k)
                n_rec += len(want)
        h.release()
    return n_rec


def run_generic_windows(engine, rnd, n_cases):
    """Generic searches whose n-gram hits share windows (the window table, fz_device.h: FzGenDedup): exact and lightly
    edited copies of patterns with 2 .. 14 blocks (more hits per window than a slot lists members), copies at both ends
    of the text, dense repeats — raw stream, consolidated rows (block included: the smallest), the flag and the two-deep
    pipeline against the oracle."""
    import oracle
    n_rec = cases = 0
    while cases < n_cases:
        alpha = bytes(rnd.sample(range(1, 256), rnd.choice([3, 4, 8, 60])))
        k = rnd.choice([1, 2, 3, 4, 6, 9, 13])
        L = rnd.choice([2, 3, 4, 6])
        m = (k + 1) * L + rnd.randint(0, L - 1)
        p = bytes(rnd.choice(alpha) for _ in range(m))
        n = rnd.randint(m, 4000)
        t = bytearray(rnd.choice(alpha) for _ in range(n))
        for _rep in range(rnd.randint(1, 6)):
            v = edited(rnd, p, rnd.choice([0, 0, 0, 1, 2]), alpha)
            st = max(0, min(rnd.choice([0, n - len(v), rnd.randint(0, max(0, n - len(v)))]), n - len(v)))
            t[st:st + len(v)] = v
        if rnd.random() < 0.15:
            t = bytearray((p * (n // m + 1))[:n])                   # dense repeats: every window shared, long member lists
        t = bytes(t)
        lim = (rnd.randint(0, k), rnd.randint(0, min(k, 3)), rnd.randint(0, min(k, 3)), k)
        try:
            want = oracle.generic_ngrams_raw(p, t, *lim)
        except Exception:
            continue
        if len(want) > 200000:
            continue
        h = engine.upload(t)
        try:
            got = engine.generic_ngrams(h, p, *lim)
        except NotImplementedError:
            h.release()
            continue
        assert got == want, ("generic raw", p, t, lim)
        cons = engine.generic_ngrams_consolidated(h, p, *lim)
        assert [r[:3] for r in cons] == oracle.consolidate(want), ("generic consolidated", p, t, lim)
        from fuzzysearch_amd import _native
        assert cons == [tuple(r) for r in _native.consolidate(got)], ("consolidated rows incl. block", p, t, lim)
        assert engine.generic_ngrams_any(h, p, *lim) == (len(want) > 0)
        engine.generic_ngrams_begin(h, p, *lim)
        engine.generic_ngrams_begin(h, p, *lim, consolidated=True)
        assert engine.search_end() == want and engine.search_end() == cons, ("generic, two in flight", p, t, lim)
        h.release()
        n_rec += len(want)
        cases += 1
    return cases, n_rec


def seam_search(engine, h, kind, p, k):
    """The raw stream of one search of a seam case (tests/seam_case.py), as the oracle states it."""
    if kind == "lev":
        return engine.lev_ngrams(h, p, k)
    if kind == "subs":
        return engine.subs_ngrams(h, p, k)
    if kind == "exact":
        return engine.search_exact(h, p)
    return engine.generic_ngrams(h, p, kind[1], kind[2], kind[3], k)


def check_seam_case(engine, route, case, want, what):
    """Upload, search, the full ordered raw stream against `want`, the form the route is there for; generic searches: the
    consolidated rows and the flag as well."""
    import oracle
    p, k = case.pattern, case.k
    h = engine.upload(case.text)
    try:
        got = seam_search(engine, h, route.kind, p, k)
        form = engine.stats()["verify_form"]
        if got != want:
            bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise AssertionError("%s %s: %d rows against %d expected, first difference at row %d: %r / %r" % (
                route.name, what, len(got), len(want), bad, got[bad:bad + 2], want[bad:bad + 2]))
        assert form == route.form, (route.name, what, "verify_form", form)
        if route.kind[0] == "generic":
            cons = engine.generic_ngrams_consolidated(h, p, route.kind[1], route.kind[2], route.kind[3], k)
            assert [r[:3] for r in cons] == oracle.consolidate(want), (route.name, what, "consolidated")
            assert engine.generic_ngrams_any(h, p, route.kind[1], route.kind[2], route.kind[3], k) == (len(want) > 0)
    finally:
        h.release()
    return len(got)


def run_seam_route(engine, route, n_cus):
    """One route of tests/seam_case.py in the regime of one tile per workgroup: the wave / row / tile sweep on the quiet and
    on the noisy background, the first-tile / start / end sweeps on their small texts (every tail), patterns with NUL bytes
    at either end.  -> (coverage line, searches, rows)."""
    from tests import seam_case as sc
    p = sc.route_pattern(route)
    args = dict(pattern_alphabet=route.alpha, **sc.route_args(route))
    n_search = n_rows = 0
    ntiles = (route.n + sc.TILE - 1) // sc.TILE
    covers = []
    for background in ("quiet", "noisy") if route.noisy else ("quiet",):
        case = sc.build(p, route.k, route.n, n_cus, background, **args)
        want = sc.sparse_expected(route.kind, case) if background == "quiet" else sc.expected(route.kind, case)
        sc.check_exact_copies_found(route.kind, case, want)
        sc.check_coverage(case.coverage, route.m, route.k, route.classes, case.plan, ntiles, edited=route.copies == 2)
        n_rows += check_seam_case(engine, route, case, want, background)
        n_search += 1
        covers.append(case.coverage)
        edge = []
        for case in sc.edge_cases(route, n_cus, background=background):
            want = sc.sparse_expected(route.kind, case) if background == "quiet" else sc.expected(route.kind, case)
            n_rows += check_seam_case(engine, route, case, want, "%s edge n = %d" % (background, len(case.text)))
            n_search += 1
            edge.append(case.coverage)
        sc.check_coverage(sc.merge_coverage(edge), route.m, route.k, ("first", "start", "end"))
        covers += edge
    if route.m <= 64:                                           # the end class once more for every short last tile
        for tail in sc.EDGE_TAILS[1:]:
            edge = []
            for case in sc.edge_cases(route, n_cus, classes=("end",), tail=tail):
                n_rows += check_seam_case(engine, route, case, sc.sparse_expected(route.kind, case), "tail %d" % tail)
                n_search += 1
                edge.append(case.coverage)
            sc.check_coverage(sc.merge_coverage(edge), route.m, route.k, ("end",))
    if route.kind in ("lev", "subs") and route.form != sc.FORM_KERNEL:      # every form that fuses
        for nul in ("head", "tail"):
            p_nul = sc.route_pattern(route, nul)
            for case in sc.edge_cases(route, n_cus, p=p_nul, classes=("start", "end")):
                # (the two NUL bytes change the pattern's alphabet, which a short pattern's form depends on: the form the plan
                #  hook names for this pattern, a fused one)
                form = sc.scan_plan(p_nul, route.k, len(case.text), n_cus)[1] if route.kind == "lev" else route.form
                assert form not in (sc.FORM_NONE, sc.FORM_KERNEL)
                n_rows += check_seam_case(engine, route._replace(form=form), case, sc.sparse_expected(route.kind, case), "NUL %s" % nul)
                n_search += 1
    return sc.coverage_line(route.name, sc.merge_coverage(covers), route.form), n_search, n_rows


def run_seam_route_iterations(engine, route, n_cus, text=None, bg=None):
    """One route in the regime of several tiles per workgroup (64 MiB on 256 CUs: tile iterations 0 .. 2, the next tile's
    rows 0-1 loaded while rows 2-3 are tested; the size comes from the plan hook): the wave / row / tile sweep on the quiet
    background.  `text` / `bg`: the quiet text of an earlier route, its plants restored.  -> (line, rows, text, bg)."""
    from tests import seam_case as sc
    n = sc.size_with_iterations(n_cus, 3, (64 << 20) + 4099)
    case = sc.build(sc.route_pattern(route), route.k, n, n_cus, "quiet", text=text, bg=bg, seed=2, pattern_alphabet=route.alpha,
                    **sc.route_args(route))
    try:
        ntiles = (n + sc.TILE - 1) // sc.TILE
        sc.check_coverage(case.coverage, route.m, route.k, route.classes, case.plan, ntiles, edited=route.copies == 2)
        assert max(o[1] for o in case.coverage["tile"]["tiles"]) >= 2
        want = sc.sparse_expected(route.kind, case)
        sc.check_exact_copies_found(route.kind, case, want)
        rows = check_seam_case(engine, route, case, want, "quiet, %d MiB" % (n >> 20))
    finally:
        case.bg.restore(case.text, case.plants)
    return "%s | grid %d, %d MiB" % (sc.coverage_line(route.name, case.coverage, route.form), case.plan[0], n >> 20), rows, case.text, case.bg


# -- the batch seam sweep (tests/batch_seam_case.py) ---------------------------------------------------------------------------
def batch_rows(engine, h, mode, p, k, reduced):
    """fz_batch_search -> rows (sequence, start, end, dist, block); seq_of is non-decreasing."""
    import numpy as np
    rows, seq_of = engine.batch_search(h, mode, p, k, reduced=reduced)
    assert len(rows) == len(seq_of)
    assert np.all(np.diff(seq_of.astype(np.int64)) >= 0), "seq_of is non-decreasing"
    return [(int(j),) + tuple(int(x) for x in r) for j, r in zip(seq_of.tolist(), rows.tolist())]


def batch_form(route, p, n, n_cus):
    """The verify_form a batch of n packed bytes must report: what the plan hook names for the unsegmented search of the same
    pattern over the same length (tests/test_gpu_batch.py::test_one_pass pins that a batch plans as that search does) - and
    that is the form the route is there for."""
    from tests import seam_case as sc
    form = sc.scan_plan(p, route.k, n, n_cus)[1] if route.kind == "lev" else route.form
    assert form == route.form, (route.name, "the plan names form", form)
    return form


def check_batch_seam_case(engine, route, p, cls, seqs, plants, cache, n_cus):
    """One batch: upload, the raw and the reduced search; the full ordered raw stream with its sequence numbers, the reduced
    rows, stats()["raw_matches"] and ["verify_form"] against the oracle per sequence.  -> rows compared."""
    from tests import batch_seam_case as bc
    mode = bc.MODE[route.kind]
    blob, offs = bc.pack(seqs)
    want_raw, want_red = bc.expected(mode, p, seqs, route.k, cache)
    form = batch_form(route, p, len(blob), n_cus)

    def differ(what, got, want):
        bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        j = (got[bad] if bad < len(got) else want[bad])[0]
        raise AssertionError("%s %s, %s: %d rows against %d expected, first difference at row %d: %r / %r; plants there (class, d): %r" % (
            route.name, cls, what, len(got), len(want), bad, got[bad:bad + 2], want[bad:bad + 2], bc.near(plants, seqs, j)))

    h = engine.upload_batch(blob, offs)
    try:
        got = batch_rows(engine, h, mode, p, route.k, False)
        st = engine.stats()
        if got != want_raw:
            differ("raw", got, want_raw)
        assert st["raw_matches"] == len(want_raw), (route.name, cls, "raw_matches", st["raw_matches"], len(want_raw))
        assert st["verify_form"] == form, (route.name, cls, "verify_form", st["verify_form"], form)
        if route.kind == "lev" and len(p) // (len(p) // (route.k + 1)) > 16:
            assert st["filter_launches"] >= 2, (route.name, cls, "more than 16 blocks: a second launch")
        got = [g[:4] for g in batch_rows(engine, h, mode, p, route.k, True)]
        if got != want_red:
            differ("reduced", got, want_red)
    finally:
        h.release()
    return len(want_raw) + len(want_red)


def check_batch_public(route, p, seqs, plants):
    """find_near_matches_batch over the sequences that hold (a part of) a plant against the loop of find_near_matches."""
    import numpy as np
    import fuzzysearch_amd as fa
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    held = sorted(set(j for pl in plants for j in range(int(np.searchsorted(offs, pl.start, side="right")) - 1,
                                                          int(np.searchsorted(offs, pl.start + len(pl.data) - 1, side="right")))))
    step = max(1, len(held) // 48)
    sub = [seqs[j] for j in held[::step]]
    kw = dict(max_substitutions=route.k, max_insertions=0, max_deletions=0) if route.kind == "subs" else dict(max_l_dist=route.k)
    got = fa.find_near_matches_batch(p, sub, **kw)
    want = [fa.find_near_matches(p, s, **kw) for s in sub]
    assert got == want, (route.name, "find_near_matches_batch")
    assert [[x.matched for x in g] for g in got] == [[x.matched for x in w] for w in want], (route.name, "matched")
    assert sum(len(g) for g in got) > 0
    return len(sub)


def run_batch_seam_route(engine, route, n_cus, public=False, classes=None):
    """Every batch of one route of tests/batch_seam_case.py (of `classes`) -> (line, searches, rows compared)."""
    from tests import batch_seam_case as bc
    from tests import seam_case as sc
    p = sc.route_pattern(route)
    cache = {}
    n_search = n_rows = 0
    parts = []
    for cls, seqs, plants, cover in bc.batches(route, p, classes):
        bc.check_coverage(route, cls, cover, seqs)
        n_rows += check_batch_seam_case(engine, route, p, cls, seqs, plants, cache, n_cus)
        n_search += 2
        parts.append("%s %d seqs %d plants" % (cls, len(seqs), len(plants)))
        if public and cls == "mid":
            parts.append("public %d seqs" % check_batch_public(route, p, seqs, plants))
    return "batch seams %-22s form %s | %s" % (route.name, route.form, "; ".join(parts)), n_search, n_rows


def run_batch_noisy(engine, route, n_cus, tiles=3, side=None):
    """One noisy batch of the route: reads of 30 .. 300 bytes over the pattern's own alphabet (full queues, block-range passes,
    the slow-tile path).  `side`: 'slotted' / 'compact' - the hit list of fz_batch_verify_wf_kernel on that side of
    FZ_WF_COMPACT_MIN, by the oracle's own count of n-gram hits AND by the device's (stats()["ngram_hits"], the length of the
    list the kernel reads; it holds the oracle's hits and those the per-sequence range test then drops).  -> (rows, hits, device hits)."""
    from tests import batch_seam_case as bc
    from tests import seam_case as sc
    p = sc.route_pattern(route)
    seqs, plants = bc.noisy(route, p, tiles)
    hits = bc.ngram_hits(p, seqs, route.k)
    if side == "compact":
        assert hits > bc.WF_COMPACT_MIN, (route.name, "n-gram hits", hits)
    if side == "slotted":
        assert 0 < hits <= bc.WF_COMPACT_MIN, (route.name, "n-gram hits", hits)
    rows = check_batch_seam_case(engine, route, p, "noisy", seqs, plants, {}, n_cus)
    assert rows > 0
    blob, offs = bc.pack(seqs)
    h = engine.upload_batch(blob, offs)
    try:
        engine.batch_search(h, bc.MODE[route.kind], p, route.k)
        on_device = engine.stats()["ngram_hits"]
    finally:
        h.release()
    if side:
        assert on_device >= hits, (route.name, "the device lists fewer n-gram hits than the oracle verifies", on_device, hits)
        assert (on_device > bc.WF_COMPACT_MIN) == (side == "compact"), (route.name, side, on_device)
    return rows, hits, on_device


# -- the multi-pattern seam sweep (tests/mp_seam_case.py) ----------------------------------------------------------------------
def mp_search(engine, h, r, pats):
    """One multi-pattern call of the route's mode over resident `h` -> the raw stream of every pattern of the list."""
    from tests import mp_seam_case as mc
    if r.mode == "lev":
        return engine.lev_ngrams_multi(h, pats, r.k)
    if r.mode == "subs":
        return engine.subs_ngrams_multi(h, pats, r.k)
    return engine.subs_ngrams_multi_classes(h, pats, r.k, mc.tables())


def check_mp_streams(r, pats, got, want, st, what, raw_matches=None):
    """Every pattern's full ordered stream against `want`; the call rode a pass and counted its raw rows (`raw_matches`: how
    many, where `want` is not the raw stream)."""
    from tests import mp_seam_case as mc
    assert len(got) == len(want) == len(pats)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            bad = next((j for j, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            raise AssertionError("%s %s, pattern %d (m = %d): %d rows against %d expected, first difference at row %d: %r / %r" % (
                r.name, what, i, len(pats[i]), len(g), len(w), bad, g[bad:bad + 2], w[bad:bad + 2]))
    assert st["verify_form"] == mc.FORM_KERNEL, (r.name, what, "verify_form", st["verify_form"])
    n_raw = sum(len(w) for w in want) if raw_matches is None else raw_matches
    assert st["raw_matches"] == n_raw, (r.name, what, "raw_matches", st["raw_matches"], n_raw)
    return sum(len(w) for w in want)


def check_mp_case(engine, case, want, what):
    """Upload the case's text, one call for the whole list, check_mp_streams.  -> rows compared."""
    h = engine.upload(case.text)
    try:
        got = mp_search(engine, h, case.route, case.patterns)
        st = engine.stats()
    finally:
        h.release()
    return check_mp_streams(case.route, case.patterns, got, want, st, what)


def run_mp_shard_cut(engine, r, cut, n):
    """The sweep of every carrier across a shard cut at byte `cut` of an n-byte text (seam_case's class `first` with the cut
    for its seam: one text per carrier and phase): the text whole, and as two shards with the halo the mode needs - m + k for
    Levenshtein, m for substitutions and classes.  Per pattern the two shards' rows together, by (block, start), are the
    whole text's rows and the oracle's.  -> (coverage per carrier, texts, rows)."""
    from tests import mp_seam_case as mc
    from tests import seam_case as sc
    pats, carriers = mc.list_of(r)
    halo = max(len(p) for p in pats) + (r.k if r.mode == "lev" else 0)
    covers, texts, rows, straddling = {}, 0, 0, 0
    for i in carriers:
        m = len(pats[i])
        per = []
        for ph in range(sc.phases("first", m, r.k)):
            case = mc.build(r, n, 1, specs=[(i, ("first",), ph, cut)], seed=17 + ph)
            want = mc.expected(case)
            mc.check_exact_copies_found(case, want)
            text = case.text.tobytes()
            whole = engine.upload(text)
            a = engine.upload_shard(text[:cut + halo], 0, 0, cut, n)
            b = engine.upload_shard(text[cut - halo:], cut - halo, cut, n, n)
            try:
                got = mp_search(engine, whole, r, pats)
                check_mp_streams(r, pats, got, want, engine.stats(), "whole, carrier %d phase %d" % (i, ph))
                ra = mp_search(engine, a, r, pats)
                sa = engine.stats()
                rb = mp_search(engine, b, r, pats)
                sb = engine.stats()
            finally:
                for h in (whole, a, b):
                    h.release()
            both = [sorted(x + y, key=lambda row: (row[3], row[0])) for x, y in zip(ra, rb)]
            assert sa["raw_matches"] == sum(len(x) for x in ra) and sb["raw_matches"] == sum(len(x) for x in rb)
            assert sa["verify_form"] == sb["verify_form"] == mc.FORM_KERNEL
            sb["raw_matches"] += sa["raw_matches"]
            rows += check_mp_streams(r, pats, both, want, sb, "two shards, carrier %d phase %d, d = %s" % (
                i, ph, [pl.d for pl in case.plants]))
            straddling += sum(1 for w in want for row in w if row[0] < cut < row[1])
            per.append(case.coverage[i])
            texts += 1
        covers[i] = sc.merge_coverage(per)
        mc.check_edge_coverage(covers[i], m, r.k)
    assert straddling > 0
    return covers, texts, rows


# -- the shard-cut sweep of the single-pattern routes (tests/shard_cut_case.py) -------------------------------------------------
def two_shards(eng2, text, cut, halo):
    """A sharded sequence of a two-device engine: fz_seq_new and one fz_seq_add_shard per device, at halo `halo`."""
    from tests import shard_cut_case as cc
    seq = eng2.new_sequence(len(text))
    try:
        for dev, (buf, off, lo, hi) in enumerate(cc.buffers(text, cut, halo)):
            eng2.add_shard(seq, dev, buf, off, lo, hi)
    except Exception:
        seq.release()
        raise
    return seq


def differ(name, what, got, want):
    if got != want:
        bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s %s: %d rows against %d expected, first difference at row %d: %r / %r" % (
            name, what, len(got), len(want), bad, got[bad:bad + 2], want[bad:bad + 2]))


def shardcut_extras(eng, h, route, p, want, what, two_in_flight):
    """On a handle whose raw stream was `want`: the consolidated rows (Levenshtein, generic), the flag (substitutions,
    generic) and - `two_in_flight` - two searches begun before either is collected."""
    import oracle
    k = route.k
    if route.kind == "lev":
        differ(route.name, what + ", consolidated", [r[:3] for r in eng.lev_ngrams_consolidated(h, p, k)], oracle.consolidate(want))
    elif route.kind == "subs":
        assert eng.subs_ngrams_any(h, p, k) == bool(want), (route.name, what, "subs_ngrams_any")
    elif route.kind != "exact":
        lim = route.kind[1:] + (k,)
        differ(route.name, what + ", consolidated", [r[:3] for r in eng.generic_ngrams_consolidated(h, p, *lim)], oracle.consolidate(want))
        assert eng.generic_ngrams_any(h, p, *lim) == bool(want), (route.name, what, "generic_ngrams_any")
    if two_in_flight and route.kind != "exact":
        for _ in range(2):
            if route.kind == "lev":
                eng.lev_ngrams_begin(h, p, k)
            elif route.kind == "subs":
                eng.subs_ngrams_begin(h, p, k)
            else:
                eng.generic_ngrams_begin(h, p, *(route.kind[1:] + (k,)))
        differ(route.name, what + ", older of two in flight", eng.search_end(), want)
        differ(route.name, what + ", younger of two in flight", eng.search_end(), want)
        return 1
    return 0


def run_shardcut_merged(eng2, route, cases, extras=True):
    """(a) Every case on a two-device engine, the library merging the shards' streams: the ordered raw stream, verify_form and
    raw_matches against the expected stream of the whole text; main-cut extras on the same handle.
    -> (cases run, rows compared, searches with two in flight, expected rows of all cases)."""
    from tests import shard_cut_case as cc
    p = sc_pattern(route)
    halo = cc.halo(route)
    n_rows = n_flight = n_cases = 0
    all_rows = []
    for c in cases:
        want = cc.expected(route, c)
        what = "two devices, cut %d, d = %d %s" % (c.cut, c.d, "exact" if c.exact else "edited")
        h = two_shards(eng2, c.case.text.tobytes(), c.cut, halo)
        try:
            got = seam_search(eng2, h, route.kind, p, route.k)
            st = eng2.stats()
            differ(route.name, what, got, want)
            assert st["verify_form"] == route.form, (route.name, what, "verify_form", st["verify_form"])
            assert st["raw_matches"] == len(want), (route.name, what, "raw_matches", st["raw_matches"], len(want))
            if extras:
                n_flight += shardcut_extras(eng2, h, route, p, want, what, c.exact and c.d == cc.straddling_d(route))
        finally:
            h.release()
        n_rows += len(want)
        n_cases += 1
        all_rows += want
    return n_cases, n_rows, n_flight, all_rows


def run_shardcut_handles(engine, route, cases):
    """(b) Each shard alone, as a handle of its own on a one-device engine (fz_seq_upload_shard): A's rows and B's rows
    together, stably sorted by block (exact search: as they come), are the expected stream; raw_matches of both calls,
    verify_form of a shard that owns a byte; the whole text through fz_seq_upload as the control.  -> (cases, rows)."""
    from tests import shard_cut_case as cc
    p = sc_pattern(route)
    halo = cc.halo(route)
    n_rows = n_cases = 0
    for c in cases:
        want = cc.expected(route, c)
        what = "two handles, cut %d, d = %d %s" % (c.cut, c.d, "exact" if c.exact else "edited")
        text = c.case.text.tobytes()
        (a, a_off, a_lo, a_hi), (b, b_off, b_lo, b_hi) = cc.buffers(text, c.cut, halo)
        hs = [engine.upload_shard(a, a_off, a_lo, a_hi, len(text)), engine.upload_shard(b, b_off, b_lo, b_hi, len(text)), engine.upload(text)]
        try:
            parts = []
            for h, owns in ((hs[0], a_hi > a_lo), (hs[1], b_hi > b_lo)):
                rows = seam_search(engine, h, route.kind, p, route.k)
                st = engine.stats()
                assert st["raw_matches"] == len(rows), (route.name, what, "raw_matches", st["raw_matches"], len(rows))
                if owns:
                    assert st["verify_form"] == route.form, (route.name, what, "verify_form", st["verify_form"])
                parts.append(rows)
            both = parts[0] + parts[1]
            if route.kind != "exact":
                both.sort(key=lambda r: r[3])                   # stable: block major, shard order keeps the index ascending
            differ(route.name, what, both, want)
            differ(route.name, what + ", the whole text", seam_search(engine, hs[2], route.kind, p, route.k), want)
        finally:
            for h in hs:
                h.release()
        n_rows += len(want)
        n_cases += 1
    return n_cases, n_rows


def sc_pattern(route):
    from tests import seam_case as sc
    return sc.route_pattern(route)


def run_shardcut_route(eng2, engine, route):
    """(a) and (b) for one route: the main cut's full sweep and the secondary cuts on the two-device engine, the main cut
    through two handles.  -> the coverage line that was asserted."""
    from tests import shard_cut_case as cc
    main = list(cc.texts(route))
    n_main, rows, n_flight, all_rows = run_shardcut_merged(eng2, route, main)
    cover, nb, across = cc.check_coverage(route, main, all_rows)
    assert n_flight == (0 if route.kind == "exact" else 1)
    n_sec, rows_sec, _f, _r = run_shardcut_merged(eng2, route, list(cc.secondary(route)) + [cc.both_sides(route)], extras=False)
    n_two, rows_two = run_shardcut_handles(engine, route, main)
    assert n_two == n_main and rows_two == rows
    return "%s | secondary cuts: %d texts, %d rows; two handles: %d texts" % (
        cc.coverage_line(route, cover, nb, across, n_main), n_sec, rows_sec, n_two)


def mp_batch_expected(r, pats, seqs, caches):
    """The oracle (lev, subs) or the class model (cls) per (pattern, sequence) -> per pattern (raw rows, reduced rows) as
    (sequence, start, end, dist[, block]).  `caches`: one dict per pattern, by sequence bytes."""
    from fuzzysearch_amd import _native
    from tests import batch_seam_case as bc
    from tests import classes_model
    from tests import seam_case as sc
    out = []
    for p, cache in zip(pats, caches):
        if r.mode != "cls":
            out.append(bc.expected(bc.MODE[r.mode], p, seqs, r.k, cache))
            continue
        raw, red = [], []
        for j, s in enumerate(seqs):
            if len(s) < len(p):
                continue
            hit = cache.get(s)
            if hit is None:
                rows = classes_model.raw_rows(p, s, r.k, sc.iupac_accept())
                hit = cache[s] = (rows, [tuple(x)[:3] for x in _native.group_best(rows)] if rows else [])
            raw += [(j,) + row for row in hit[0]]
            red += [(j,) + row for row in hit[1]]
        out.append((raw, red))
    return out


def run_mp_batch_seams(engine, r):
    """The seam classes of tests/batch_seam_case.py for every carrier of the route's list, each batch searched with the WHOLE
    list through fz_batch_search_multi (classes: fz_batch_search_multi_cls), raw and reduced: every (pattern, sequence) slice
    against the oracle run on that sequence alone, no row outside its sequence.  -> (line, searches, rows compared)."""
    import numpy as np
    from tests import batch_seam_case as bc
    from tests import mp_seam_case as mc
    from tests import seam_case as sc
    pats, carriers = mc.list_of(r)
    caches = [{} for _ in pats]
    rnd = random.Random(23)
    n_search = n_rows = 0
    parts = []
    for i in carriers:
        rr = sc._r("%s-m%d" % (r.name, len(pats[i])), "lev" if r.mode == "lev" else "subs", len(pats[i]), r.k, sc.FORM_KERNEL, alpha=r.alpha)
        assert bc.tier(rr) == 0
        for cls, seqs, plants, cover in bc.batches(rr, pats[i]):
            bc.check_coverage(rr, cls, cover, seqs)
            if r.mode == "cls":                                 # every copy as one of its spellings
                blob = bytearray(b"".join(seqs))
                for pl in plants:
                    blob[pl.start:pl.start + len(pl.data)] = mc.spell(rnd, pl.data)
                ends = np.cumsum([len(s) for s in seqs]).tolist()
                seqs = [bytes(blob[lo:hi]) for lo, hi in zip([0] + ends[:-1], ends)]
            blob, offs = bc.pack(seqs)
            want = mp_batch_expected(r, pats, seqs, caches)
            h = engine.upload_batch(blob, offs)
            try:
                if r.mode == "cls":
                    raw = engine.batch_search_multi_classes(h, pats, r.k, mc.tables(), reduced=False)
                    st_raw = engine.stats()
                    red = engine.batch_search_multi_classes(h, pats, r.k, mc.tables(), reduced=True)
                else:
                    raw = engine.batch_search_multi(h, mc.MODES[r.mode], pats, r.k, reduced=False)
                    st_raw = engine.stats()
                    red = engine.batch_search_multi(h, mc.MODES[r.mode], pats, r.k, reduced=True)
                st_red = engine.stats()
            finally:
                h.release()
            what = "%s carrier %d" % (cls, i)
            got_raw = [batch_flat(*x) for x in raw]
            n_raw = check_mp_streams(r, pats, got_raw, [w[0] for w in want], st_raw, what + ", raw")
            # (the reduced call reduces the same raw rows: its own stats count them, and name the pass)
            got_red = [[g[:4] for g in batch_flat(*x)] for x in red]
            check_mp_streams(r, pats, got_red, [w[1] for w in want], st_red, what + ", reduced", raw_matches=n_raw)
            for g in got_raw:
                assert all(0 <= row[1] <= row[2] <= len(seqs[row[0]]) for row in g), (r.name, what, "a row leaves its sequence")
            assert sum(len(w[0]) for w in want) > 0, (r.name, what)
            n_search += 2
            n_rows += sum(len(w[0]) + len(w[1]) for w in want)
        parts.append("m %d: %s" % (len(pats[i]), ", ".join(bc.classes_of(rr))))
    return "mp batch seams %-12s %d patterns | %s" % (r.name, len(pats), "; ".join(parts)), n_search, n_rows


def batch_flat(rows, seq_of):
    """(rows, seq_of) of one pattern of a batch call -> [(sequence, start, end, dist, block)]; seq_of is non-decreasing."""
    import numpy as np
    assert len(rows) == len(seq_of)
    assert np.all(np.diff(seq_of.astype(np.int64)) >= 0), "seq_of is non-decreasing within a pattern's slice"
    return [(int(j),) + tuple(int(x) for x in row) for j, row in zip(seq_of.tolist(), rows.tolist())]


# -- the file stream (tests/file_seam_case.py) -------------------------------------------------------------------------------
DEFAULT_BATCH = 64 << 20


def file_stream(engine, route, p, S, pre, post, batch_bytes):
    from fuzzysearch_amd import _native
    from tests import file_seam_case as fc
    return _native.FileStream(engine, fc.MODE[route.kind], p, route.limits or (0, 0, 0), route.k, S, pre, post, batch_bytes)


def feed_full(st, data):
    """Every staging buffer filled to its end; a short fill is the last one (fuzzysearch_amd._file_stream._feed_readinto)."""
    pos = 0
    while True:
        view = st.buffer()
        room = len(view)
        if room == 0:
            break
        piece = data[pos:pos + room]
        view[:len(piece)] = piece
        del view
        st.submit(len(piece), len(piece) < room)
        pos += len(piece)
        if len(piece) < room:
            break


def feed_random(st, data, rnd):
    """Submits of 0, 1 .. 64 KiB bytes, then submit(0, last)."""
    pos = 0
    while pos < len(data):
        view = st.buffer()
        take = min(len(view), len(data) - pos, rnd.choice([0, 1, 2, rnd.randint(1, 4096), rnd.randint(1, 65536)]))
        view[:take] = data[pos:pos + take]
        del view
        st.submit(take, False)
        pos += take
    st.submit(0, True)


def stream_rows(engine, case, batch_bytes, feed="full", seed=0, fd=None, threads=1, as_arrays=False):
    """One file stream over the case's file -> (rows (start, end, dist, block) as a list, chunk numbers as a list, form);
    `as_arrays`: as finish() returns them."""
    st = file_stream(engine, case.route, case.pattern, case.S, case.pre, case.post, batch_bytes)
    try:
        if feed == "full":
            feed_full(st, case.data)
        elif feed == "random":
            feed_random(st, case.data, random.Random(seed))
        else:
            assert st.read_fd(fd, 0, threads) == len(case.data)
        raw, seg = st.finish()
        form = engine.stats()["verify_form"]
    finally:
        st.close()
    if as_arrays:
        return raw, seg, form
    return raw.tolist(), seg.tolist(), form


def check_file_stream(engine, case, want, batch_bytes, what, **feed):
    """The stream's rows and chunk numbers against the model's, exactly and in order; the form the route is there for
    (files with at least one whole chunk: the last batch ran a search).  `want`: the model's rows, or (millions of them) an
    int64 array of shape (rows, 5), compared column by column; the rows are listed only when a column differs."""
    import numpy as np
    got, seg, form = stream_rows(engine, case, batch_bytes, as_arrays=isinstance(want, np.ndarray), **feed)
    if isinstance(want, np.ndarray):
        if len(got) == len(want) and all(np.array_equal(got[f], want[:, i]) for i, f in enumerate(("start", "end", "dist", "block"))) \
                and np.array_equal(seg, want[:, 4]):
            assert form == case.route.form, (case.route.name, what, "verify_form", form)
            return len(got)
        got, seg, want = got.tolist(), seg.tolist(), [tuple(r) for r in want.tolist()]
    exp = [r[:4] for r in want]
    exp_seg = [r[4] for r in want]
    if got != exp or seg != exp_seg:
        both = list(zip(zip(got, seg), zip(exp, exp_seg)))
        bad = next((i for i, (a, b) in enumerate(both) if a != b), min(len(got), len(exp)))
        raise AssertionError("%s %s S %d %s batch %d, %d bytes: %d rows against %d expected, first difference at row %d: got %r / %r, "
                             "expected %r / %r" % (case.route.name, what, case.S, "text" if case.text else "binary", batch_bytes,
                                                    len(case.data), len(got), len(exp), bad, got[bad:bad + 3], seg[bad:bad + 3],
                                                    exp[bad:bad + 3], exp_seg[bad:bad + 3]))
    if len(case.data) > case.S + case.pre + case.post:
        assert form == case.route.form, (case.route.name, what, "verify_form", form)
    return len(got)


def eight_chunk_batch(S):
    """A batch size of about eight chunks of stride S whose batch buffers start off the 16 KiB tile grid."""
    return 8 * S + S // 3 + 5


def run_file_route(engine, route, ends=True, public=False):
    """One route of tests/file_seam_case.py: every sweep of fc.sweeps(route) and the file ends, each at the default batch (one
    batch), a batch of about eight chunks, the three-chunk batch the sweep is planted on and the smallest batch; `public`: every
    third sweep through find_near_matches_in_file as well.  -> (coverage lines, streams run, rows compared)."""
    from tests import file_seam_case as fc
    lines, n_streams, n_rows, n_cases, n_public = [], 0, 0, 0, 0
    for (g, text, background) in fc.sweeps(route):
        case = fc.build(route, fc.stride(route, g), text, background)
        want = fc.expected(case)
        fc.check_expectation(case, want, count=False)          # (the counts: tests/test_file_seam_case.py)
        small = set(fc.batch_seams(len(case.data), case.S, case.pre, case.post, fc.small_batch(case.S)))
        assert all(pl.seam in small for pl in case.plants)
        for batch in (DEFAULT_BATCH, eight_chunk_batch(case.S), fc.small_batch(case.S), 1):
            n_rows += check_file_stream(engine, case, want, batch, "%s %s" % (g, background))
            n_streams += 1
        if public and n_cases % 3 == 0:
            n_public += check_public(case)
        n_cases += 1
        if background == "quiet":
            lines.append(fc.coverage_line(route.name, case, route.form) + ", %d rows" % len(want))
    if ends:
        for text in (False, True):
            S = fc.odd_stride(route)
            _S, pre, post, _c = fc.geometry(route, S, text)
            j_end = fc.batches(12 * S, S, pre, post, eight_chunk_batch(S))[0].j1
            covers = {"start": set(), "end": set()}
            for case in fc.end_cases(route, S, text, (3, j_end)):
                want = fc.expected(case)
                for batch in (DEFAULT_BATCH, eight_chunk_batch(case.S), fc.small_batch(case.S), 1):
                    n_rows += check_file_stream(engine, case, want, batch, "file end n = %d" % len(case.data))
                    n_streams += 1
                for side in covers:
                    covers[side] |= case.coverage[side]["exact"] | case.coverage[side]["edited"]
            lines.append("file ends  %-22s %-6s S %5d | chunk %d ends a batch; start items %d, end items %d" % (
                route.name, "text" if text else "binary", S, j_end, len(covers["start"]), len(covers["end"])))
    if public:
        lines.append("%s: %d matches through find_near_matches_in_file (every third sweep)" % (route.name, n_public))
    return lines, n_streams, n_rows


class NamedBytesIO(io.BytesIO):
    mode = 'rb'


def file_route(name):
    from tests import file_seam_case as fc
    return next(r for r in fc.ROUTES if r.name == name)


def plain_case(r, p, data, S, text):
    from tests import file_seam_case as fc
    S, pre, post, chunk_size = fc.geometry(r, S, text)
    return fc.Case(r, p, data, S, pre, post, chunk_size, text, [], {})


def check_public(case):
    """find_near_matches_in_file on the case's file against file_model.file_result: Levenshtein and generic equal or equal
    modulo ties inside an overlap group, substitutions equal modulo ties of equal distance and length, exact equal."""
    import fuzzysearch_amd as fa
    from tests import file_model, golden_io
    from tests import file_seam_case as fc
    r = case.route
    kw = fc.kwargs(r)
    exp, rows = file_model.file_result(case.pattern, case.data, kw, case.chunk_size, case.text)
    if case.text:
        text = case.data.decode('latin-1')
        got = fa.find_near_matches_in_file(case.pattern.decode('latin-1'), io.StringIO(text), _chunk_size=case.chunk_size, **kw)
        assert all(m.matched == text[m.start:m.end] for m in got)
    else:
        got = fa.find_near_matches_in_file(case.pattern, NamedBytesIO(case.data), _chunk_size=case.chunk_size, **kw)
        assert all(bytes(m.matched) == case.data[m.start:m.end] for m in got)
    got = [(m.start, m.end, m.dist) for m in got]
    what = (r.name, case.S, case.text, len(case.data))
    if r.kind in ("lev", "generic"):
        assert got == exp or golden_io.equal_modulo_ties(got, exp, [x[:3] for x in rows]), what
    elif r.kind == "subs":
        assert len(got) == len(exp) and all(g == e or (g[2] == e[2] and g[1] - g[0] == e[1] - e[0]) for g, e in zip(got, exp)), what
    else:
        assert got == exp, what
    return len(got)


# -- re-runs inside a stream -----------------------------------------------------------------------------------------------------
def rerun_many_rows(engine):
    """More than 16 384 records in ONE batch (the search leaves direct mode): files of back-to-back copies, every fifth one
    edited, through the stream (one batch, and batches of about eight chunks) and through the API."""
    from tests import file_seam_case as fc
    n_rows = 0
    # (KiB of file: as small as gives the route its 16 384 rows with a margin - the generic search reports 570 rows per KiB)
    for name, kib in (("seg-band-20-2", 168), ("seg-wf-24-5", 104), ("file-subs-24-3", 152), ("file-generic-20", 40), ("file-exact-8", 216)):
        r = file_route(name)
        p = fc.route_pattern(r)
        rnd = random.Random(9)
        parts = []
        while sum(len(x) for x in parts) < (kib << 10):
            v = p if len(parts) % 5 else fc.edited_copy(rnd, p, r.k, bytes(r.alpha), r.kind == "subs", r.limits)
            parts.append(v + b"0123456"[:len(parts) % 7 + 1])
        for text in (False, True):
            case = plain_case(r, p, b"".join(parts), 7001, text)
            want = fc.expected(case)
            assert len(fc.batches(len(case.data), case.S, case.pre, case.post, DEFAULT_BATCH)) == 1 and len(want) > 16384, len(want)
            for batch in (DEFAULT_BATCH, eight_chunk_batch(case.S)):
                n_rows += check_file_stream(engine, case, want, batch, "many rows")
            if not text:
                check_public(case)
    return n_rows


HIT_LIST_BYTES = (80 << 20) + 4099


def rerun_hit_list(cache):
    """DNA, 80 MiB, m = 20, k = 5 (L = 3, six blocks: about len * 6 / 64 hits) at the default batch: stream_launch sizes the hit
    list max(2^20, len / 64), so the first batch overflows it and runs again.  On an engine of its own: the list only ever
    grows, so on a used engine an earlier search may have left one that is large enough.  `cache`: where the model's rows (and
    the matches expected of the API) are kept between the run in this process and the one under FZ_NO_DIRECT=1."""
    import time
    import numpy as np
    import fuzzysearch_amd as fa
    from fuzzysearch_amd import _native
    from tests import golden_io, workloads
    from tests import file_seam_case as fc
    r = fc.Route("rerun-20-5", "lev", 20, 5, None, fc.DNA, fc.FORM_KERNEL, {}, True, 2)
    t0 = time.time()
    seq = workloads.dna(HIT_LIST_BYTES, 777)
    pattern = workloads.dna(20, 1)
    workloads.plant_variants(seq, pattern, 400, 6)
    keep = fc.keep_of(r)
    case = plain_case(r, pattern.tobytes(), seq.tobytes(), (1 << 20) - keep, False)
    if os.path.exists(cache):
        with np.load(cache) as f:
            want, exp = f["rows"], f["matches"]
    else:
        import oracle
        rows = fc.expected(case)
        want = np.array(rows, dtype=np.int64).reshape(-1, 5)
        exp = np.array(oracle.consolidate([x[:4] for x in rows]), dtype=np.int64).reshape(-1, 3)
        with open(cache, "wb") as f:
            np.savez(f, rows=want, matches=exp)
    bs = fc.batches(len(case.data), case.S, case.pre, case.post, DEFAULT_BATCH)
    first, last = bs[0], bs[-1]
    t1 = time.time()
    eng = _native.Engine([0])
    try:
        n_rows = check_file_stream(eng, case, want, DEFAULT_BATCH, "hit list")
        hits = eng.stats()["ngram_hits"]                      # (of the last batch: every launch starts the counters again)
    finally:
        eng.close()
    # the first batch of this engine met a list of max(2^20, len / 64) entries; the last batch gives the hits per byte
    last_len, first_len = last.data_hi - last.stage_off, first.data_hi - first.stage_off
    room = max(1 << 20, first_len // 64)
    print("hit list: %d rows; last batch %d bytes, %d hits; first batch %d bytes for a list of %d" % (n_rows, last_len, hits, first_len, room))
    assert hits > max(1 << 20, last_len // 64) and first_len > last_len and hits / last_len * first_len > 2 * room, (hits, room)
    t2 = time.time()
    got = fa.find_near_matches_in_file(case.pattern, NamedBytesIO(case.data), max_l_dist=5)
    got = [(m.start, m.end, m.dist) for m in got]
    print("hit list: file and model %.1f s, stream %.1f s, API %.1f s" % (t1 - t0, t2 - t1, time.time() - t2))
    exp = [tuple(x) for x in exp.tolist()]
    assert got == exp or golden_io.equal_modulo_ties(got, exp, [tuple(x) for x in want[:, :3].tolist()])
    assert len(exp) > 300
    return n_rows


def main(argv):
    from fuzzysearch_amd import _native
    what = argv[0]
    if what == "file":
        # one route of tests/file_seam_case.py under the process-wide switch it needs (FZ_FORCE_BIG_VERIFY): argv = route name
        from tests import file_seam_case as fc
        route = next(r for r in fc.ROUTES if r.name == argv[1])
        eng = _native.Engine([0])
        lines, n_streams, n_rows = run_file_route(eng, route)
        eng.close()
        print("\n".join(lines))
        print("OK %d %d" % (n_streams, n_rows))
        return
    if what == "file-reruns":
        # FZ_NO_DIRECT=1: the re-runs inside a stream with records and counters through D2H copies
        eng = _native.default_engine()
        n_rows = rerun_many_rows(eng) + rerun_hit_list(argv[1])
        print("OK 2 %d" % n_rows)
        return
    if what == "seams":
        # one route of tests/seam_case.py under the process-wide switch it needs (FZ_NO_BITS, FZ_WF32, FZ_FORCE_BIG_VERIFY,
        # FZ_NO_SLOT_AND): argv = route name, CU count of the device
        from tests import seam_case as sc
        route = next(r for r in sc.ROUTES if r.name == argv[1])
        eng = _native.Engine([0])
        line, n_search, n_rows = run_seam_route(eng, route, int(argv[2]))
        print(line)
        line, rows, _text, _bg = run_seam_route_iterations(eng, route, int(argv[2]))
        n_search, n_rows = n_search + 1, n_rows + rows
        eng.close()
        print(line)
        print("OK %d %d" % (n_search, n_rows))
        return
    if what == "shardcut":
        # one route of tests/shard_cut_case.py under the process-wide switch it needs: argv = route name
        from tests import shard_cut_case as cc
        route = next(r for r in cc.ROUTES if r.name == argv[1])
        eng2, eng = _native.Engine([0, 0]), _native.Engine([0])
        line = run_shardcut_route(eng2, eng, route)
        eng2.close()
        eng.close()
        print(line)
        print("OK %s" % route.name)
        return
    if what == "batch-seams":
        # one route of tests/batch_seam_case.py under the process-wide switch it needs (FZ_NO_BITS, FZ_NO_WF_FUSE,
        # FZ_FORCE_BIG_VERIFY): argv = route name, CU count of the device[, classes]
        from tests import batch_seam_case as bc
        eng = _native.Engine([0])
        line, n_search, n_rows = run_batch_seam_route(eng, bc.route(argv[1]), int(argv[2]), classes=argv[3].split(",") if len(argv) > 3 else None)
        eng.close()
        print(line)
        print("OK %d %d" % (n_search, n_rows))
        return
    eng = _native.Engine([0])
    rnd = random.Random(int(argv[2]) if len(argv) > 2 else 5)
    n = int(argv[1]) if len(argv) > 1 else 300
    if what == "big":
        # FZ_FORCE_BIG_VERIFY=1: every verification by fz_verify_big_kernel — small budgets (one cell per lane) up to
        # wide ones (CPL 2, 4), short and long pieces, segment ends
        cases = random_cases(rnd, n, [1, 2, 3, 5, 8, 12, 31, 32, 40, 70, 100], 260, 700)
    elif what == "slots":
        # FZ_NO_SLOT_AND=1 (the general slot form of the filter) and FZ_MAX_BLOCKS (several launches per search)
        cases = random_cases(rnd, n, [1, 2, 3, 4, 5, 7], 120, 3000)
        import numpy as np
        from tests import workloads
        seq = workloads.dna(4 << 20, 31)
        pat = workloads.dna(20, 1)
        workloads.plant_variants(seq, pat, 256, 3)
        cases.append((pat.tobytes(), seq.tobytes(), 2))
        seq = workloads.text65(2 << 20, 32)
        pat = workloads.text65(36, 2)
        workloads.plant_edits(seq, pat, 128, 4, workloads.TEXT65, lambda i: i % 4)
        cases.append((pat.tobytes(), seq.tobytes(), 3))
    elif what == "copy":
        # FZ_NO_DIRECT=1: counters and records through D2H copies (the path of searches with more records than the
        # pinned staging buffer holds) — one call at a time and two in flight, where the younger search has to wait
        # for the older one's records to leave the shared device buffer
        cases = random_cases(rnd, n, [1, 2, 3, 4, 5], 60, 3000)
        for sigma, nn, m, k in ((5, 300000, 5, 3), (4, 200000, 8, 1), (3, 100000, 12, 2)):
            alpha = bytes(rnd.sample(range(1, 256), sigma))
            cases.append((bytes(rnd.choices(alpha, k=m)), bytes(rnd.choices(alpha, k=nn)), k))   # up to 2.6e5 records per search
        n_rec = run_pipelined(eng, cases)
    elif what == "taper":
        # the scan grid's regions (FZ_TAPER_STEPS / FZ_TAPER_MIN / FZ_TAPER_WG_PER_CU): a launch big enough to taper its
        # last resident round must return the same streams however the tiles are dealt out
        import hashlib
        from tests import workloads
        seq, pat, _ = workloads.cfg2(n << 20, n)
        p = pat.tobytes()
        h = eng.upload(seq)
        dig = hashlib.sha1()
        n_rec = 0
        lev = eng.lev_ngrams(h, p, 2, as_array=True)
        for rows in (lev, eng.search_exact(h, p, as_array=True),
                     eng.subs_ngrams(h, p, 2, as_array=True), eng.lev_ngrams(h, workloads.dna(36, 9).tobytes(), 5, as_array=True)):
            dig.update(rows.tobytes())
            n_rec += len(rows)
        # ... and the END of the buffer — where the tapered workgroups of the grid's last resident round work — against the
        # ORACLE, so that whichever grid form this process runs (no regions, the default taper, a steep one) is held against
        # the reference's algorithm and not only against another run of this library: the oracle on the last 64 MiB, rows
        # that start at least 64 bytes behind the cut (their windows do not reach across it), shifted, in stream order
        import oracle
        tail = 64 << 20
        off = len(seq) - tail
        want = [(s_ + off, e_ + off, d_, g_) for (s_, e_, d_, g_) in oracle.lev_ngrams_raw(p, seq[off:].tobytes(), 2) if s_ >= 64]
        got = [tuple(int(x) for x in r) for r in lev.tolist() if int(r[0]) >= off + 64]
        assert got == want and len(want) > 30, (len(got), len(want))
        h.release()
        eng.close()
        print("OK %d %d %d" % (n, n_rec, int(dig.hexdigest()[:12], 16)))
        return
    elif what == "wf":
        # Levenshtein budgets 5 .. 15: lane-per-cell verification inside the scan kernel (default; 16 lanes per candidate up
        # to 7, 32 beyond) or in the kernel of its own (FZ_NO_WF_FUSE=1) — ragged ends, patterns up to the argument block, queues that fill up (tiny alphabets)
        cases = random_cases(rnd, n, [5, 6, 7, 8, 10, 12, 15, 20, 31], 300, 6000)   # (16 .. 31: 64 lanes, stand-alone kernel only)
        from tests import workloads
        for sigma, nn, m, k in ((2, 60000, 40, 5), (4, 400000, 30, 5), (3, 150000, 56, 7), (20, 1 << 20, 64, 6),
                                (4, 300000, 50, 8), (3, 100000, 96, 15), (20, 1 << 20, 120, 11), (4, 200000, 130, 24),
                                (2, 400000, 40, 5), (2, 300000, 75, 9), (2, 300000, 140, 19)):   # 2e4 .. 4e4 candidates: the stand-alone kernel appends its records
            alpha = bytes(rnd.sample(range(1, 256), sigma))
            pp = bytes(rnd.choices(alpha, k=m))
            tt = bytearray(rnd.choices(alpha, k=nn))
            for _ in range(40):
                v = edited(rnd, pp, rnd.randint(0, k), alpha)
                st = rnd.randint(0, nn - len(v))
                tt[st:st + len(v)] = v
            cases.append((pp, bytes(tt), k))
        seq = workloads.text65(4 << 20, 41)
        pat = workloads.text65(64, 3)
        workloads.plant_edits(seq, pat, 200, 5, workloads.TEXT65, lambda i: i % 6)
        cases.append((pat.tobytes(), seq.tobytes(), 5))
        n_rec = 0
        import oracle
        for (pp, tt, k) in cases:                               # (Levenshtein only: the substitutions form has no such path)
            h = eng.upload(tt)
            got = eng.lev_ngrams(h, pp, k)
            assert got == oracle.lev_ngrams_raw(pp, tt, k), ("lev", pp, tt[:200], k)
            n_rec += len(got)
            h.release()
        eng.close()
        print("OK %d %d" % (len(cases), n_rec))
        return
    elif what == "windows":
        # the generic search's window table, on (default) and off (FZ_GEN_NO_DEDUP=1: every hit runs the automaton)
        n_cases, n_rec = run_generic_windows(eng, rnd, n)
        eng.close()
        print("OK %d %d" % (n_cases, n_rec))
        return
    else:
        raise SystemExit("unknown case set %r" % what)
    n_rec = n_rec + run_lev_subs(eng, cases) if what == "copy" else run_lev_subs(eng, cases)
    eng.close()
    print("OK %d %d" % (len(cases), n_rec))


if __name__ == "__main__":
    main(sys.argv[1:])
