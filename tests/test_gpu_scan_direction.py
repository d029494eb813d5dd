"""-m gpu: a scan that walks the sequence backwards (FZ_FLAG_REVERSE: every step of a workgroup's walk reads the mirror
tile) returns the rows of the forward one.  Ordered raw streams against the oracle under set_scan_direction(1) (always
forward), (2) (always reversed) and (0) (alternating: searched twice, so that both directions run), for every verification
form, on the smallest buffers at which the walk can go wrong - one, two and three tiles, whole and one byte either side, with
copies at index 0, ending at the last byte and across every tile seam - on the shortest text whose plan gives a workgroup
three tile iterations (queue codes of iterations >= 1 decoded through the mirrored walk), and on the smallest text whose
plan has regions.  The pipeline: six searches, two in flight, on one and on two streams - the directions alternate launch
by launch; a result set beyond the pinned slot found by a reversed scan - the re-run goes forward.  Batches, has_near_match
and file streams always go forward."""
import random

import numpy as np
import pytest

import oracle
from fuzzysearch_amd import _native
from tests import gpu_cases
from tests import seam_case as sc
from tests.test_gpu_scan_seams import device_cus

pytestmark = pytest.mark.gpu

T = sc.TILE


def _dna(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def _forms():
    rnd = random.Random(20)
    lean = _dna(rnd, 20)
    rep = _dna(rnd, 6)
    return [
        # name, kind, pattern, k, verify_form (None: not asserted), alphabet of the background
        ("lean-band", "lev", lean, 2, sc.FORM_BAND),
        ("repeated-ngram", "lev", rep + rep + _dna(rnd, 8), 2, sc.FORM_BAND),          # two blocks hash alike: the full instance
        ("bits-k3", "lev", _dna(rnd, 24), 3, sc.FORM_BITS32),
        ("cells-m150-k6", "lev", _dna(rnd, 150), 6, sc.FORM_CELLS),
        ("subs", "subs", _dna(rnd, 13), 2, sc.FORM_BAND),
        ("exact", "exact", _dna(rnd, 20), 0, None),
        ("generic", ("generic", 2, 1, 1), _dna(rnd, 20), 2, None),
        ("blocks20", "lev", _dna(rnd, 60), 19, None),                                   # 20 blocks: two launches, opposite directions
    ]


FORMS = _forms()
SMALL = [tiles * T + d for tiles in (1, 2) for d in (-1, 0, 1)] + [3 * T - 1, 3 * T, 2 * T + 777]     # 1, 2 and 3 tiles


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine([0])
    yield e
    e.close()


def _planted(rnd, p, n):
    """Random DNA with the pattern at index 0, ending at the last byte, and across every tile seam."""
    t = bytearray(_dna(rnd, n))
    m = len(p)
    if n >= m:
        t[:m] = p
        t[n - m:] = p
        for S in range(T, n, T):
            at = S - m // 2
            if at > m and at + m < n - m:
                t[at:at + m] = p
    return bytes(t)


def _in_every_direction(eng, h, kind, p, k, want, what, form=None):
    """Forward, reversed, and alternating twice: every stream is `want`; the reversed launches are all of 'always reversed'
    and every other one of the alternating calls.  -> scan launches of one search."""
    start = eng.scan_direction(h)[1]
    for mode in (1, 2, 0, 0):
        eng.set_scan_direction(mode)
        got = gpu_cases.seam_search(eng, h, kind, p, k)
        if got != want:
            bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise AssertionError("%s, direction mode %d: %d rows against %d expected, first difference at row %d: %r / %r" % (
                what, mode, len(got), len(want), bad, got[bad:bad + 2], want[bad:bad + 2]))
        if form is not None:
            assert eng.stats()["verify_form"] == form, (what, mode)
    eng.set_scan_direction(0)
    launches = eng.stats()["filter_launches"]
    if kind in ("lev", "subs"):                                 # (stats() counts the scan launches of these kinds only)
        assert launches >= 1 and eng.scan_direction(h)[1] - start == 2 * launches, (what, launches, eng.scan_direction(h)[1] - start)
    else:
        assert eng.scan_direction(h)[1] - start >= 2, what
    return launches


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_small_buffers_in_every_direction(eng, form):
    name, kind, p, k, vform = form
    rnd = random.Random(len(p) * 31 + k)
    for n in SMALL:
        text = _planted(rnd, p, n)
        want = sc.oracle_fn(kind, p, k)(text)
        assert len(want) >= 1, (name, n)
        h = eng.upload(np.frombuffer(text, dtype=np.uint8))
        try:
            launches = _in_every_direction(eng, h, kind, p, k, want, "%s n = %d" % (name, n), vform)
        finally:
            h.release()
        assert kind not in ("lev", "subs") or launches >= (2 if name == "blocks20" else 1), (name, n, launches)


def test_a_run_of_one_character_is_enumerated_in_reverse(eng):
    """A text of one character against a pattern of that character: every tile overflows the empty queue and is enumerated
    (the `slow` path), here through the mirrored walk."""
    p, k = b"A" * 12, 1
    for n in (T + 1, 3 * T - 1):
        text = b"A" * n
        want = oracle.lev_ngrams_raw(p, text, k)
        assert len(want) > n
        h = eng.upload(np.frombuffer(text, dtype=np.uint8))
        try:
            _in_every_direction(eng, h, "lev", p, k, want, "run of one character, n = %d" % n)
        finally:
            h.release()


ITER_ROUTES = ("band-L6-k2", "bits32-20-4", "cells16-150-5", "subs-L6-k3", "exact-20", "generic-20", "blocks20-60-19")


def _route(name):
    return next(r for r in sc.ROUTES if r.name == name)


@pytest.fixture(scope="module")
def iter_text():
    """The shortest text (from 16 MiB up, steps of 1.5) whose plan gives some workgroup three tiles; quiet, re-planted."""
    n = sc.size_with_iterations(device_cus(), 3, (16 << 20) + 4099)
    return {"n": n, "text": None, "bg": None}


@pytest.mark.parametrize("name", ITER_ROUTES)
def test_tile_iterations_through_the_mirrored_walk(eng, iter_text, name):
    r = _route(name)
    n = iter_text["n"]
    case = sc.build(sc.route_pattern(r), r.k, n, device_cus(), "quiet", text=iter_text["text"], bg=iter_text["bg"], seed=5,
                    pattern_alphabet=r.alpha, **dict(sc.route_args(r), classes=("tile", "start", "end"), copies=1))
    iter_text["text"], iter_text["bg"] = case.text, case.bg
    try:
        its = set(o[1] for o in case.coverage["tile"]["tiles"])
        assert {0, 1} <= its and any(o[3] and o[1] >= 2 for o in case.coverage["tile"]["tiles"]), sorted(its)
        want = sc.sparse_expected(r.kind, case)
        sc.check_exact_copies_found(r.kind, case, want)
        h = eng.upload(case.text)
        try:
            _in_every_direction(eng, h, r.kind, case.pattern, r.k, want, "%s, %d MiB" % (name, n >> 20), r.form)
        finally:
            h.release()
    finally:
        case.bg.restore(case.text, case.plants)


def test_the_smallest_text_with_regions(eng):
    """The synchronous plan's regions (the overlapped plan has none at any size: asserted).  Tile sweep and both seams of the
    first and last tile of every region."""
    cus = device_cus()
    ntiles = next(t for t in range(cus, 1 << 18, max(1, cus // 4)) if sc.scan_plan(b"ACGTACGT", 1, t * T + 777, cus)[3])
    n = ntiles * T + 777
    assert not sc.scan_plan(b"ACGTACGT", 1, n, cus, 1)[3] and not sc.scan_plan(b"ACGTACGT", 1, 4 * n, cus, 1)[3]
    text = bg = None
    for name in ("band-L6-k2", "bits32-20-4", "exact-20"):
        r = _route(name)
        case = sc.build(sc.route_pattern(r), r.k, n, cus, "quiet", text=text, bg=bg, seed=7, pattern_alphabet=r.alpha,
                        **dict(sc.route_args(r), classes=("region", "tile"), copies=1))
        text, bg = case.text, case.bg
        assert case.plan[3] and case.coverage["region"]["seams"]
        want = sc.sparse_expected(r.kind, case)
        h = eng.upload(case.text)
        try:
            _in_every_direction(eng, h, r.kind, case.pattern, r.k, want, "%s, regions, %d MiB" % (name, n >> 20), r.form)
        finally:
            h.release()
            case.bg.restore(case.text, case.plants)


def test_pipeline_alternates_launch_by_launch(eng, iter_text):
    """Six searches, two in flight, on two streams and on one: before every launch the debug call names its direction, the
    launch takes it and flips the sequence's bit; every stream is the synchronous one."""
    r = _route("band-L6-k2")
    case = sc.build(sc.route_pattern(r), r.k, iter_text["n"], device_cus(), "quiet", text=iter_text["text"], bg=iter_text["bg"],
                    seed=9, pattern_alphabet=r.alpha, **dict(sc.route_args(r), classes=("tile", "start", "end"), copies=1))
    try:
        want = sc.sparse_expected(r.kind, case)
        h = eng.upload(case.text)
        try:
            eng.set_scan_direction(0)
            assert eng.lev_ngrams(h, case.pattern, r.k) == want
            for streams in (2, 1):
                eng.set_streams(streams)
                seen = []
                pending = 0
                for i in range(6):
                    nxt, count = eng.scan_direction(h)
                    eng.lev_ngrams_begin(h, case.pattern, r.k)
                    after, count_after = eng.scan_direction(h)
                    assert after == (not nxt) and count_after - count == int(nxt), (streams, i)
                    seen.append(nxt)
                    pending += 1
                    if pending == 2:
                        assert eng.search_end() == want, (streams, i)
                        pending -= 1
                assert eng.search_end() == want
                assert seen == [seen[0], not seen[0]] * 3
            eng.set_streams(2)
        finally:
            h.release()
    finally:
        eng.set_streams(2)
        case.bg.restore(case.text, case.plants)


def test_overflow_found_in_reverse_is_rerun_forward(eng):
    """More rows than the pinned result slot holds (16 384 records), found by a reversed scan: the search is run again in
    copy mode, forward - one reversed launch in all - and the rows are the oracle's."""
    rnd = random.Random(4)
    p = _dna(rnd, 20)
    n = 24000 * 64 + 333
    text = bytearray(rnd.choice(b"0123456789") for _ in range(n))
    for at in range(0, n - 64, 64):
        text[at + 7:at + 27] = p
    text = bytes(text)
    want = oracle.lev_ngrams_raw(p, text, 2)
    assert len(want) > 3 * 16384
    # the pipeline first, on an engine whose buffers have not grown: two searches in flight, both launched reversed, both
    # beyond the slot - the fallback synchronises the streams and re-runs each in copy mode, forward
    fresh = _native.Engine([0])
    try:
        hf = fresh.upload(np.frombuffer(text, dtype=np.uint8))
        fresh.set_scan_direction(2)
        fresh.lev_ngrams_begin(hf, p, 2)
        fresh.lev_ngrams_begin(hf, p, 2)
        assert fresh.search_end() == want, "older of two in flight"
        assert fresh.search_end() == want, "younger of two in flight"
        assert fresh.scan_direction(hf)[1] == 2, fresh.scan_direction(hf)      # one reversed launch per search: its first
        hf.release()
    finally:
        fresh.close()
    h = eng.upload(np.frombuffer(text, dtype=np.uint8))
    try:
        eng.set_scan_direction(2)
        before = eng.scan_direction(h)[1]
        got = eng.lev_ngrams(h, p, 2)
        assert eng.scan_direction(h)[1] - before == 1
        assert got == want
        assert eng.lev_ngrams(h, p, 2) == want                   # (the buffers have grown: one launch, reversed)
        assert eng.scan_direction(h)[1] - before == 2
    finally:
        eng.set_scan_direction(0)
        h.release()


def test_batches_has_near_match_and_file_streams_go_forward(engine, tmp_path):
    """Under 'always reversed' none of them launches a reversed scan, and their answers are what they were."""
    import fuzzysearch_amd as fa
    rnd = random.Random(6)
    p = _dna(rnd, 20)
    reads = [_dna(rnd, rnd.randint(30, 400)) for _ in range(300)]
    for i in range(0, 300, 7):
        reads[i] = reads[i][:5] + p + reads[i][5:]
    blob = b"".join(reads)
    offs = np.cumsum([0] + [len(x) for x in reads]).astype(np.uint64)
    text = _planted(rnd, p, 5 * T + 99)
    path = tmp_path / "text.bin"                                # a regular binary file: the streaming pipeline (fz_stream)
    path.write_bytes(text)

    def in_file(**limits):
        with open(path, "rb") as f:
            return fa.find_near_matches_in_file(p, f, **limits)
    subs = dict(max_substitutions=2, max_insertions=0, max_deletions=0)
    engine.set_scan_direction(1)
    try:
        b = engine.upload_batch(np.frombuffer(blob, dtype=np.uint8), offs)
        h = engine.upload(np.frombuffer(text, dtype=np.uint8))
        fwd_batch = engine.batch_search(b, _native.MODE_LEV, p, 2)
        fwd_file = in_file(max_l_dist=2)
        fwd_subs = in_file(**subs)                                # (unsegmented chunks)
        assert fwd_subs == fa.find_near_matches(p, text, **subs)
        assert len(fwd_batch[0]) >= 40 and len(fwd_file) >= 5 and len(fwd_subs) >= 5
        engine.set_scan_direction(2)
        before = engine.scan_direction(h)[1]
        rev_batch = engine.batch_search(b, _native.MODE_LEV, p, 2)
        assert np.array_equal(rev_batch[0], fwd_batch[0]) and np.array_equal(rev_batch[1], fwd_batch[1])
        assert engine.scan_direction(h)[1] == before, "a batch search launched a reversed scan"
        assert engine.subs_ngrams_any(h, p, 2) and not engine.subs_ngrams_any(h, b"TTTTTTGGGGGGCCCCCCAA", 1)
        assert engine.scan_direction(h)[1] == before, "has_near_match launched a reversed scan"
        assert in_file(max_l_dist=2) == fwd_file and in_file(**subs) == fwd_subs
        assert engine.scan_direction(h)[1] == before, "a file stream launched a reversed scan"
        assert engine.lev_ngrams(h, p, 2) == oracle.lev_ngrams_raw(p, text, 2)
        assert engine.scan_direction(h)[1] == before + 1         # (the hook does count: a whole scan of the sequence)
        b.release()
        h.release()
    finally:
        engine.set_scan_direction(0)


def test_rounds_plan_two_in_flight_in_both_directions(monkeypatch):
    """FZ_SCAN_ROUNDS=1 (the first and last resident round of a scan behind another one in address order): 1 GiB, quiet, the
    tile sweep under that plan's regions; six searches, two in flight, alternating directions: every stream is the expected one."""
    L = _native.load_library()
    monkeypatch.setenv("FZ_SCAN_ROUNDS", "1")
    L.fz_debug_reload_switches()
    e = _native.Engine([0])
    try:
        r = _route("band-L6-k2")
        n = (1 << 30) + 777
        over = sc.scan_plan(sc.route_pattern(r), r.k, n, device_cus(), 1)
        case = sc.build(sc.route_pattern(r), r.k, n, device_cus(), "quiet", seed=13, pattern_alphabet=r.alpha, plan=over,
                        **dict(sc.route_args(r), classes=("region", "tile"), copies=1))
        assert over[2] and (len(over[3]) == 3 or device_cus() * 14 > over[0])
        want = sc.sparse_expected(r.kind, case)
        h = e.upload(case.text)
        assert e.lev_ngrams(h, case.pattern, r.k) == want
        seen = []
        e.lev_ngrams_begin(h, case.pattern, r.k)
        for _ in range(6):
            seen.append(e.scan_direction(h)[0])
            e.lev_ngrams_begin(h, case.pattern, r.k)
            assert e.search_end() == want
        assert e.search_end() == want and set(seen) == {True, False}
        h.release()
    finally:
        e.close()
        monkeypatch.delenv("FZ_SCAN_ROUNDS")
        L.fz_debug_reload_switches()
