"""The batch seam sweep's construction (tests/batch_seam_case.py), on the CPU: for every route, every class holds every offset
it is meant to, and the inputs DISCRIMINATE - a kernel that ignores the seams between the sequences, or one of the two
clamps, would return another stream than the oracle per sequence (where no input can discriminate - a one-byte pattern, exact
search and the clamp at sa, the flush copies of the edge batches - the models must EQUAL the oracle instead); every exact copy flush against a seam is expected at
distance 0 in its sequence.  These are conditions on the inputs: tests/test_gpu_batch_seams.py runs the same batches on the
device."""
import pytest

from tests import batch_seam_case as bc


@pytest.mark.parametrize("r", bc.ROUTES, ids=lambda r: r.name)
def test_coverage_and_discrimination(r):
    p = bc.sc.route_pattern(r)
    mode = bc.MODE[r.kind]
    cache = {}
    seen = set()
    for cls, seqs, plants, cover in bc.batches(r, p):
        bc.check_coverage(r, cls, cover, seqs)
        seen.add(cls.split("-")[0])
        raw, red = bc.expected(mode, p, seqs, r.k, cache)
        assert raw and red, (r.name, cls, "an empty expected stream")
        assert all(0 <= row[1] <= row[2] <= len(seqs[row[0]]) for row in raw), "rows lie inside their sequences"
        assert not bc.flush_missing(mode, p, seqs, plants, raw), (r.name, cls, bc.flush_missing(mode, p, seqs, plants, raw)[:5])
        side_cache = {}
        blind = bc.seam_blind(mode, p, seqs, r.k, plants, side_cache)
        no_se = bc.clamped_one_side(mode, p, seqs, r.k, "sa", side_cache)
        no_sa = bc.clamped_one_side(mode, p, seqs, r.k, "se", side_cache)
        if r.m == 1:
            # a copy of one byte cannot be cut by a seam: no input discriminates, and the three models say so themselves
            assert blind == raw and no_se == raw and no_sa == raw, (r.name, cls)
            continue
        if cls.startswith("edge"):
            # no copy crosses a seam there (flush copies only): the exact rows of the models are the expected ones
            exact_rows = [row for row in raw if row[3] == 0]
            assert exact_rows and all(row in blind and row in no_se and row in no_sa for row in exact_rows), (r.name, cls)
            continue
        assert blind != raw, (r.name, cls, "a seam-blind kernel passes")
        assert no_se != raw, (r.name, cls, "a kernel without the clamp at se passes")
        if mode == bc.EXACT:
            # exact search has no window to the left of its hit, nothing reaches below sa: the model without that clamp IS the
            # oracle per sequence, on any input
            assert no_sa == raw, (r.name, cls)
        else:
            assert no_sa != raw, (r.name, cls, "a kernel without the clamp at sa passes")
    assert seen == set(bc.classes_of(r))


@pytest.mark.parametrize("name, tiles, side", bc.NOISY_ROUTES)
def test_noisy_batches(name, tiles, side):
    """The noisy batches: a non-empty expected stream, and the oracle's own count of n-gram hits on the side of
    FZ_WF_COMPACT_MIN the batch is there for."""
    r = bc.route(name)
    p = bc.sc.route_pattern(r)
    seqs, plants = bc.noisy(r, p, tiles)
    assert 2 <= sum(len(s) for s in seqs) // bc.TILE <= 4 and all(30 <= len(s) <= 300 for s in seqs[:-1]) and plants
    raw, red = bc.expected(bc.MODE[r.kind], p, seqs, r.k, {})
    assert raw and red
    hits = bc.ngram_hits(p, seqs, r.k)
    if side == "slotted":
        assert 0 < hits <= bc.WF_COMPACT_MIN, hits
    if side == "compact":
        assert hits > bc.WF_COMPACT_MIN, hits


def test_the_models_agree_where_no_copy_meets_a_seam():
    """The three models of a wrong kernel are the oracle per sequence on a batch whose copies lie inside their sequences."""
    r = bc.route("band-L6-k2")
    p = bc.sc.route_pattern(r)
    quiet = bc.sc.quiet_alphabet(p)
    pad = bytes(quiet[i % len(quiet)] for i in range(60))
    seqs = [pad + p + pad, pad, b"", pad + p[:5] + p[6:] + pad]
    plants = [bc.Plant(60, p, "none", 0, 0, True), bc.Plant(len(seqs[0]) + 120, p[:5] + p[6:], "none", 0, 0, False)]
    cache = {}
    raw, _red = bc.expected(bc.LEV, p, seqs, r.k, cache)
    assert raw and {row[0] for row in raw} == {0, 3}
    assert bc.seam_blind(bc.LEV, p, seqs, r.k, plants, cache) == raw
    assert bc.clamped_one_side(bc.LEV, p, seqs, r.k, "sa", cache) == raw
    assert bc.clamped_one_side(bc.LEV, p, seqs, r.k, "se", cache) == raw


def test_routes_follow_the_scan_sweep():
    names = [r.name for r in bc.ROUTES]
    assert len(names) == len(set(names))
    for m in (1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 300, 1030):
        assert "exact-%d" % m in names
    shared = [r for r in bc.sc.ROUTES if r in bc.ROUTES]
    assert len(shared) >= 30
    assert {bc.tier(r) for r in bc.ROUTES} == {0, 1, 2}
    assert [r.name for r in bc.ROUTES if bc.tier(r) == 2] == ["big16-257-256", "big32-513-512"]    # k >= 256 only
    assert all(bc.route(name) for name, _tiles, _side in bc.NOISY_ROUTES)
