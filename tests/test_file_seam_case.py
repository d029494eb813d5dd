"""CPU: the construction of the file stream's seam sweep (tests/file_seam_case.py) - the coverage conditions for every route
and geometry, that the expectation is not vacuous and is the FILE's semantics (not the in-memory one), the batching rule of
fz_stream_submit restated, and the raw form of the file model (tests/file_model.py, raw=True) against its default form on the
golden records."""
import os
import random

import pytest

from tests import file_model
from tests import file_seam_case as fc

HERE = os.path.dirname(os.path.abspath(__file__))


def test_raw_form_reduces_to_the_default_form():
    """raw=True keeps the unreduced n-gram stream of every chunk of a substitutions-only search; the per-chunk reduction
    (what _file_stream._post_process applies after finish()) gives the default form, which is pinned to the reference.
    Every other kind: the two forms are the same rows."""
    n = {"lev": 0, "subs": 0, "exact": 0, "generic": 0}
    reduced = 0
    for rec in file_model.load():
        kind, rows = file_model.file_raw(rec["p"], rec["data"], rec["kwargs"], rec["chunk"], rec["text"])
        kind2, raw = file_model.file_raw(rec["p"], rec["data"], rec["kwargs"], rec["chunk"], rec["text"], raw=True)
        assert kind == kind2
        if kind == "subs":
            k = file_model.route(rec["kwargs"])[1]
            if k and len(rec["p"]) // (k + 1) >= 3:
                by_chunk = {}
                for r in raw:
                    by_chunk.setdefault(r[4], []).append(r)
                assert sorted(by_chunk) == list(by_chunk), "chunks out of order"
                again = []
                for j, part in by_chunk.items():
                    keep = len(rec["p"]) - 1
                    a = file_model.chunk_bounds(len(rec["data"]), rec["chunk"], keep, rec["text"])[j][0]
                    local = file_model.reduce_subs([(s - a, e - a, d, g) for (s, e, d, g, _j) in part], rec["text"])
                    again += [(s + a, e + a, d, g, j) for (s, e, d, g) in local]
                assert again == rows, (rec["kwargs"], rec["chunk"], rec["text"])
                reduced += len(raw) != len(rows)
            else:
                assert raw == rows
        else:
            assert raw == rows
        n[kind] += 1
    assert all(v >= 80 for v in n.values()) and reduced > 20, (n, reduced)


def test_routes_take_the_strategy_class_they_name():
    for r in fc.ROUTES:
        kind, k, limits, extra = file_model.route(fc.kwargs(r))
        assert kind == r.kind and k == r.k
        if r.kind != "exact":
            assert r.m // (r.k + 1) >= 3                       # the n-gram route, which is what the stream runs
        S = fc.smallest_stride(r)
        keep = fc.keep_of(r)
        assert r.m + 2 * r.k + 2 <= S and keep <= S // 2       # fz_stream_open's conditions
        assert r.m + 2 * r.k + 2 > S - 1 or keep > (S - 1) // 2 or 2 * keep + 2 > S - 1
    assert fc.keep_of(next(r for r in fc.ROUTES if r.name == "file-exact-1")) == 0
    assert set(r.name for r in fc.ROUTES if r.name not in fc.HEAVY) | set(fc.HEAVY) == set(r.name for r in fc.ROUTES)


def test_batching_rule_deals_every_chunk_to_one_batch():
    """Properties every batching must have, for the restatement of fz_stream_submit's rule (the device tests compare whole
    streams and do not depend on it; it backs the claim that the planted chunk seams are batch seams)."""
    # every chunk in exactly one batch, in order; a batch's buffer holds all its chunks need; no batch beyond the capacity
    rnd = random.Random(4)
    for _ in range(3000):
        keep = rnd.randint(0, 60)
        S = rnd.randint(2 * keep + 2, 400)
        text = rnd.random() < 0.5
        pre, post = (keep, 0) if text else (0, keep)
        n = rnd.choice([0, 1, post, post + 1, S, rnd.randint(0, 40 * S)])
        B = rnd.choice([1, S, fc.small_batch(S), 3 * S + 5, 8 * S + S // 3 + 5, 1 << 20])
        bs = fc.batches(n, S, pre, post, B)
        bounds = file_model.chunk_bounds(n, S if text else S + keep, keep, text)
        assert [b.j0 for b in bs] == [0] + [b.j1 for b in bs[:-1]] if bs else not bounds
        assert (bs[-1].j1 if bs else 0) == len(bounds)
        for b in bs:
            assert b.data_hi - b.stage_off <= fc.capacity(S, pre, post, B)
            assert b.stage_off <= bounds[b.j0][0] and bounds[b.j1 - 1][1] <= b.data_hi
        if B == fc.small_batch(S) and len(bs) > 2:
            assert all(b.j1 - b.j0 == 3 for b in bs[:-1])
        if B == 1 and len(bs) > 2:
            assert all(b.j1 - b.j0 <= 2 for b in bs[:-1]) and bs[-1].j1 - bs[-1].j0 <= 3     # (the end of the file: what is there)


@pytest.mark.parametrize("r", fc.ROUTES, ids=lambda r: r.name)
def test_coverage_of_every_route_and_geometry(r):
    """fc.check_coverage for every sweep: every d exact and edited on a chunk seam and on both sides, on batch seams of the
    three-chunk batch; all 16 lane residues at the odd strides; per geometry a seam within `keep` of a wave, a row and a tile
    seam unless the geometry has none (the strides on the grid always have).  (No model run.)"""
    near = {"wave": 0, "row": 0, "tile": 0}
    n = 0
    for g in fc.GEOMETRIES:
        if not fc.admissible(r, g):
            continue
        for text in (False, True):
            if r.name in fc.HEAVY and (g, text) not in fc.HEAVY[r.name]:
                continue
            case = fc.build(r, fc.stride(r, g), text)
            got = fc.check_coverage(case)
            for key in near:
                near[key] += got[key]
            if g in ("odd", "16383", "16385"):
                assert got["residues"] == 16
            if g in ("1024", "4096", "16384"):
                assert not case.coverage["unattainable"] and min(got[key] for key in near) > 0
            bounds = file_model.chunk_bounds(len(case.data), case.chunk_size, fc.keep_of(r), text)
            assert len(bounds) >= 2 * len(case.plants) >= 2 * r.copies * len(fc.sweep_offsets(r.m, fc.keep_of(r)))
            # ... and under the batch of about eight chunks the planted seams are mostly INSIDE a batch
            eight = set(fc.batch_seams(len(case.data), case.S, case.pre, case.post, 8 * case.S + case.S // 3 + 5))
            assert sum(pl.seam in eight for pl in case.plants) < len(case.plants) / 2
            n += 1
    assert n >= 1 and all(v > 0 for v in near.values()), near
    assert ("odd", False, "quiet") in fc.sweeps(r) or r.name in fc.HEAVY


CHEAP = [r for r in fc.ROUTES if r.name not in fc.HEAVY and r.name != "seg-vlanes-300-2"]


@pytest.mark.parametrize("r", CHEAP, ids=lambda r: r.name)
def test_expectation_is_the_file_semantics(r):
    """The model's rows for the sweeps: every exact plant wholly inside a chunk is a row of that chunk with distance 0;
    Levenshtein and generic: windows reported by two chunks, and chunks whose rows no in-memory search of the file gives
    (the clamps) - the expectation separates the file semantics from the in-memory one."""
    total = [0, 0, 0]
    for (g, text, background) in fc.sweeps(r):
        if g not in ("odd", "smallest", "1024"):
            continue
        case = fc.build(r, fc.stride(r, g), text, background)
        rows = fc.expected(case)
        for i, v in enumerate(fc.check_expectation(case, rows)):
            total[i] += v
        assert [x[4] for x in rows] == sorted(x[4] for x in rows)
    assert total[0] >= len(fc.sweep_offsets(r.m, fc.keep_of(r)))
    if r.kind in ("lev", "generic"):
        assert total[1] > 0, "no window is reported by two chunks"
    if r.kind == "lev":
        assert total[2] > 0, "no chunk differs from the in-memory search"


def test_file_ends_cover_the_existence_rule_and_every_edge_item():
    for r in fc.ROUTES:
        if r.name in fc.HEAVY:
            continue
        for text in (False, True):
            S = fc.odd_stride(r)
            _S, pre, post, chunk_size = fc.geometry(r, S, text)
            sizes, seen = set(), {"start": set(), "end": set()}
            n_chunks = set()
            for case in fc.end_cases(r, S, text, (3, 8)):
                sizes.add(len(case.data))
                n_chunks.add(len(file_model.chunk_bounds(len(case.data), chunk_size, fc.keep_of(r), text)))
                for side in seen:
                    seen[side] |= case.coverage[side]["exact"]
            assert sizes == set(fc.end_sizes(S, post, (3, 8)))
            assert {0, 1, 3, 4, 8, 9} <= n_chunks, n_chunks
            assert seen["start"] == seen["end"] == set(fc.edge_items(r.m, r.k)), r.name
