"""tests/seam_case.py on the CPU: the licence for holding the device against the SPARSE expected stream at sizes where the
oracle never runs on the whole text, and the conditions the built inputs have to meet (they are conditions, not measurements)."""
import pytest

from tests import seam_case as sc

N_CUS = 256


def test_layout_constants_mirror_the_kernel_header():
    assert sc.header_layout() == (sc.LANE, sc.WAVE, sc.ROW, sc.TILE) == (16, 1024, 4096, 16384)


@pytest.mark.parametrize("route", sc.ROUTES, ids=lambda r: r.name)
def test_sparse_stream_is_the_full_oracle_stream(route):
    """Every parameter set of the device tests at a CPU-sized n (about 4 MiB, odd length; longer where the sweep needs more
    seams), quiet background: sparse expected stream == oracle on the whole text, order included; every d of every class
    placed as an exact and as an edited copy, no plant skipped (build() asserts room for every one); every exact copy has
    its row."""
    p = sc.route_pattern(route)
    case = sc.build(p, route.k, route.n, N_CUS, "quiet", pattern_alphabet=route.alpha, **sc.route_args(route))
    sparse = sc.sparse_expected(route.kind, case)
    assert sparse == sc.expected(route.kind, case)
    sc.check_exact_copies_found(route.kind, case, sparse)
    sc.check_coverage(case.coverage, route.m, route.k, route.classes, case.plan, (route.n + sc.TILE - 1) // sc.TILE,
                      edited=route.copies == 2)
    assert len(case.plants) == len(route.classes) * route.copies * len(sc.sweep_offsets(route.m, route.k))
    for a, b in zip(case.plants, case.plants[1:]):
        assert a.start + len(a.data) < b.start
    seams = {"wave": lambda s: s % sc.WAVE == 0 and s % sc.ROW, "row": lambda s: s % sc.ROW == 0 and s % sc.TILE,
             "tile": lambda s: s % sc.TILE == 0}
    for pl in case.plants:
        assert seams[pl.cls](pl.seam) and pl.start == pl.seam + pl.d


@pytest.mark.parametrize("route", sc.ROUTES, ids=lambda r: r.name)
def test_edge_texts_sparse_stream_and_coverage(route):
    """The few-seam classes (first tile seam, start, end; the tails 1, 15, 16, 17 and an odd one) on their small texts,
    both backgrounds: sparse == full on the quiet one, every d of every class over the phases, exact copies found."""
    covers = []
    for case in sc.edge_cases(route, N_CUS):
        sparse = sc.sparse_expected(route.kind, case)
        assert sparse == sc.expected(route.kind, case)
        sc.check_exact_copies_found(route.kind, case, sparse)
        covers.append(case.coverage)
    sc.check_coverage(sc.merge_coverage(covers), route.m, route.k, ("first", "start", "end"))
    if route.m <= 64:
        for tail in sc.EDGE_TAILS[1:]:
            cov = sc.merge_coverage(c.coverage for c in sc.edge_cases(route, N_CUS, classes=("end",), tail=tail))
            sc.check_coverage(cov, route.m, route.k, ("end",))


@pytest.mark.parametrize("nul", ["head", "tail"])
def test_nul_patterns_on_the_edge_texts(nul):
    route = next(r for r in sc.ROUTES if r.name == "band-L6-k2")
    p = sc.route_pattern(route, nul)
    assert (p[:2] if nul == "head" else p[-2:]) == b"\0\0"
    for case in sc.edge_cases(route, N_CUS, p=p, classes=("start", "end")):
        assert sc.sparse_expected("lev", case) == sc.expected("lev", case)


@pytest.mark.parametrize("n_cus", [8, 64, 256, 304])
def test_tile_map_follows_the_scan_plan(n_cus):
    """tile -> (workgroup, iteration, region) against fz_debug_scan_plan: every tile has exactly one owner and iteration,
    the workgroups' iterations are 0, 1, 2 .. without gaps, inside the grid; the plants of a text in the tapered regime reach
    iterations 0, 1 and last and the first and last tile of every region."""
    p = b"ACGTTGCAACGGTACCATGA"
    for n, shares in (((4 << 20) + 777, 0), ((64 << 20) + 5, 0), ((1 << 30) + 12345, 0), ((1 << 30) + 12345, 1)):
        grid, _form, ov, regions = sc.scan_plan(p, 2, n, n_cus, shares)
        ntiles = (n + sc.TILE - 1) // sc.TILE
        assert ov == bool(shares) and (not ov or not regions)
        seen = {}
        for T in range(ntiles):
            wg, it, reg, last = sc.tile_owner(T, ntiles, grid, regions)
            assert 0 <= wg < grid and (wg, it) not in seen
            seen[(wg, it)] = T
            if last:
                assert (wg, it + 1) not in seen
        per_wg = {}
        for (wg, it) in seen:
            per_wg[wg] = max(per_wg.get(wg, -1), it)
        assert all((wg, i) in seen for wg, top in per_wg.items() for i in range(top + 1))
        assert len(per_wg) == grid
    # the tapered plan of 1 GiB on this CU count (or, on a small chip, its plain one): tile and region classes, plants only
    n = (1 << 30) + 12345
    ntiles = (n + sc.TILE - 1) // sc.TILE
    case = sc.build(p, 2, n, n_cus, "quiet", classes=("tile", "region"), copies=1, dry=True)
    sc.check_coverage(case.coverage, 20, 2, ("tile",), case.plan, ntiles, edited=False)
    if case.plan[3]:
        nseams = len(sc.region_seams(ntiles, case.plan[3], n))
        covers = [case.coverage] + [sc.build(p, 2, n, n_cus, "quiet", classes=("region",), phase=ph, dry=True).coverage
                                    for ph in range(1, sc.phases("region", 20, 2, nseams) // 2)]
        sc.check_coverage(sc.merge_coverage(covers), 20, 2, ("region",), case.plan, ntiles, edited=False)
