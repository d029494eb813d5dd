"""Seam-sweep inputs for the FILE stream (fz_stream_*, include/fzhip.h) and their expected raw streams.

find_near_matches_in_file searches a file chunk by chunk; the stream uploads many chunks per batch and searches them as
SEGMENTS of one buffer with per-chunk clamps (fzhip.hip: fz_stream_submit, stream_launch, stream_collect; fz_kernels.h: the
SEG instantiations; fz_device.h: fz_segment).  This module builds files that put a copy of the pattern at EVERY offset
across both seams of a chunk boundary - the start of chunk j (`lo`) and the end of chunk j - 1 (`hi`, `keep` bytes later) -
on chunk boundaries that are also BATCH boundaries when the stream runs with three-chunk batches, and the file ends the
existence rule of the last chunk turns on.  The expected stream is tests/file_model.py (the reference's chunk loop over the
oracle, raw=True) on the whole file: no sparse expectation.  In the spirit of tests/seam_case.py, whose sweep, edits,
backgrounds and alphabets are used here.

    build(route, S, text, background)  -> Case: the chunk-seam sweep, one plant per planted seam
    end_cases(route, S, text, ...)     -> Cases: the file ends, copies that lose 0 .. k characters to either end
    expected(case)                     -> rows (start, end, dist, block, chunk) of the whole file
    batches(n, S, pre, post, B)        -> the batches fz_stream_submit launches when every staging buffer is filled

tests/test_file_seam_case.py checks the construction on the CPU; tests/test_gpu_file_stream_raw.py runs it on the device.
"""
import collections
import random

import numpy as np

from tests import file_model
from tests.seam_case import (DIGITS, DNA, FORM_BAND, FORM_KERNEL, FORM_NONE, LANE, ROW, TILE, WAVE, WIDE, Background,
                             edge_items, edited_copy, quiet_alphabet, sweep_offsets)

MODE = {"exact": 0, "lev": 1, "subs": 2, "generic": 3}       # fuzzysearch_amd._file_stream.MODE_*
SIZE_CAP = 6 << 20                                            # a sweep file is at most this long (see admissible())

Route = collections.namedtuple("Route", "name kind m k limits alpha form env noisy copies")
Plant = collections.namedtuple("Plant", "start data seam side d exact whole")
Case = collections.namedtuple("Case", "route pattern data S pre post chunk_size text plants coverage")
Batch = collections.namedtuple("Batch", "j0 j1 stage_off data_hi")


def _r(name, kind, m, k, form, alpha=DNA, limits=None, env=None, noisy=True, copies=2):
    return Route(name, kind, m, k, limits, alpha, form, env or {}, noisy, copies)


ROUTES = (
    # Levenshtein, k <= 4: the register band inside the SEG scan kernel
    [_r("seg-band-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BAND, alpha=WIDE if mk[0] // (mk[1] + 1) < 6 else DNA)
     for mk in ((8, 1), (12, 1), (20, 2), (24, 3), (40, 4))] +
    # ... dense candidates: the wave's queue overflows, the tile is enumerated inside SEG
    [_r("seg-dense-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BAND) for mk in ((12, 2), (20, 4))] +
    # ... long patterns: fewer than 64 verifying lanes
    [_r("seg-vlanes-%d-%d" % mk, "lev", mk[0], mk[1], FORM_BAND) for mk in ((300, 2), (600, 4))] +
    # Levenshtein, k > 4: hit list + a verification kernel of its own with two candidate segments per hit
    [_r("seg-wf-%d-%d" % mk, "lev", mk[0], mk[1], FORM_KERNEL) for mk in ((24, 5), (54, 8), (64, 15), (128, 31))] +
    [_r("seg-ring-140-34", "lev", 140, 34, FORM_KERNEL, noisy=False),
     # (the pattern in HBM; the oracle's verification is quadratic in m: exact copies only, as in tests/seam_case.py)
     _r("seg-big-1030-2", "lev", 1030, 2, FORM_KERNEL, noisy=False, copies=1),
     _r("seg-forced-20-2", "lev", 20, 2, FORM_KERNEL, env={"FZ_FORCE_BIG_VERIFY": "1"}),
     _r("seg-forced-54-8", "lev", 54, 8, FORM_KERNEL, env={"FZ_FORCE_BIG_VERIFY": "1"})] +
    # substitutions only: the in-memory forms on a buffer that starts anywhere; windows dealt to chunks afterwards
    [_r("file-subs-%d-%d" % mk, "subs", mk[0], mk[1], FORM_BAND, alpha=WIDE) for mk in ((13, 2), (24, 3), (21, 1))] +
    [_r("file-subs-dense-%d-%d" % mk, "subs", mk[0], mk[1], FORM_BAND) for mk in ((12, 3), (20, 4))] +
    # exact (m = 1: keep = 0, chunks do not overlap at all)
    [_r("file-exact-%d" % m, "exact", m, 0, FORM_NONE, alpha=DIGITS if m in (2, 4, 9) else DNA, noisy=m >= 5, copies=1)
     for m in (1, 2, 3, 4, 5, 8, 9, 20, 300)] +
    # generic: win = the segment, segment-major order
    [_r("file-generic-20", "generic", 20, 2, FORM_NONE, limits=(2, 1, 1)),
     _r("file-generic-64", "generic", 64, 5, FORM_NONE, limits=(5, 2, 2), alpha=WIDE)]
)


def route_pattern(route):
    rnd = random.Random(len(route.name) * 7919 + route.m * 31 + route.k)
    return bytes(rnd.choice(route.alpha) for _ in range(route.m))


def kwargs(route):
    """The arguments of find_near_matches_in_file that take the route."""
    if route.kind == "exact":
        return {"max_l_dist": 0}
    if route.kind == "lev":
        return {"max_l_dist": route.k}
    if route.kind == "subs":
        return {"max_substitutions": route.k, "max_insertions": 0, "max_deletions": 0}
    s, i, d = route.limits
    return {"max_substitutions": s, "max_insertions": i, "max_deletions": d, "max_l_dist": route.k}


def keep_of(route):
    kind, _k, _limits, extra = file_model.route(kwargs(route))
    assert kind == route.kind, (route.name, kind)
    return route.m - 1 + extra


# -- geometries --------------------------------------------------------------------------------------------------------------
def smallest_stride(route):
    """The smallest stride fz_stream_open accepts (m + 2k + 2 <= S, pre + post <= S / 2) that the API's planner passes on
    as well (chunk_size >= 2 * keep + 2, _file_stream.plan): a position lies in two chunks almost everywhere."""
    return max(route.m + 2 * route.k + 2, 2 * keep_of(route) + 2)


def odd_stride(route):
    """= 1 mod 16, a few KiB: successive seams step through every lane residue and drift across wave and row seams."""
    s = max(2049, smallest_stride(route) + 17)
    return s + (1 - s) % 16


GEOMETRIES = ("odd", "1024", "4096", "16384", "16383", "16385", "smallest")


def stride(route, geometry):
    return odd_stride(route) if geometry == "odd" else smallest_stride(route) if geometry == "smallest" else int(geometry)


def geometry(route, S, text):
    """-> (S, pre, post, chunk_size): binary chunk j = [j S, j S + C), S = C - keep; text chunk j = [j C - keep, (j + 1) C)."""
    keep = keep_of(route)
    return (S, keep, 0, S) if text else (S, 0, keep, S + keep)


def small_batch(S):
    """batch_bytes that makes every batch THREE chunks (capacity() = 3 S + keep): its seams are the chunk numbers 3, 6, 9, ...
    The smallest batch (batch_bytes = 1) holds two chunks, so its seams are even chunk numbers only and, for any stride, reach
    half of the lane residues at most; the sweep is planted on the three-chunk seams, which walk all 16 for an odd stride."""
    return 2 * S


def plant_step(route, S):
    """Seams of the three-chunk batch between two plants: neighbouring plants, each anywhere in its sweep around either
    seam, keep m + 2k + 8 bytes of background between them."""
    need = 3 * keep_of(route) + 3 * route.m + 4 * route.k + 10
    return -(-need // (3 * S))


def sweep_items(route):
    """(d, exact) of one sweep; sweeps shorter than 16 offsets (m <= 4) are repeated until 16 seams are planted."""
    offs = sweep_offsets(route.m, keep_of(route))
    reps = -(-16 // len(offs))
    return [(d, exact) for exact in (True, False)[:route.copies] for d in offs * reps]


def sweep_size(route, S):
    return (3 * plant_step(route, S) * (len(sweep_items(route)) + 2) + 4) * S + 7


def admissible(route, geometry_name):
    """The stream accepts the stride, and the sweep (one plant per planted seam) fits SIZE_CAP: the long patterns' sweeps
    (m >= 128: 400 .. 3100 offsets) run at the strides of a few KiB and leave the 4 and 16 KiB ones to the shorter ones."""
    S = stride(route, geometry_name)
    if S < smallest_stride(route):
        return False
    return geometry_name in ("odd", "smallest") or sweep_size(route, S) <= SIZE_CAP


# The oracle's verification is quadratic in m and these sweeps hold 500 .. 3600 copies: the long patterns run the sweep at the
# geometries named here instead of all admissible ones.
HEAVY = {"seg-vlanes-600-4": (("odd", True),), "seg-big-1030-2": (("odd", False),),
         "seg-wf-128-31": (("odd", False), ("smallest", True)), "seg-ring-140-34": (("odd", True), ("smallest", False))}


def sweeps(route):
    """[(geometry name, text, background)] of the route's chunk-seam sweeps: quiet at every admissible stride in both file
    modes, noisy at the odd stride (binary) and the smallest one (text)."""
    if route.name in HEAVY:
        return [(g, text, "quiet") for (g, text) in HEAVY[route.name]]
    out = [(g, text, "quiet") for g in GEOMETRIES if admissible(route, g) for text in (False, True)]
    if route.noisy:
        out += [("odd", False, "noisy"), ("smallest", True, "noisy")]
    return out


# -- the batching rule of fz_stream_submit, restated ---------------------------------------------------------------------------
def capacity(S, pre, post, batch_bytes):
    return max(batch_bytes, S + pre + post) + S + pre + post


def segments_at_eof(n, S, post):
    return 0 if n == 0 else 1 if n <= post else (n - post - 1) // S + 1


def batches(n, S, pre, post, batch_bytes):
    """The batches of a file of n bytes when every staging buffer is filled before it is submitted (a short fill is the
    last one): [(j0, j1, file offset of the batch's buffer, end of its data)]."""
    cap = capacity(S, pre, post, batch_bytes)
    out, stage_off, next_seg = [], 0, 0
    while True:
        data_end = min(n, stage_off + cap)
        eof = n < stage_off + cap
        j1 = segments_at_eof(data_end, S, post) if eof else ((data_end - post) // S if data_end >= post + S else 0)
        if j1 > next_seg:
            out.append(Batch(next_seg, j1, stage_off, data_end if eof else j1 * S + post))
            next_seg = j1
        else:
            assert eof, "staging buffer smaller than one chunk"
        if eof:
            return out
        stage_off = max(max(0, j1 * S - pre), stage_off)


def batch_seams(n, S, pre, post, batch_bytes):
    """Chunk numbers j whose boundary (chunk j - 1 | chunk j) separates two batches."""
    return [b.j1 for b in batches(n, S, pre, post, batch_bytes)[:-1]]


# -- the chunk-seam sweep ------------------------------------------------------------------------------------------------------
def seam_bytes(j, S, pre, post):
    """(lo, hi) of the boundary in front of chunk j: chunk j starts at lo, chunk j - 1 ends at hi = lo + keep."""
    return j * S - pre, j * S + post


def _background(route, p, background, seed):
    return Background(background, quiet_alphabet(p) if background == "quiet" else bytes(sorted(set(route.alpha))), seed)


NEAR = (("wave", WAVE), ("row", ROW), ("tile", TILE))


def _off_grid(B, unit):
    return min(B % unit, unit - B % unit)


def build(route, S, text, background="quiet", seed=1):
    """-> Case.  For every d of sweep_offsets(m, keep) an exact and an edited copy (routes with copies = 1: exact only), each
    at B + d for a seam B of its own; the side flips with every 16th d, with exact / edited and with the file mode, so that
    every d meets `lo` and `hi`, exact on one side and edited on the other, and 16 successive seams lie on one side.  The
    planted chunk boundaries are batch boundaries of the three-chunk batch (batch_seams(..., small_batch(S))).  Behind the
    sweep, for each of wave / row / tile that no planted seam lies within `keep` of: an exact copy (d = 0) on the next seam
    that does, if one exists within 1 MiB (coverage["unattainable"] names the others)."""
    p = route_pattern(route)
    m, k = route.m, route.k
    keep = keep_of(route)
    S, pre, post, chunk_size = geometry(route, S, text)
    offs = sweep_offsets(m, keep)
    items = sweep_items(route)
    step = plant_step(route, S)
    first = next(q for q in range(1, 10 ** 6) if 3 * q * S - pre + offs[0] >= 0)
    rnd = random.Random(seed * 1000003 + S)
    alpha = bytes(sorted(set(route.alpha)))
    placed = []                                                  # (chunk number, side, d, exact)
    for i, (d, exact) in enumerate(items):
        idx = i % (len(items) // route.copies)
        side = "lo" if (idx // 16 + int(text) + int(not exact)) % 2 == 0 else "hi"
        placed.append((3 * (first + i * step), side, d, exact))
    unattainable = set()
    q = first + len(items) * step
    for name, unit in NEAR:
        if any(_off_grid(seam_bytes(j, S, pre, post)[side == "hi"], unit) <= keep for (j, side, _d, _e) in placed):
            continue
        hit = next(((3 * qq, side) for qq in range(q, q + min(6000, (1 << 20) // (3 * S)) + 1) for side in ("lo", "hi")
                    if _off_grid(seam_bytes(3 * qq, S, pre, post)[side == "hi"], unit) <= keep), None)
        if hit is None:
            unattainable.add(name)
        else:
            placed.append((hit[0], hit[1], 0, True))
            q = hit[0] // 3 + step
    n = (placed[-1][0] + 4) * S + post + 7
    bg = _background(route, p, background, seed)
    data = bg.fill(n).copy()
    plants = []
    cover = {side: {"exact": set(), "edited": set()} for side in ("lo", "hi")}
    cover["seams"], cover["unattainable"] = [], unattainable
    for (j, side, d, exact) in placed:
        B = seam_bytes(j, S, pre, post)[side == "hi"]
        v = p if exact else edited_copy(rnd, p, k, alpha, route.kind == "subs", route.limits)
        assert 0 <= B + d and B + d + len(v) <= n
        data[B + d:B + d + len(v)] = np.frombuffer(v, dtype=np.uint8)
        plants.append(Plant(B + d, v, j, side, d, exact, True))
        cover[side]["exact" if exact else "edited"].add(d)
        cover["seams"].append(B)
    return Case(route, p, data.tobytes(), S, pre, post, chunk_size, text, plants, cover)


def end_sizes(S, post, js):
    """File lengths around the existence rule of the last chunk (chunk j >= 1 exists iff j S + post < n)."""
    out = [0, 1, post, post + 1]
    for j in js:
        out += [j * S + post - 1, j * S + post, j * S + post + 1, j * S, j * S - 1, j * S + 1]
    return sorted(set(out))


def end_cases(route, S, text, js, background="quiet", seed=1):
    """Small files of every length of end_sizes(): a copy at the START and one at the END of the file, d >= 0: whole, d bytes
    off the edge; d < 0: -d characters lost to it (edge_items) - every item exact and, whole copies, edited, over as many
    files as that takes."""
    p = route_pattern(route)
    m, k = route.m, route.k
    S, pre, post, chunk_size = geometry(route, S, text)
    sizes = end_sizes(S, post, js)
    items = edge_items(m, k)
    bg = _background(route, p, background, seed)
    rnd = random.Random(seed * 7 + S)
    alpha = bytes(sorted(set(route.alpha)))
    turn = {"start": 0, "end": k + 1}                           # the next item of either end: it moves on when a file took it
    done = {"start": 0, "end": 0}
    i = 0
    while i < len(sizes) or min(done.values()) < route.copies * len(items):
        n = sizes[i % len(sizes)]
        i += 1
        data = bg.fill(n).copy()
        plants = []
        cover = {side: {"exact": set(), "edited": set()} for side in ("start", "end")}
        for side in ("start", "end"):
            d = items[turn[side] % len(items)]
            exact = (done[side] // len(items)) % 2 == 0
            if d >= 0:
                v = p if exact else edited_copy(rnd, p, k, alpha, route.kind == "subs", route.limits)
                at = d if side == "start" else n - d - len(v)
            else:
                v = p[-d:] if side == "start" else p[:m + d]
                at = 0 if side == "start" else n - len(v)
            if at < 0 or at + len(v) > n or any(at < q.start + len(q.data) + m + 2 * k + 8 for q in plants):
                continue
            data[at:at + len(v)] = np.frombuffer(v, dtype=np.uint8)
            plants.append(Plant(at, v, 0 if side == "start" else n, side, d, exact or d < 0, d >= 0))
            cover[side]["exact" if plants[-1].exact else "edited"].add(d)
            turn[side] += 1
            done[side] += 1
        yield Case(route, p, data.tobytes(), S, pre, post, chunk_size, text, plants, cover)


def expected(case):
    """(start, end, dist, block, chunk) of the whole file: tests/file_model.py, unreduced."""
    kind, rows = file_model.file_raw(case.pattern, case.data, kwargs(case.route), case.chunk_size, case.text, raw=True)
    assert kind == case.route.kind
    return rows


# -- conditions on the inputs --------------------------------------------------------------------------------------------------
def check_coverage(case):
    """Every d, exact and (copies = 2) edited, on a chunk seam, and on both sides; the plants' seams are batch seams of the
    three-chunk batch (and those with an even chunk number of the smallest batch as well).  Odd strides (one plant per three-chunk seam): the planted
    seams take all 16 lane residues.  Every stride: some planted seam lies within `keep` of a wave, of a row and of a tile seam
    of the file - where the single batch's buffer has them - unless no seam of the geometry does within 1 MiB behind the
    sweep (coverage["unattainable"]).  -> {"wave" / "row" / "tile": planted seams that near, "residues": lane residues}."""
    r, cov = case.route, case.coverage
    keep = keep_of(r)
    want = set(sweep_offsets(r.m, keep))
    assert cov["lo"]["exact"] | cov["hi"]["exact"] == want
    if r.copies == 2:
        assert cov["lo"]["edited"] | cov["hi"]["edited"] == want
        assert cov["lo"]["exact"] | cov["lo"]["edited"] == want and cov["hi"]["exact"] | cov["hi"]["edited"] == want
    three = set(batch_seams(len(case.data), case.S, case.pre, case.post, small_batch(case.S)))
    two = set(batch_seams(len(case.data), case.S, case.pre, case.post, 1))
    assert all(pl.seam in three for pl in case.plants)
    assert all(pl.seam in two for pl in case.plants if pl.seam % 2 == 0)
    seams = np.array(cov["seams"])
    out = {"residues": len(set((seams % LANE).tolist()))}
    if case.S % 2 and plant_step(r, case.S) == 1:              # (every odd stride of a KiB or more)
        assert out["residues"] == 16, (r.name, case.S, out["residues"])
    for name, unit in NEAR:
        out[name] = int((np.minimum(seams % unit, unit - seams % unit) <= keep).sum())
        assert out[name] > 0 or name in cov["unattainable"], (r.name, case.S, case.text, name)
    return out


def coverage_line(name, case, form=None):
    cov = case.coverage
    near = check_coverage(case)
    return ("file seams %-22s %-6s S %5d form %s | lo %d+%d d, hi %d+%d d, %d chunks, %d residues, seams within keep of "
            "wave/row/tile %d/%d/%d%s" % (
                name, "text" if case.text else "binary", case.S, form, len(cov["lo"]["exact"]), len(cov["lo"]["edited"]),
                len(cov["hi"]["exact"]), len(cov["hi"]["edited"]),
                len(file_model.chunk_bounds(len(case.data), case.chunk_size, keep_of(case.route), case.text)), near["residues"],
                near["wave"], near["row"], near["tile"],
                (" (no seam can: %s)" % ",".join(sorted(cov["unattainable"]))) if cov["unattainable"] else ""))


def check_expectation(case, rows, count=True):
    """The expectation is not vacuous, and it is the FILE's semantics: every exact plant that lies wholly inside a chunk is a
    row of that chunk with distance 0 (generic: a row of that chunk covers it); Levenshtein and generic: windows
    reported by two chunks and chunks with rows that the in-memory search of the file does not have are COUNTED (which d
    and side show them depends on the route; tests/test_file_seam_case.py holds the counts per route; count=False leaves
    the counting, a second pass of the oracle over the file, out).  -> (rows of plants found, windows in two chunks, chunks
    that differ from the in-memory stream)."""
    import oracle
    r = case.route
    m = r.m
    bounds = file_model.chunk_bounds(len(case.data), case.chunk_size, keep_of(r), case.text)
    by_chunk = collections.defaultdict(list)
    for row in rows:
        by_chunk[row[4]].append(row)
    found = 0
    for pl in case.plants:
        if not (pl.exact and pl.whole):
            continue
        for j in (pl.seam - 1, pl.seam):
            if 0 <= j < len(bounds) and bounds[j][0] <= pl.start and pl.start + m <= bounds[j][1]:
                if r.kind == "generic":
                    ok = any(row[0] <= pl.start + r.k and row[1] >= pl.start + m - r.k for row in by_chunk[j])
                else:
                    ok = any(row[:3] == (pl.start, pl.start + m, 0) for row in by_chunk[j])
                assert ok, (r.name, "exact plant without a row in chunk", j, pl.start)
                found += 1
    twice = differ = 0
    if count and r.kind in ("lev", "generic") and any(pl.side in ("lo", "hi") for pl in case.plants):
        seen = {}
        for row in rows:
            if seen.setdefault(row[:2], row[4]) != row[4]:
                twice += 1
        if r.kind == "lev":
            whole = collections.defaultdict(list)
            for (s, e, d, g) in oracle.lev_ngrams_raw(case.pattern, case.data, r.k):
                whole[(s, e, d, g)].append(1)
            for j, (a, b) in enumerate(bounds):
                if any((row[0], row[1], row[2], row[3]) not in whole for row in by_chunk[j]):
                    differ += 1
    return found, twice, differ
