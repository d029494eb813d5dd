"""-m gpu: end overlaps on the device (fz_batch_end_overlaps / Engine.batch_end_overlaps / find_end_overlaps_batch) — every
array against the model of the definition (tests/overlap_model.py), exactly, for every generated read."""
import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import overlap_case as oc
from tests import overlap_model as om
from tests import records_model as rm
from tests.test_overlap_host import MODES, assert_same

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("mode", sorted(MODES), ids=lambda m: MODES[m])
CHUNK = {om.LEV: 8, om.SUBS: 64}                            # patterns per launch (csrc/fz_device.h: FZ_OVL_CHUNK_*)


def device(engine, mode, patterns, reads, k, o):
    """Engine.batch_end_overlaps over a fresh upload -> ((pattern, overlap, dist, start), stats of the call)"""
    blob, _lens = oc.pack(reads)
    h = engine.upload_batch(blob, oc.offsets(reads))
    try:
        rows = engine.batch_end_overlaps(h, mode, patterns, k, o)
        st = engine.stats()
    finally:
        h.release()
    assert rows.dtype == _native.overlap_dtype() and len(rows) == len(reads)
    return oc.rows_arrays(rows), st


# ---- 1. every prefix, every edit, every alignment, every kind of neighbour: one launch per mode

SWEEP_P, SWEEP_K, SWEEP_O = b"ACGTTGCAAGCCTAGGATCC", 2, 3


def sweep_reads():
    """The pattern's prefixes of o .. 19 bytes with 0, 1 and 2 substitutions, insertions and deletions, each at the end of a
    read that ends at every offset mod 16 of the packed bytes (a filler read in front steers it), empty reads and reads of
    1 .. 4 bytes in between, the adversarial neighbours in the middle, a prefix in the first and in the last read."""
    rng = oc.rng_of("sweep")
    reads = [b"GATTA" + SWEEP_P[:9]]
    at, short = len(reads[0]), 0
    variants = [(0, "s")] + [(e, kind) for e in (1, 2) for kind in "sid"]
    for target in range(16):
        for i in range(SWEEP_O, len(SWEEP_P)):
            for edits, kind in variants:
                read = oc.planted_read(rng, SWEEP_P, i, edits, rng.randrange(0, 30), kinds=kind)
                filler = oc.rand_bytes(rng, (target - at - len(read)) % 16 + (16 if rng.random() < 0.3 else 0))
                reads += [filler, read]
                at += len(filler) + len(read)
                assert at % 16 == target
                if rng.random() < 0.15:
                    reads.append(oc.rand_bytes(rng, short % 5))  # 0 .. 4 bytes
                    at += short % 5
                    short += 1
        if target == 8:
            reads += oc.adversarial_neighbours(SWEEP_P, SWEEP_O)
            at = sum(len(r) for r in reads)
    reads.append(b"CC" + SWEEP_P[:14])
    return reads


@pytest.fixture(scope="module")
def sweep():
    reads = sweep_reads()
    return reads, {mode: om.end_overlaps(mode, [SWEEP_P], reads, SWEEP_K, SWEEP_O) for mode in MODES}


@BOTH
def test_seam_sweep(engine, sweep, mode):
    reads, want = sweep
    got, st = device(engine, mode, [SWEEP_P], reads, SWEEP_K, SWEEP_O)
    assert_same(got, want[mode], MODES[mode])
    assert st["filter_launches"] == 1
    found = want[mode][0] >= 0
    assert found[0] and found[-1] and found.sum() >= 500 and (~found).sum() >= 1000     # (an edited prefix of under 10 bytes is over its scaled budget)
    assert set(want[mode][1][found].tolist()) == set(range(SWEEP_O, len(SWEEP_P)))       # every prefix length is an answer somewhere


# ---- 2. shapes

@BOTH
@pytest.mark.parametrize("m,k", [(1, 0), (2, 0), (8, 1), (33, 3), (64, 16), (64, 0)])
def test_shapes(engine, mode, m, k):
    rng = oc.rng_of("shapes", mode, m, k)
    for alphabet in (b"ACGT", bytes([0x00, 0xff])):
        p = oc.rand_bytes(rng, m, alphabet)
        reads = oc.mixed_reads(rng, [p], k, 150, alphabet) + [b"", p, p[:m - 1], p[:m // 2]]
        ones = {}
        for o in (1, 3, m):
            got, _st = device(engine, mode, [p], reads, k, o)
            assert_same(got, om.end_overlaps(mode, [p], reads, k, o), "%s m=%d k=%d o=%d" % (MODES[mode], m, k, o))
            ones[o] = int((got[0] >= 0).sum())
        assert ones[m] == 0 and (m < 8 or ones[1] >= 30), ones


# ---- 3. panels: more patterns than one launch holds

@pytest.fixture(scope="module")
def panel():
    rng = oc.rng_of("panel")
    k, o = 2, 3
    patterns = [oc.TIE_Y, oc.TIE_X] + [oc.rand_bytes(rng, rng.randrange(4, 65)) for _ in range(68)]
    patterns[8] = patterns[5]                                # a duplicate inside the panel of 9
    patterns[69] = patterns[1]
    reads = [oc.TIE_READ] + oc.mixed_reads(rng, patterns, k, 120) + [b"AC" + patterns[5][:len(patterns[5]) - 1]]
    return k, o, patterns, reads, {mode: om.per_pattern(mode, patterns, reads, k, o) for mode in MODES}


@BOTH
@pytest.mark.parametrize("n_pats", [1, 2, 9, 64, 70])
def test_panels(engine, panel, mode, n_pats):
    k, o, patterns, reads, ones = panel
    got, st = device(engine, mode, patterns[:n_pats], reads, k, o)
    want = om.choose(ones[mode], reads, n_pats)
    assert_same(got, want, "%s %d patterns" % (MODES[mode], n_pats))
    assert st["filter_launches"] == -(-n_pats // CHUNK[mode])
    if n_pats == 70:
        assert st["filter_launches"] > 1 and len(set(want[0].tolist())) > 20
        assert 69 not in want[0] and 8 not in want[0]        # a pattern listed twice answers with its first position
    if n_pats >= 2 and mode == om.LEV:
        assert (want[0][0], want[2][0]) == (1, 0)            # ten matched bytes both, X without an edit: the tie goes to the distance


# ---- 4. read counts

@pytest.fixture(scope="module")
def many():
    rng = oc.rng_of("many")
    reads = oc.mixed_reads(rng, [SWEEP_P], SWEEP_K, 5000, longest=60)
    return reads, {mode: om.end_overlaps(mode, [SWEEP_P], reads, SWEEP_K, 2) for mode in MODES}


@BOTH
def test_read_counts(engine, many, mode):
    reads, want = many
    for count in (1, 63, 64, 65, 257, 5000):
        got, _st = device(engine, mode, [SWEEP_P], reads[:count], SWEEP_K, 2)
        assert_same(got, tuple(x[:count] for x in want[mode]), "%s %d reads" % (MODES[mode], count))
    got, st = device(engine, mode, [SWEEP_P], [b""] * 300, SWEEP_K, 2)
    assert got[0].tolist() == [-1] * 300 and got[3].tolist() == [0] * 300 and st["filter_launches"] == 0


# ---- 5. handles, and the public call

def test_handles_answer_as_the_list_of_their_sequences(engine):
    rng = oc.rng_of("handles")
    adapter = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    reads = []
    for _ in range(400):
        body = oc.rand_bytes(rng, rng.randrange(20, 60))
        reads.append(body + oc.edited(rng, adapter[:rng.randrange(3, 33)], rng.randrange(0, 2)) if rng.random() < 0.5 else body)
    held = fa.resident_records(rm.fastq(reads), engine=engine)
    try:
        trimmed = held.derive(ends=[max(len(r) - 4, 0) for r in reads])
        minus = held.derive(reverse=True, translate=fa.DNA_COMPLEMENT)
        rc_adapter = adapter.translate(fa.DNA_COMPLEMENT)[::-1]
        for what, handle, patterns in (("records", held, [adapter]), ("trimmed", trimmed, [adapter, rc_adapter]), ("minus", minus, [rc_adapter, adapter])):
            seqs = [bytes(s) for s in handle.sequences]
            for kw, mode, k in ((dict(max_l_dist=3), om.LEV, 3), (dict(max_substitutions=2, max_insertions=0, max_deletions=0), om.SUBS, 2)):
                res = fa.find_end_overlaps_batch(patterns, handle, min_overlap=3, **kw)
                assert_same(oc.result_arrays(res), om.end_overlaps(mode, patterns, seqs, k, 3), what)
                assert_same(oc.result_arrays(fa.find_end_overlaps_batch(patterns, seqs, min_overlap=3, **kw)), oc.result_arrays(res), what + " as a list")
        assert [bytes(s) for s in held.sequences] == reads
        trimmed.release()
        minus.release()
    finally:
        held.release()


def test_trimming_at_start_leaves_nothing_as_good_to_find(engine):
    rng = oc.rng_of("round trip")
    adapter = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    reads = []
    for _ in range(500):
        body = bytes(rng.choice(b"xyzw") for _ in range(rng.randrange(0, 50)))        # a background free of the adapter's symbols
        reads.append(body + oc.edited(rng, adapter[:rng.randrange(1, 33)], rng.randrange(0, 3)) if rng.random() < 0.7 else body)
    held = fa.resident_batch(reads, engine=engine)
    try:
        first = fa.find_end_overlaps_batch(adapter, held, max_l_dist=3)
        assert_same(oc.result_arrays(first), om.end_overlaps(om.LEV, [adapter], reads, 3, 3), "first")
        assert repr(first) == "EndOverlaps(500 sequences, %d found)" % (first.pattern >= 0).sum() and (first.pattern >= 0).sum() >= 200
        cut = held.derive(ends=first.start)
        rest = [r[:s] for r, s in zip(reads, first.start.tolist())]
        assert [bytes(s) for s in cut.sequences] == rest
        second = fa.find_end_overlaps_batch(adapter, cut, max_l_dist=3)
        assert_same(oc.result_arrays(second), om.end_overlaps(om.LEV, [adapter], rest, 3, 3), "second")
        again = second.pattern >= 0
        assert not (again & (first.pattern < 0)).any()
        assert ((second.overlap - second.dist)[again] < (first.overlap - first.dist)[again]).all()
        cut.release()
    finally:
        held.release()


def test_handles_the_call_does_not_take(engine):
    plain = engine.upload(b"ACGT" * 100)
    try:
        plain.n_seqs = 0
        with pytest.raises(_native.UnsupportedSearch, match="takes a batch handle"):
            engine.batch_end_overlaps(plain, om.LEV, [b"ACGTACGT"], 1, 3)
    finally:
        plain.release()
    blob, _lens = oc.pack([b"ACGTACGT", b"TT"])
    h = engine.upload_batch(blob, oc.offsets([b"ACGTACGT", b"TT"]))
    try:
        with pytest.raises(ValueError, match="min_overlap must be at least 1"):
            engine.batch_end_overlaps(h, om.LEV, [b"ACGTACGT"], 1, 0)
        rows = engine.batch_end_overlaps(h, om.SUBS, [], 0, 3)
        assert rows["pattern"].tolist() == [0xffff, 0xffff] and rows["start"].tolist() == [8, 2]
        ms = engine.overlap_ms()
        assert set(ms) == {"tables_h2d", "kernels", "rows_d2h", "call"} and ms["call"] >= 0
    finally:
        h.release()
