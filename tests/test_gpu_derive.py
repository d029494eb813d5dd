"""-m gpu: derive_batch / fz_batch_derive — a batch made from a batch on the device — against the three-line model
(tests/derive_model.py): the packed bytes and tables of the four forms on a case built for the gather's seams, the scan's
seams, the degenerate cases, the verdict on bad items, and the result used as a batch by every batch search."""
import functools
import random

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import derive_model
from tests import records_model as rm
from tests import fasta_model as fm

pytestmark = pytest.mark.gpu

TILE = 16384
FORMS = [(False, False), (True, False), (False, True), (True, True)]       # (reverse, translate)
FORM_IDS = ["plain", "reverse", "translate", "both"]
SEAM_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 150, 16383, 16384, 16385, 40000]


def dna(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def _table():
    t = list(range(256))
    random.Random(256).shuffle(t)
    return bytes(t)


TABLE = _table()                                                           # a permutation of all byte values


@functools.lru_cache(maxsize=None)
def seam_case(delta):
    """-> (parent sequences, index, starts, ends): a few thousand outputs, a few hundred KiB, their total a multiple of the
    16 KiB tile plus delta (-1, 0, 1)."""
    rnd = random.Random(18)
    seqs = [bytes(rnd.randrange(256) for _ in range(n)) for n in SEAM_LENGTHS]
    big = len(seqs) - 1
    items = []
    for a in range(16):                                                     # every source residue, every length 0 .. 48
        for n in range(49):
            s = a + 16 * rnd.randrange(2000)
            items.append((big, s, s + n))
    items += [(i, 0, len(s)) for i, s in enumerate(seqs)]                   # whole sequences, the long ones across tile seams
    for _ in range(1500):                                                   # short cuts of everything, empty ones among them
        i = rnd.randrange(len(seqs))
        b = rnd.randint(0, min(len(seqs[i]), 64))
        items.append((i, rnd.randint(0, b), b))
    total = sum(b - a for _i, a, b in items)
    fill = TILE - total % TILE                                              # 1 .. TILE: this output ends exactly on a tile seam
    items.append((big, 5, 5 + fill))
    items.append((big, 3, 3 + TILE - 7))                                    # ends 7 in front of the next seam
    items.append((big, 11, 11 + 20))                                        # straddles it
    items.append((big, 9, 9 + TILE - 13 + delta))                           # the total: a multiple of the tile + delta
    index, starts, ends = (np.array(c) for c in zip(*items))
    assert int((ends - starts).sum()) % TILE == delta % TILE
    at = np.concatenate([[0], np.cumsum(ends - starts)])
    offs = derive_model.offsets(seqs)
    src = np.array([offs[i] for i in index]) + starts
    assert set((src % 16).tolist()) == set(range(16)) and set((at[:-1] % 16).tolist()) == set(range(16))
    assert set(range(49)) <= set((ends - starts).tolist()) and 2000 < len(items) < 5000 and 100 << 10 < at[-1] < 400 << 10
    seam = at[-4]                                                           # the end of the output that fills its tile
    assert seam % TILE == 0 and at[-3] == seam + TILE - 7 and at[-2] == seam + TILE + 13
    return seqs, index, starts, ends


def check_handle(engine, handle, seqs, index, starts, ends, reverse, translate):
    """The derived handle's bytes and tables against the model's."""
    want = derive_model.model(seqs, index, starts, ends, reverse, TABLE if translate else None)
    assert handle.n_seqs == len(want) and len(handle) == sum(map(len, want)) == handle.info["packed_bytes"]
    assert handle.info["longest"] == max([len(w) for w in want] or [0])
    got = engine.batch_bytes(handle)
    assert got == b"".join(want)
    src, got_ends = engine.batch_tables(handle)
    assert got_ends.tolist() == np.cumsum([len(w) for w in want]).tolist()
    offs = derive_model.offsets(seqs)
    n_out = len(want)
    idx = range(n_out) if index is None else index
    a = [0] * n_out if starts is None else starts
    assert src.tolist() == [offs[int(i)] + int(s) for i, s in zip(idx, a)]   # the lowest source byte in the parent's packed bytes


@pytest.fixture(scope="module")
def seam_parent(engine):
    seqs = seam_case(0)[0]
    held = fa.resident_batch(seqs, engine=engine)
    yield held
    held.release()


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_bytes_and_tables_on_the_seam_case(engine, seam_parent, form, delta):
    seqs, index, starts, ends = seam_case(delta)
    reverse, translate = form
    h = engine.derive_batch(seam_parent.handle, index.astype(np.uint32), starts.astype(np.uint64), ends.astype(np.uint64),
                            reverse=reverse, translate=TABLE if translate else None)
    try:
        check_handle(engine, h, seqs, index, starts, ends, reverse, translate)
    finally:
        h.release()


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_scan_seams(engine, off):
    """n_out one below, at and one above the items of one scan workgroup: the scan over n_out + 1 entries goes to two levels."""
    rnd = random.Random(off)
    seqs = [dna(rnd, n) for n in (0, 1, 7, 16, 40, 150)]
    n_out = _native.scan_items() + off
    index = np.array([rnd.randrange(len(seqs)) for _ in range(n_out)], dtype=np.uint32)
    ends = np.array([rnd.randint(0, len(seqs[i])) for i in index], dtype=np.uint64)
    starts = np.array([rnd.randint(0, int(e)) for e in ends], dtype=np.uint64)
    parent = engine.upload_batch(b"".join(seqs), np.array(derive_model.offsets(seqs), dtype=np.uint64))
    try:
        for reverse, translate in FORMS:
            h = engine.derive_batch(parent, index, starts, ends, reverse=reverse, translate=TABLE if translate else None)
            try:
                check_handle(engine, h, seqs, index, starts, ends, reverse, translate)
            finally:
                h.release()
    finally:
        parent.release()


def test_degenerate_cases(engine):
    rnd = random.Random(7)
    seqs = [dna(rnd, n) for n in (40, 0, 17, 150)]
    held = fa.resident_batch(seqs, engine=engine)
    empty = engine.upload_batch(b"", np.zeros(1, dtype=np.uint64))
    try:
        for reverse, translate in FORMS:
            kw = dict(reverse=reverse, translate=TABLE if translate else None)
            for index, starts, ends in (([], [], []),                                              # n_out = 0
                                        ([0, 3, 1, 2], [40, 7, 0, 17], [40, 7, 0, 17]),            # every output empty
                                        (None, None, None),                                        # identity (with X)
                                        ([3, 3, 0, 3, 2, 3, 0, 0], None, None),                    # repeats: larger than the parent
                                        (None, [1, 0, 17, 100], None), (None, None, [39, 0, 1, 149])):
                d = held.derive(index, starts, ends, **kw)
                try:
                    check_handle(engine, d.handle, seqs, index, starts, ends, reverse, translate)
                    assert len(d) == (4 if index is None else len(index)) and list(d.sequences) == derive_model.model(seqs, index, starts, ends, **kw)
                    assert d.lengths.tolist() == [len(s) for s in d.sequences]
                finally:
                    d.release()
            h = engine.derive_batch(empty, reverse=reverse, translate=TABLE if translate else None)   # an empty parent
            assert h.n_seqs == 0 and len(h) == 0 and engine.batch_bytes(h) == b""
            h.release()
        ident = held.derive()
        assert engine.batch_bytes(ident.handle) == engine.batch_bytes(held.handle) == b"".join(seqs)
        assert len(held.derive(index=[3] * 9).handle) == 9 * 150 > len(held.handle)
        with pytest.raises(IndexError, match="item 0:"):                                           # nothing is in an empty parent
            engine.derive_batch(empty, np.zeros(2, dtype=np.uint32))
    finally:
        empty.release()
        held.release()


@pytest.mark.parametrize("reason", [1, 2, 3])
def test_bad_items(engine, reason):
    """Each reason at an item of the first workgroup and at one far beyond it; of two bad items the lower one is reported;
    no handle is made and the next call works."""
    rnd = random.Random(reason)
    seqs = [dna(rnd, n) for n in (10, 2, 0, 5)]
    n_out = 70010
    held = fa.resident_batch(seqs, engine=engine)

    def tables():
        index = np.array([rnd.randrange(4) for _ in range(n_out)], dtype=np.uint32)
        ends = np.array([rnd.randint(0, len(seqs[i])) for i in index], dtype=np.uint64)
        return index, (ends * np.array([rnd.random() for _ in range(n_out)])).astype(np.uint64), ends

    def spoil(t, j, why):
        index, starts, ends = t
        if why == 1:
            index[j] = 4 + j % 3 * 1000000
        elif why == 2:
            starts[j] = ends[j] + 1
        else:
            ends[j] = len(seqs[index[j]]) + 1 + (j // 70000 << 40)
    exc = IndexError if reason == 1 else ValueError
    try:
        for j in (2, 70000):
            t = tables()
            spoil(t, j, reason)
            with pytest.raises(exc, match="item %d:" % j) as e:
                engine.derive_batch(held.handle, *t)
            assert (e.value.info["bad_item"], e.value.info["bad_reason"]) == (j, reason)
            with pytest.raises(exc, match="item %d:" % j):                  # the public call says the same
                held.derive(*t, reverse=True, translate=fa.DNA_COMPLEMENT)
            for other in (1, 2, 3):                                         # a second bad item behind it
                t2 = tuple(c.copy() for c in t)
                spoil(t2, j + 1 + (other + 5 if j > 60000 else 300 * other), other)
                with pytest.raises(exc) as e:
                    engine.derive_batch(held.handle, *t2)
                assert (e.value.info["bad_item"], e.value.info["bad_reason"]) == (j, reason)
            good = tables()
            h = engine.derive_batch(held.handle, *good)                     # a good call afterwards
            assert h.n_seqs == n_out and engine.batch_bytes(h) == b"".join(derive_model.model(seqs, *good))
            h.release()
    finally:
        held.release()


def test_refusals(engine):
    rnd = random.Random(11)
    seqs = [dna(rnd, 60) for _ in range(4)]
    held = fa.resident_batch(seqs, engine=engine)
    plain = engine.upload(b"".join(seqs))
    try:
        with pytest.raises(TypeError, match="resident batch"):              # a plain resident sequence
            fa.derive_batch(fa.resident(b"".join(seqs)), ends=[3])
        with pytest.raises(ValueError, match="batch handle"):
            engine.derive_batch(plain)
        plain.n_seqs = 1                                                    # ... and what the library says to its handle
        with pytest.raises(ValueError, match="batch handle"):
            engine.derive_batch(plain)
        with pytest.raises(ValueError):                                     # without an index: one output per sequence
            engine.derive_batch(held.handle, None, None, np.zeros(3, dtype=np.uint64), n_out=3)
        engine.lev_ngrams_begin(plain, seqs[0][:20], 2)                     # a pipelined search outstanding: as the uploads
        try:
            with pytest.raises(ValueError, match="in flight"):
                engine.derive_batch(held.handle)
            with pytest.raises(ValueError, match="in flight"):
                engine.upload_batch(b"", np.zeros(1, dtype=np.uint64))
        finally:
            assert len(engine.lev_ngrams_end()) >= 1
        d = held.derive(ends=[10, 20, 30, 40])
        held.release()                                                      # the parent's device memory may go first
        assert engine.batch_bytes(d.handle) == b"".join(s[:n] for s, n in zip(seqs, (10, 20, 30, 40)))
        assert list(d.sequences) == [s[:n] for s, n in zip(seqs, (10, 20, 30, 40))]
        with pytest.raises(ValueError, match="released"):                   # a released parent
            held.derive()
        d2 = d.derive(reverse=True)
        assert list(d2.sequences) == [s[:n][::-1] for s, n in zip(seqs, (10, 20, 30, 40))]
        d.release()
        with pytest.raises(ValueError, match="released"):
            d.derive()
        d2.release()
    finally:
        plain.release()
        held.release()


# ---- the result is a batch

P, Q, LEAK = b"ACGTTGCAGGATCCATAGCT", b"TTGACCGTAAGCTAGGCATC", b"GGCCAATTCGCGATATGCAT"
SUBS = dict(max_insertions=0, max_deletions=0)


def trimmed_case():
    """Reads and a trim per read.  Every third read carries P on the first and Q on the last bytes of its cut (some with an
    edit); the others carry LEAK across the cut's start or end: half of it inside, the other half present in the parent."""
    rnd = random.Random(1818)
    reads, starts, ends = [], [], []
    for j in range(90):
        r = bytearray(bytes(rnd.choice(b"AC") for _ in range(rnd.randint(90, 200))))     # (no pattern occurs by chance)
        a = rnd.randint(10, 25)
        b = len(r) - rnd.randint(10, 25)
        if j % 3 == 0:
            p, q = bytearray(P), bytearray(Q)
            if j % 2:
                p[7], q[11] = ord("A") if p[7] != ord("A") else ord("C"), ord("G") if q[11] != ord("G") else ord("T")
            r[a:a + 20], r[b - 20:b] = p, q
        elif j % 3 == 1:
            r[a - 10:a + 10] = LEAK
        else:
            r[b - 10:b + 10] = LEAK
        reads.append(bytes(r)); starts.append(a); ends.append(b)
    return reads, starts, ends


def triples(per_pattern_or_sequence):
    return [[(m.start, m.end, m.dist, bytes(m.matched) if not isinstance(m.matched, str) else m.matched) for m in per]
            for per in per_pattern_or_sequence]


def same_best(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in a.__slots__)


def test_the_result_is_a_batch(engine):
    reads, starts, ends = trimmed_case()
    want = derive_model.model(reads, None, starts, ends)
    held = fa.resident_batch(reads, engine=engine)
    derived = held.derive(starts=starts, ends=ends)
    model = fa.resident_batch(want, engine=engine)
    try:
        assert engine.batch_bytes(derived.handle) == engine.batch_bytes(model.handle)
        for pat in (P, Q, LEAK):
            for kw in (dict(max_l_dist=0), dict(max_l_dist=2), dict(max_substitutions=2, **SUBS)):
                got = triples(fa.find_near_matches_batch(pat, derived, **kw))
                assert got == triples(fa.find_near_matches_batch(pat, model, **kw)), (pat, kw)
                if pat is LEAK:                                             # no byte outside the cut came along
                    assert got == [[] for _ in reads]
                    assert sum(1 for per in fa.find_near_matches_batch(pat, held, **kw) if per) == 60   # (the parent has it)
        lev = triples(fa.find_near_matches_batch(P, derived, max_l_dist=2))
        last = triples(fa.find_near_matches_batch(Q, derived, max_l_dist=2))
        for j in range(0, 90, 3):                                           # planted on the first and on the last bytes
            n = ends[j] - starts[j]
            if j % 2 == 0:
                assert (0, 20, 0, want[j][:20]) in lev[j] and (n - 20, n, 0, want[j][-20:]) in last[j]          # matched: the lazy view's
            else:
                assert [m[2] for m in lev[j]] == [1] == [m[2] for m in last[j]]
        multi = fa.find_near_matches_multi_batch([P, Q, LEAK], derived, max_l_dist=2)
        assert [triples(per) for per in multi] == [triples(per) for per in fa.find_near_matches_multi_batch([P, Q, LEAK], model, max_l_dist=2)]
        assert multi[2] == [[] for _ in reads] and sum(map(len, multi[0])) >= 30
        deg = [P[:12] + b"N" + P[13:], Q[:3] + b"R" + Q[4:], LEAK[:9] + b"NN" + LEAK[11:]]
        kw = dict(max_substitutions=2, classes=fa.IUPAC_DNA, **SUBS)
        best = fa.find_best_matches_batch(deg, derived, **kw)
        assert same_best(best, fa.find_best_matches_batch(deg, model, **kw))
        assert set(best.pattern[0::3].tolist()) == {0} and set(best.pattern[1::3].tolist()) == set(best.pattern[2::3].tolist()) == {-1}
        assert same_best(fa.find_best_matches_batch([P, Q], derived, max_l_dist=2), fa.find_best_matches_batch([P, Q], model, max_l_dist=2))
    finally:
        for h in (held, derived, model):
            h.release()


def _parents(engine, reads):
    yield "list", fa.resident_batch(reads, engine=engine)
    yield "records", fa.resident_records(rm.fastq(reads), engine=engine)
    yield "fasta", fa.resident_fasta(fm.fasta([r.lower() for r in reads], width=60), upper=True, engine=engine)
    first = fa.resident_batch([r + b"TT" for r in reads[::-1]], engine=engine)
    yield "derived", first.derive(index=list(range(len(reads)))[::-1], ends=[len(r) for r in reads])
    first.release()
    yield "str", fa.resident_batch([r.decode() for r in reads], engine=engine)


def test_every_parent_kind(engine):
    reads, starts, ends = trimmed_case()
    reads, starts, ends = reads[:30], starts[:30], ends[:30]
    index = [0, 29, 3, 3, 6, 1, 2, 0]
    a, b = [starts[i] for i in index], [ends[i] for i in index]
    for name, parent in _parents(engine, reads):
        try:
            src = list(parent.sequences)
            assert [s.encode() if name == "str" else bytes(s) for s in src] == reads
            for reverse, translate in FORMS:
                if translate and name == "str":
                    with pytest.raises(TypeError):
                        parent.derive(index, a, b, reverse, fa.DNA_COMPLEMENT)
                    continue
                table = fa.DNA_COMPLEMENT if translate else None
                d = parent.derive(index, a, b, reverse, table)
                want = derive_model.model(src, index, a, b, reverse, table)
                assert list(d.sequences) == want and d.kind == parent.kind and d.parent is parent
                packed = "".join(want).encode("latin-1") if name == "str" else b"".join(want)
                assert engine.batch_bytes(d.handle) == packed and d.lengths.tolist() == [len(w) for w in want]
                if not reverse and not translate:
                    pat = P.decode() if name == "str" else P
                    got = fa.find_near_matches_batch(pat, d, max_l_dist=2)
                    model = fa.resident_batch(want, engine=engine)
                    assert triples(got) == triples(fa.find_near_matches_batch(pat, model, max_l_dist=2))
                    assert [len(g) for g in got] == [1, 0, 1, 1, 1, 0, 0, 1] and got[0][0].matched == want[0][:20]
                    model.release()
                d.release()
        finally:
            parent.release()


def test_the_pipeline_trim_then_search(engine):
    """Find the adapter, cut it off where it was found, search what is left: the second search equals the model's."""
    rnd = random.Random(4)
    adapter, barcode = b"AGATCGGAAGAGCACACGTC", b"TTGGCCAATTGGCCAAGTCA"
    reads = []
    for j in range(120):
        body = bytearray(bytes(rnd.choice(b"AC") for _ in range(rnd.randint(60, 150))))
        if j % 4 != 3:
            body[5:25] = barcode
        if j % 5 == 4:
            body[8] = ord("G") if body[8] != ord("G") else ord("T")
        ad = bytearray(adapter)
        if j % 2:
            ad[j % 20] = ord("T") if ad[j % 20] != ord("T") else ord("A")
        reads.append(bytes(body) + (bytes(ad) + bytes(rnd.choice(b"AC") for _ in range(j % 30)) if j % 6 else b""))
    held = fa.resident_records(rm.fastq(reads), engine=engine)
    try:
        best = fa.find_best_matches_batch([adapter], held, max_l_dist=2)
        cut = np.where(best.pattern >= 0, best.start, held.lengths)                # the documented expression, as it is
        assert (best.pattern >= 0).sum() == 100
        trimmed = held.derive(ends=cut)
        want = derive_model.model(reads, None, None, cut)
        assert list(trimmed.sequences) == want and engine.batch_bytes(trimmed.handle) == b"".join(want)
        got = fa.find_near_matches_batch(barcode, trimmed, max_l_dist=1)
        assert triples(got) == triples(fa.find_near_matches_batch(barcode, want, max_l_dist=1))
        assert sum(map(len, got)) == 90 and all(adapter not in w for w in want)
        assert triples(fa.find_near_matches_batch(adapter, trimmed, max_l_dist=2)) == [[] for _ in reads]
        trimmed.release()
    finally:
        held.release()


def test_reverse_complement_finds_the_minus_strand(engine):
    rnd = random.Random(6)
    rc = lambda s: s.translate(fa.DNA_COMPLEMENT)[::-1]
    reads, where = [], []
    for j in range(40):
        r = bytearray(bytes(rnd.choice(b"AC") for _ in range(rnd.randint(40, 170))))
        s = (0, len(r) - 20, rnd.randint(0, len(r) - 20))[j % 3]
        r[s:s + 20] = rc(P)
        reads.append(bytes(r)); where.append(s)
    held = fa.resident_batch(reads, engine=engine)
    try:
        assert sum(map(len, fa.find_near_matches_batch(P, held, max_l_dist=1))) == 0
        minus = held.derive(reverse=True, translate=fa.DNA_COMPLEMENT)
        assert engine.batch_bytes(minus.handle) == b"".join(rc(r) for r in reads)
        got = triples(fa.find_near_matches_batch(P, minus, max_l_dist=1))
        assert got == [[(len(r) - s - 20, len(r) - s, 0, P)] for r, s in zip(reads, where)]         # the mirrored coordinates
        minus.release()
    finally:
        held.release()


def test_timing_spans(engine):
    seqs = seam_case(0)[0]
    held = fa.resident_batch(seqs, engine=engine)
    try:
        held.derive(index=[12] * 50, reverse=True, translate=fa.DNA_COMPLEMENT).release()
        ms = engine.derive_ms()
        assert sorted(ms) == ["call", "ends_d2h", "gather", "measure_scan", "tables_h2d"]
        assert all(np.isfinite(v) and v >= 0 for v in ms.values()) and ms["gather"] > 0 and ms["measure_scan"] > 0 and ms["call"] > 0, ms
    finally:
        held.release()
