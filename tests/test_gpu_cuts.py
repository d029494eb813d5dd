"""-m gpu: score cuts on the device (fz_batch_score_cuts / Engine.batch_score_cuts / find_score_cuts_batch, quality_cuts,
poly_tail_cuts) — both arrays against the model of the definition (tests/cuts_model.py), exactly, for every generated read."""
import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import cuts_case as cc
from tests import cuts_model as cm
from tests import fasta_model as fm
from tests import records_model as rm
from tests.test_cuts_host import assert_same

pytestmark = pytest.mark.gpu


def device(engine, w3, w5, reads, stop=True, rate=None, stop5=None):
    """Engine.batch_score_cuts over a fresh upload -> ((start, end), stats of the call)"""
    blob, _lens = cc.pack(reads)
    h = engine.upload_batch(blob, cc.offsets(reads))
    num, den = rate if rate is not None else (0, 1)
    try:
        rows = engine.batch_score_cuts(h, w3, w5, cc.flags_of(stop, stop if stop5 is None else stop5, rate), num, den)
        st = engine.stats()
    finally:
        h.release()
    assert rows.dtype == _native.cut_dtype() and len(rows) == len(reads)
    return cc.rows_arrays(rows), st


# ---- 1. the emulation's groups: every length 0 .. 2 pieces + 9 at every start alignment, each side and both, stop and rate
#         on and off, 0x00 / 0xff behind the data and around every read with the highest score

@pytest.fixture(scope="module")
def groups():
    gs = cc.groups(range(0, 2 * cc.PIECE + 10))
    return gs, [cm.score_cuts(reads, w3, w5, stop, stop, rate) for w3, w5, stop, rate, reads, _pad in gs]


def test_the_emulation_s_groups_on_the_device(engine, groups):
    gs, want = groups
    cut = 0
    for (w3, w5, stop, rate, reads, pad), (start, end) in zip(gs, want):
        got, st = device(engine, w3, w5, reads, stop, rate)
        assert_same(got, (start, end), "sides %d%d stop %s rate %s pad %#x" % (w3 is not None, w5 is not None, stop, rate, pad))
        assert st["filter_launches"] == 1
        cut += int(((start > 0) | (end < np.array([len(r) for r in reads]))).sum())
    assert cut >= 5000


# ---- 2. the twin's batches: adversarial neighbours at every read count, and one lane carried over many pieces

@pytest.mark.parametrize("n_seqs", [1, 63, 64, 65, 257])
def test_read_counts_with_adversarial_neighbours(engine, n_seqs):
    rng = cc.rng_of("twin", n_seqs)
    for top in (0x00, 0xff):
        alphabet = cc.ALPHABETS[2]
        w3, w5 = cc.rand_table(rng, alphabet, top=top), cc.rand_table(rng, alphabet, top=top)
        reads = cc.twin_batch(rng, n_seqs, w3, alphabet, top)
        for stop, rate in ((True, None), (False, None), (False, (1, 5))):
            for a, b in ((w3, None), (None, w5), (w3, w5)):
                got, _st = device(engine, a, b, reads, stop, rate)
                assert_same(got, cm.score_cuts(reads, a, b, stop, stop, rate), "%d reads, stop %s, rate %s" % (n_seqs, stop, rate))


def test_one_live_lane_over_many_pieces(engine):
    rng = cc.rng_of("long")
    alphabet, top = cc.ALPHABETS[2], 0xff
    w3, w5 = cc.rand_table(rng, alphabet, top=top), cc.rand_table(rng, alphabet, top=top)
    reads = cc.twin_batch(rng, 90, w3, alphabet, top, long_at=41)
    assert len(reads[41]) == 70000
    for stop, rate in ((True, None), (False, None), (False, (1, 5))):
        want = cm.score_cuts(reads, w3, w5, stop, stop, rate)
        got, _st = device(engine, w3, w5, reads, stop, rate)
        assert_same(got, want, "long read, stop %s, rate %s" % (stop, rate))
    got, _st = device(engine, w3, w5, reads, True, (1, 5), stop5=False)
    assert_same(got, cm.score_cuts(reads, w3, w5, True, False, (1, 5)), "stop on 3' only")
    want3 = cm.score_cuts(reads, w3, None, False, False, None)
    assert want3[1][41] < 70000 - 10 * cc.PIECE
    got, _st = device(engine, w3, None, reads, False, None)
    assert_same(got, want3, "long read, 3' alone")


# ---- 3. both sides in one call, reads where they cross; a table without a positive score launches nothing

def test_both_sides_cross(engine):
    rng = cc.rng_of("cross")
    q3, q5 = cm.quality_table(20), cm.quality_table(25)
    quals = []
    for j in range(700):
        n = rng.randrange(0, 160)
        low5, low3 = rng.randrange(0, n + 1), rng.randrange(0, n + 1)        # low ends that often overlap: the sides cross
        q = bytearray(33 + rng.randrange(28, 41) for _ in range(n))
        for i in range(low5):
            q[i] = 33 + rng.randrange(2, 24)
        for i in range(n - low3, n):
            q[i] = 33 + rng.randrange(2, 24)
        quals.append(bytes(q))
    want = cm.score_cuts(quals, q3, q5)
    got, st = device(engine, q3, q5, quals)
    assert_same(got, want, "both sides")
    lens = np.array([len(q) for q in quals])
    crossed = (lens > 0) & (want[0] == 0) & (want[1] == 0)
    assert crossed.sum() >= 50 and ((want[0] > 0) & (want[1] < lens)).sum() >= 100 and st["filter_launches"] == 1
    res = fa.quality_cuts(quals, 20, 25)
    assert_same((res.start, res.end), want, "quality_cuts over a list")


def test_a_table_without_a_positive_score_launches_nothing(engine):
    reads = [b"ACGT" * 10, b"", b"AC"] * 100
    lens = [40, 0, 2] * 100
    got, st = device(engine, [0] * 256, [-5] * 256, reads, False, None)
    assert (got[0].tolist(), got[1].tolist()) == ([0] * 300, lens) and st["filter_launches"] == 0
    got, st = device(engine, cm.poly_table(), None, reads, False, (1, 5))
    assert st["filter_launches"] == 1                           # (the same batch with a score above 0 is launched)
    got, st = device(engine, None, [0] * 256, reads)
    assert (got[0].tolist(), got[1].tolist()) == ([0] * 300, lens) and st["filter_launches"] == 0
    ms = engine.cuts_ms()
    assert set(ms) == {"tables_h2d", "kernels", "rows_d2h", "call"} and ms["call"] >= 0 and ms["kernels"] == 0


# ---- 4. handles

@pytest.fixture(scope="module")
def fastq_reads():
    rng = cc.rng_of("fastq")
    reads, quals = [], []
    for j in range(500):
        n = rng.randrange(0, 120)
        tail = rng.randrange(0, 30) if rng.random() < 0.5 else 0
        body = cc.rand_bytes(rng, max(n - tail, 0))
        reads.append(body + bytes(rng.choice(b"AAAAAAAAAC") for _ in range(min(tail, n))))
        low = rng.randrange(0, 40) if rng.random() < 0.7 else 0
        quals.append(bytes(33 + (rng.randrange(2, 22) if i >= n - low else rng.randrange(25, 41)) for i in range(n)))
    return reads, quals


def test_handles_answer_as_the_list_of_their_sequences(engine, fastq_reads):
    reads, quals = fastq_reads
    heads, bases, qual = fa.resident_records(rm.fastq(reads, quals=quals), engine=engine, lines=(0, 1, 3))
    contigs = [r for r in reads if r][:60]
    fasta = fa.resident_fasta(fm.fasta(contigs, width=50), engine=engine)
    try:
        q = fa.quality_cuts(qual, 20, 15)
        assert_same((q.start, q.end), cm.score_cuts(quals, cm.quality_table(20), cm.quality_table(15)), "records")
        tails = fa.poly_tail_cuts(bases)
        assert_same((tails.start, tails.end), cm.score_cuts(reads, cm.poly_table(), None, False, False, (1, 5)), "poly-A over records")
        assert (tails.end < bases.lengths.astype(np.int64)).sum() >= 100
        got = fasta.score_cuts({b"A": 1, "default": -2}, stop=False, max_miss_rate=(1, 5))
        assert_same((got.start, got.end), cm.score_cuts(contigs, cm.poly_table(), None, False, False, (1, 5)), "fasta")
        # the minus strand of the reads trimmed by 3 at both ends: its poly-T head is what poly-A was
        lens = bases.lengths.astype(np.int64)
        cut = bases.derive(starts=np.minimum(3, lens), ends=np.maximum(lens - 3, np.minimum(3, lens)), reverse=True, translate=fa.DNA_COMPLEMENT)
        seqs = [bytes(s) for s in cut.sequences]
        assert seqs == [r[3:max(len(r) - 3, min(3, len(r)))].translate(fa.DNA_COMPLEMENT)[::-1] for r in reads]
        table = {b"T": 1, "default": -2}
        got = fa.find_score_cuts_batch(cut, None, table, stop=False, max_miss_rate=(1, 5))
        assert_same((got.start, got.end), cm.score_cuts(seqs, None, cm.poly_table(b"T"), False, False, (1, 5)), "derived, reversed")
        assert (got.start > 0).sum() >= 100
        cut.release()
        assert [bytes(s) for s in qual.sequences] == quals
    finally:
        for h in (heads, bases, qual, fasta):
            h.release()


def test_handles_the_call_does_not_take(engine):
    plain = engine.upload(b"ACGT" * 100)
    try:
        plain.n_seqs = 0
        with pytest.raises(_native.UnsupportedSearch, match="takes a batch handle"):
            engine.batch_score_cuts(plain, cm.poly_table(), None, 0)
    finally:
        plain.release()
    blob, _lens = cc.pack([b"ACGTACGT", b"TT"])
    h = engine.upload_batch(blob, cc.offsets([b"ACGTACGT", b"TT"]))
    try:
        with pytest.raises(ValueError, match="both null"):
            engine.batch_score_cuts(h, None, None, 0)
        with pytest.raises(ValueError, match="rate_den must not be 0"):
            engine.batch_score_cuts(h, cm.poly_table(), None, cc.RATE, 1, 0)
        rows = engine.batch_score_cuts(h, None, cm.poly_table(b"T"), 0)
        assert (rows["start"].tolist(), rows["end"].tolist()) == ([0, 2], [8, 2])
    finally:
        h.release()


# ---- 5. the pipeline: quality cut, adapter cut, derive of bases and qualities, the FASTQ text

def test_pipeline_equals_the_python_loop_over_the_model(engine, fastq_reads):
    reads, quals = fastq_reads
    rng = cc.rng_of("pipeline")
    adapter = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    reads = [r[:len(r) - k] + adapter[:k] if len(r) >= k else r for r, k in ((r, rng.randrange(0, 20)) for r in reads)]
    head_lines = [b"@r%d" % j for j in range(len(reads))]
    heads, bases, qual = fa.resident_records(rm.fastq(reads, quals=quals), engine=engine, lines=(0, 1, 3))
    try:
        q = fa.quality_cuts(qual, 20)
        ov = fa.find_end_overlaps_batch(adapter, bases, max_l_dist=0, min_overlap=3)
        ends = np.minimum(ov.start, q.end)
        out_bases, out_qual = bases.derive(ends=ends), qual.derive(ends=ends)
        text = fa.format_records([heads, out_bases, out_qual], "fastq").tobytes()
        out_bases.release()
        out_qual.release()
    finally:
        for h in (heads, bases, qual):
            h.release()
    w = cm.quality_table(20)
    want, shorter = [], 0
    for head, r, ql in zip(head_lines, reads, quals):
        cut = len(r)
        for i in range(len(adapter) - 1, 2, -1):                # the longest exact prefix of 3 .. 32 bytes that ends the read
            if len(r) >= i and r.endswith(adapter[:i]):
                cut = len(r) - i
                break
        cut = min(cut, cm.cut3(ql, w, True))
        shorter += cut < len(r)
        want += [head, r[:cut], b"+", ql[:cut]]
    assert text == b"".join(l + b"\n" for l in want) and shorter >= 250
