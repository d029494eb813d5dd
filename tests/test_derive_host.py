"""derive_batch, host side (CPU only): the measure step and scan of fz_batch_derive run on the host through the function the
kernel runs (fz_debug_derive_plan) against the three-line model (tests/derive_model.py), the gather's address rule compiled
with g++ (tests/derive_emul.cpp, a stand-alone program), and the Python layer over a stub engine."""
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, batch, derive, fasta, records
from tests import derive_model

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the plan: fz_derive_item + the scan

def _plan_equals_model(seqs, index, starts, ends):
    n_out = len(seqs) if index is None else len(index)
    offs = derive_model.offsets(seqs)
    src, at, info = _native.derive_plan(offs, index, starts, ends, n_out)
    want = derive_model.model(seqs, index, starts, ends)
    blob = b"".join(seqs)
    assert [blob[int(s):int(s) + int(e - a)] for s, a, e in zip(src, at[:-1], at[1:])] == want
    assert at[0] == 0 and list(np.diff(at)) == [len(w) for w in want]
    assert info["n_out"] == n_out and info["packed_bytes"] == sum(map(len, want)) == at[-1]
    assert info["longest"] == max([len(w) for w in want] or [0]) and info["bad_reason"] == 0


def _random_case(rnd, n_src, n_out):
    seqs = [bytes(rnd.choice(b"ACGT") for _ in range(rnd.choice((0, 1, 5, 16, 33)))) for _ in range(n_src)]
    index = [rnd.randrange(n_src) for _ in range(n_out)]
    ends = [rnd.randint(0, len(seqs[i])) for i in index]
    starts = [rnd.randint(0, e) for e in ends]
    return seqs, index, starts, ends


def test_plan_equals_the_model_with_every_default_and_with_repeats():
    rnd = random.Random(1801)
    for n_src, n_out in ((1, 1), (7, 7), (7, 40), (30, 5), (9, 0)):
        seqs, index, starts, ends = _random_case(rnd, n_src, n_out)
        for use_s in (False, True):
            for use_e in (False, True):
                _plan_equals_model(seqs, index, starts if use_s else None, ends if use_e else None)
        assert n_out != 40 or len(set(index)) < len(index)                   # repeats: the result is larger than the parent
        e2 = [rnd.randint(0, len(s)) for s in seqs]                          # without an index: one output per sequence
        s2 = [rnd.randint(0, e) for e in e2]
        for s, e in ((None, None), (s2, None), (None, e2), (s2, e2)):
            _plan_equals_model(seqs, None, s, e)


def test_plan_starts_without_ends_reach_the_sequence_end():
    seqs = [b"ACGTACGT", b"", b"TT"]
    _plan_equals_model(seqs, [0, 2, 0, 1], [3, 2, 8, 0], None)
    _plan_equals_model(seqs, [0, 0, 0], [0, 0, 0], [8, 0, 3])


def test_plan_over_an_empty_parent():
    src, at, info = _native.derive_plan([0], None, None, None, 0)
    assert len(src) == 0 and list(at) == [0] and info["n_out"] == 0 and info["packed_bytes"] == 0
    src, at, info = _native.derive_plan([0], [], [], [], 0)
    assert list(at) == [0]
    with pytest.raises(IndexError, match="item 0") as e:
        _native.derive_plan([0], [0, 0], None, None, 2)
    assert e.value.info["bad_item"] == 0 and e.value.info["bad_reason"] == 1
    with pytest.raises(ValueError):                                          # no index: one output per sequence
        _native.derive_plan([0, 4], None, None, None, 2)


@pytest.mark.parametrize("reason", [1, 2, 3])
def test_plan_reports_every_reason_and_the_lower_of_two_bad_items(reason):
    seqs = [b"ACGTACGTAC", b"GG", b"", b"TTTTT"]
    offs = derive_model.offsets(seqs)
    n_out = 300
    rnd = random.Random(reason)

    def tables():
        index = [rnd.randrange(4) for _ in range(n_out)]
        ends = [rnd.randint(0, len(seqs[i])) for i in index]
        return index, [rnd.randint(0, e) for e in ends], ends

    def spoil(t, j, why):
        index, starts, ends = t
        if why == 1:
            index[j] = 4
        elif why == 2:
            starts[j], ends[j] = ends[j] + 1, ends[j]
        else:
            ends[j] = len(seqs[index[j]]) + 1
    exc = IndexError if reason == 1 else ValueError
    for j in (0, 2, 299):
        t = tables()
        spoil(t, j, reason)
        assert derive_model.first_bad(seqs, *t) == (j, reason)
        with pytest.raises(exc, match="item %d:" % j) as e:
            _native.derive_plan(offs, t[0], t[1], t[2], n_out)
        assert (e.value.info["bad_item"], e.value.info["bad_reason"]) == (j, reason)
        for other in (1, 2, 3):                                              # a second bad item behind it changes nothing
            t2 = ([*t[0]], [*t[1]], [*t[2]])
            if j < 299:
                spoil(t2, j + 1 + rnd.randrange(299 - j), other)
            assert derive_model.first_bad(seqs, *t2) == (j, reason)
            with pytest.raises(exc) as e:
                _native.derive_plan(offs, t2[0], t2[1], t2[2], n_out)
            assert (e.value.info["bad_item"], e.value.info["bad_reason"]) == (j, reason)
    # start > end wins over end > length in one item (the rule's order), and the next call works
    with pytest.raises(ValueError) as e:
        _native.derive_plan(offs, [1], [50], [40], 1)
    assert e.value.info["bad_reason"] == 2
    _plan_equals_model(seqs, [3, 3], [1, 0], [5, 0])


# ---- the gather's address rule

def test_gather_address_rule_at_every_alignment_and_length():
    exe = os.path.join(tempfile.gettempdir(), "fz_derive_emul_%d" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", os.path.join(HERE, "derive_emul.cpp"), "-o", exe])
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    finally:
        os.unlink(exe)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", str(16 * 16 * 49 * 2 * 2)]


# ---- the Python layer over a stub engine

class _StubHandle(object):
    _h = 1

    def __init__(self, n_seqs):
        self.n_seqs = n_seqs

    def release(self):
        self._h = None


class _StubEngine(object):
    """Logs what reaches the engine; a derived handle knows its number of sequences and nothing else."""
    devices = [0]

    def __init__(self, log):
        self.log = log

    def comm_info(self):
        return 0, -1, False

    def upload_batch(self, blob, offs):
        self.log.append(("upload", len(offs) - 1))
        return _StubHandle(len(offs) - 1)

    def derive_batch(self, handle, index, starts, ends, n_out, reverse, translate):
        self.log.append(("derive", handle, index, starts, ends, n_out, reverse, translate))
        return _StubHandle(n_out)


SEQS = [b"ACGTACGTAC", b"", b"GGA", b"TTTTTTTTTTTTTTTTTTTTT", b"C"]


def _held(log, seqs=SEQS):
    held = batch.BatchSequences(seqs, engine=_StubEngine(log))
    del log[:]
    return held


def test_mask_becomes_an_index_and_none_stays_none():
    log = []
    held = _held(log)
    d = held.derive(index=[True, False, True, True, False])
    assert isinstance(d, fa.DerivedBatch) and isinstance(d, batch.BatchSequences) and len(d) == 3
    (what, handle, index, starts, ends, n_out, reverse, translate), = log
    assert what == "derive" and handle is held.handle and index.dtype == np.uint32 and list(index) == [0, 2, 3]
    assert starts is None and ends is None and n_out == 3 and reverse is False and translate is None
    assert list(d.index) == [0, 2, 3] and list(d.starts) == [0, 0, 0] and d.parent is held and d.kind == "bytes"
    del log[:]
    d = fa.derive_batch(held, index=np.array([4, 4, 0], dtype=np.int64), starts=[0, 1, 2], ends=(1, 1, 9), reverse=1, translate=fa.DNA_COMPLEMENT)
    (_w, _h, index, starts, ends, n_out, reverse, translate), = log
    assert list(index) == [4, 4, 0] and starts.dtype == ends.dtype == np.uint64 and list(starts) == [0, 1, 2] and list(ends) == [1, 1, 9]
    assert n_out == 3 and reverse is True and translate == fa.DNA_COMPLEMENT
    del log[:]
    d = held.derive()
    assert log[0][2:6] == (None, None, None, 5) and list(d.index) == [0, 1, 2, 3, 4] and len(d) == 5
    d = held.derive(index=[])                                                # an empty selection is a batch
    assert len(d) == 0 and log[-1][5] == 0 and list(d.sequences) == []
    big = held.derive(index=[1 << 40, 0])                                    # beyond the C-ABI's type: still a value beyond the parent
    assert list(big.index) == [0xffffffff, 0]


def test_the_documented_trim_expression_is_accepted():
    """where(best.pattern >= 0, best.start, reads.lengths): int64 with uint64 is float64 in numpy; whole numbers pass as integers."""
    from fuzzysearch_amd import assign
    log = []
    held = _held(log)
    best = assign.BestMatches(len(SEQS))
    best.pattern[0], best.start[0], best.pattern[3], best.start[3] = 0, 4, 1, 20
    lengths = np.array([len(s) for s in SEQS], dtype=np.uint64)             # RecordBatch.lengths, DerivedBatch.lengths
    assert best.start.dtype == np.int64
    cut = np.where(best.pattern >= 0, best.start, lengths)
    d = held.derive(ends=cut)
    (_w, _h, _i, _s, ends, n_out, _r, _t), = log
    assert ends.dtype == np.uint64 and list(ends) == [4, 0, 3, 20, 1] and n_out == 5
    assert list(d.sequences) == derive_model.model(SEQS, None, None, [4, 0, 3, 20, 1])


def test_every_refusal_comes_before_any_engine_call():
    log = []
    held = _held(log)
    for kw, exc in ((dict(index=[True, False]), ValueError), (dict(index=[0.5, 1.0]), TypeError), (dict(index=[-1]), ValueError),
                    (dict(index=[[0, 1]]), ValueError), (dict(index=["a"]), TypeError),
                    (dict(starts=[0, 0]), ValueError), (dict(ends=[1] * 6), ValueError), (dict(starts=[0, 0, -1, 0, 0]), ValueError),
                    (dict(ends=[1.5] * 5), TypeError), (dict(starts=[0.0, float('nan'), 0, 0, 0]), TypeError), (dict(ends=[2.0 ** 60] * 5), TypeError),
                    (dict(ends=[-1.0] * 5), ValueError), (dict(starts=[True] * 5), TypeError), (dict(index=[0, 1], ends=[1, 1, 1]), ValueError),
                    (dict(index=[True, False, True, True, False], starts=[0] * 5), ValueError),
                    (dict(translate=b"ACGT"), ValueError), (dict(translate="A" * 256), TypeError), (dict(translate=list(range(256))), TypeError)):
        with pytest.raises(exc):
            held.derive(**kw)
    with pytest.raises(TypeError, match="resident batch"):
        fa.derive_batch(SEQS)
    with pytest.raises(TypeError, match="resident batch"):
        fa.derive_batch(b"ACGTACGT", ends=[2])
    text = _held(log, ["ACGT", "TTGA"])
    assert text.kind == "str"
    with pytest.raises(TypeError, match="str"):
        text.derive(translate=fa.DNA_COMPLEMENT)
    assert log == []
    held.release()
    with pytest.raises(ValueError, match="released"):
        held.derive()
    assert log == []


def test_dna_complement():
    t = fa.DNA_COMPLEMENT
    assert isinstance(t, bytes) and len(t) == 256 and "DNA_COMPLEMENT" in fa.__all__
    assert all(t[t[c]] == c for c in range(256))                             # an involution
    pairs = {"A": "T", "C": "G", "R": "Y", "K": "M", "B": "V", "D": "H"}
    moved = {}
    for a, b in pairs.items():
        for x, y in ((a, b), (b, a), (a.lower(), b.lower()), (b.lower(), a.lower())):
            moved[ord(x)] = ord(y)
    assert all(t[c] == moved.get(c, c) for c in range(256))
    assert all(t[ord(c)] == ord(c) for c in "SWNswn-*.U")
    assert b"AACCGGTTRYKMBVDHSWNacgtn".translate(t)[::-1] == b"nacgtNWSDHBVKMRYAACCGGTT"


def _fastq(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def _record_parent(log):
    """A RecordBatch as resident_records leaves it, over the stub (the split comes from the host's own splitter)."""
    rb = records.RecordBatch.__new__(records.RecordBatch)
    rb.source, rb.format, rb.engine, rb.kind = _fastq(SEQS), "fastq", _StubEngine(log), "bytes"
    rb.starts, rb.lengths = records.split_records(rb.source, "fastq")
    rb.handle = _StubHandle(len(rb.starts))
    rb.sequences = records.RecordSequences(rb.source, rb.starts, rb.lengths)
    return rb


def _fasta_parent(log):
    """A FastaBatch as resident_fasta leaves it, over the stub: lazy Contig slices of a wrapped text."""
    text = b"".join(b">c%d x\n%s" % (i, b"".join(s[k:k + 7] + b"\n" for k in range(0, len(s), 7))) for i, s in enumerate(SEQS))
    fb = fasta.FastaBatch.__new__(fasta.FastaBatch)
    fb.source, fb.upper, fb.engine, fb.kind = text, False, _StubEngine(log), "bytes"
    fb._rows, _contigs = fasta.split_fasta(text)
    fb._sequences, fb._n, fb.handle = None, len(fb._rows), _StubHandle(len(fb._rows))
    assert [bytes(c) for c in fb.sequences[:]] == SEQS
    return fb


TABLES = dict(index=[3, 0, 0, 4, 1, 2, 3], starts=[2, 0, 4, 1, 0, 1, 0], ends=[21, 10, 4, 1, 0, 3, 16])


@pytest.mark.parametrize("parent", ["list", "records", "fasta", "str"])
def test_lazy_view_equals_the_model(parent):
    log = []
    held = {"list": _held, "records": _record_parent, "fasta": _fasta_parent,
            "str": lambda lg: _held(lg, [s.decode() for s in SEQS])}[parent](log)
    src = [s.decode() for s in SEQS] if parent == "str" else SEQS
    forms = [dict()] + ([] if parent == "str" else [dict(translate=fa.DNA_COMPLEMENT)])
    for form in forms:
        for reverse in (False, True):
            for tables in (dict(), TABLES, dict(index=TABLES["index"]), dict(ends=[len(s) // 2 for s in SEQS]),
                           dict(starts=[len(s) // 2 for s in SEQS]), dict(index=[True, True, False, False, True])):
                d = held.derive(reverse=reverse, **tables, **form)
                idx = tables.get("index")
                if idx is not None and isinstance(idx[0], bool):
                    idx = [i for i, m in enumerate(idx) if m]
                want = derive_model.model(src, idx, tables.get("starts"), tables.get("ends"), reverse, form.get("translate"))
                assert list(d.sequences) == want and d.sequences[:] == want and [d.sequences[j] for j in range(len(d))] == want
                assert len(d.sequences) == len(d) == len(want) and all(type(g) is type(w) for g, w in zip(d.sequences, want))
                if want:
                    assert d.sequences[-1] == want[-1] and d[0] == want[0]
                with pytest.raises(IndexError):
                    d.sequences[len(want)]
                # a derived batch of the derived batch: the view over the view
                e2 = [len(w) - len(w) // 3 for w in want]
                d2 = d.derive(index=list(range(len(want)))[::-1], ends=e2[::-1], reverse=True)
                assert list(d2.sequences) == derive_model.model(want, list(range(len(want)))[::-1], None, e2[::-1], True)
                assert log[-1][1] is d.handle and d2.parent is d
    # nothing is kept: releasing the parent's device memory leaves the view working
    d = held.derive(**TABLES)
    held.release()
    assert list(d.sequences) == derive_model.model(src, **TABLES)


def test_parent_without_a_handle_derives_in_plain_python():
    log = []
    mixed = [b"ACGTACGTAC", "text", b"", [1, 2, 3, 4]]
    held = batch.BatchSequences(mixed, engine=_StubEngine(log))
    assert held.handle is None and held.kind is None and log == []
    d = held.derive(index=[3, 0, 1, 2, 0], starts=[1, 2, 0, 0, 10], ends=[3, 10, 4, 0, 10], reverse=True)
    assert d.handle is None and d.kind is None and log == []
    assert d.sequences == [[3, 2], b"CATGCATG", "txet", b"", b""] == derive_model.model([mixed[0], "text", b"", [1, 2, 3, 4]], [3, 0, 1, 2, 0], [1, 2, 0, 0, 10], [3, 10, 4, 0, 10], True)
    assert list(d.lengths) == [2, 8, 4, 0, 0]
    only_bytes = batch.BatchSequences.__new__(batch.BatchSequences)         # an engine the batched call does not serve
    only_bytes.sequences, only_bytes.engine, only_bytes.handle, only_bytes.kind = list(SEQS), _StubEngine(log), None, None
    d = only_bytes.derive(reverse=True, translate=fa.DNA_COMPLEMENT, **TABLES)
    assert d.sequences == derive_model.model(SEQS, reverse=True, translate=fa.DNA_COMPLEMENT, **TABLES) and log == []
    # ... and the same exceptions, the smallest bad item named
    for kw, exc, j in ((dict(index=[0, 5, 9]), IndexError, 1), (dict(index=[0, 0], starts=[3, 4], ends=[3, 3]), ValueError, 1),
                       (dict(ends=[10, 0, 4, 0, 0]), ValueError, 2), (dict(index=[2, 7], ends=[4, 0]), ValueError, 0)):
        assert derive_model.first_bad(SEQS, kw.get("index"), kw.get("starts"), kw.get("ends"))[0] == j
        with pytest.raises(exc, match="item %d:" % j):
            only_bytes.derive(**kw)
    with pytest.raises(TypeError):
        held.derive(index=[1], translate=fa.DNA_COMPLEMENT)


def test_exports():
    names = {"fz_batch_derive", "fz_debug_derive_plan", "fz_debug_derive_ms"}
    assert names <= set(_native.EXPORTED_SYMBOLS)
    lib = _native.load_library()
    for name in names:
        assert getattr(lib, name) is not None
    assert {"derive_batch", "derive_ms"} <= set(dir(_native.Engine))
    assert {"derive_batch", "DerivedBatch", "DNA_COMPLEMENT"} <= set(fa.__all__)
    assert fa.derive_batch is derive.derive_batch and hasattr(batch.BatchSequences, "derive")
