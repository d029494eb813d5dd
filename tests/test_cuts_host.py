"""find_score_cuts_batch, host side (CPU only): the model (tests/cuts_model.py) against a brute force over prefix sums; the
kernel's per-lane functions compiled with g++ (tests/cuts_emul.cpp, a stand-alone program; once more under the host
sanitizers) against the model, and their bounded exit against the same functions with the bound disabled; the host twin of
the call (fz_debug_score_cuts) on packed batches with adversarial neighbours; and every refusal of the C-ABI and of the
public call over a stub engine."""
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, cuts
from tests import cuts_case as cc
from tests import cuts_model as cm

HERE = os.path.dirname(os.path.abspath(__file__))


def assert_same(got, want, what=""):
    for name, g, w in zip(("start", "end"), got, want):
        bad = np.flatnonzero(np.asarray(g) != np.asarray(w))
        assert bad.size == 0, "%s %s: read %d is %s, the model says %s" % (what, name, bad[0], g[bad[0]], w[bad[0]])


# ---- 1. the model is the definition

def test_model_equals_the_brute_force_over_prefix_sums():
    rng = cc.rng_of("model")
    edge = {"n0": 0, "cut at 0": 0, "cut at n": 0, "equal peaks": 0, "zero scores": 0, "wmax<=0": 0, "rate refuses the higher peak": 0,
            "start>=end": 0}
    cases = 0
    for t in range(1500):
        alphabet = cc.ALPHABETS[t % 3]
        w = cc.rand_table(rng, alphabet, top=rng.choice(alphabet) if t % 4 else None, hi=3 if t % 11 else 0)
        n = 0 if t % 50 == 0 else rng.randrange(0, 40)
        r = cc.ended_read(rng, n, w, alphabet)
        stop = bool(t % 2)
        rate = None if t % 3 == 0 else (rng.randrange(0, 4), rng.randrange(1, 8))
        got = cm.cut3(r, w, stop, rate)
        assert got == cm.brute_cut3(r, w, stop, rate), (r, w, stop, rate)
        assert 0 <= got <= n
        got5 = cm.cut5(r, w, stop, rate)
        assert got5 == n - cm.brute_cut3(r[::-1], w, stop, rate) and 0 <= got5 <= n
        cases += 1
        sums = np.cumsum(np.asarray(w)[np.frombuffer(r[::-1], dtype=np.uint8)]) if n else np.zeros(0, dtype=np.int64)
        edge["n0"] += n == 0
        edge["cut at 0"] += n > 0 and got == 0
        edge["cut at n"] += n > 0 and got == n
        edge["equal peaks"] += n > 0 and got < n and int((sums == sums[n - 1 - got]).sum()) > 1 and not stop and rate is None
        edge["zero scores"] += any(w[c] == 0 for c in r)
        edge["wmax<=0"] += max(w) <= 0 and n > 0
        edge["rate refuses the higher peak"] += rate is not None and not stop and cm.cut3(r, w, stop, None) < n and \
            got != cm.cut3(r, w, stop, None)
        start, end = cm.cuts_one(r, w, w, stop, stop, rate)
        in_force = None if stop else rate                    # the rate applies to the sides that do not stop
        one3, one5 = cm.cut3(r, w, stop, in_force), cm.cut5(r, w, stop, in_force)
        if one5 >= one3:
            edge["start>=end"] += 1
            assert (start, end) == (0, 0)
        else:
            assert (start, end) == (one5, one3)
        assert cm.cuts_one(r, w, None, stop, stop, rate) == (0, one3)
        assert cm.cuts_one(r, None, w, stop, stop, rate) == (one5, n)
    assert cases >= 1000 and all(edge.values()), (cases, edge)
    assert cm.cuts_one(b"", [1] * 256, [1] * 256) == (0, 0)
    # the rule stated once on a read one can check by eye: quality trimming at cutoff 20 (base 33: '5' = 20, 'I' = 40, '#' = 2)
    w = cm.quality_table(20)
    assert cm.cut3(b"IIIII##5#", w, True) == 5 and cm.cut3(b"IIIII", w, True) == 5 and cm.cut3(b"#####", w, True) == 0
    assert cm.cut3(b"IIIII##I#", w, True) == 8               # the sum falls below 0 at the 'I': the walk stops there
    assert cm.cut3(b"II5", w, True) == 3                     # a zero score is no peak above 0
    assert cm.cut5(b"##5#III", w, True) == 4
    w = cm.poly_table()
    assert cm.cut3(b"CGTCAAAAAA", w, False, (1, 5)) == 4 and cm.cut3(b"CGTCAAAGAAAAAA", w, False, (1, 5)) == 4
    assert cm.cut3(b"AAAAGA", w, False, None) == 0 and cm.cut3(b"AAAAGA", w, False, (0, 1)) == 5     # no miss allowed: the higher peaks are refused


# ---- 2. the kernel's per-lane functions, compiled for the host

@pytest.fixture(scope="module")
def emul_cases():
    groups = cc.groups(range(0, 2 * cc.PIECE + 10))
    want = [cm.score_cuts(reads, w3, w5, stop, stop, rate) for w3, w5, stop, rate, reads, _pad in groups]
    return groups, want


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_lane_functions_equal_the_model_over_the_dword_staged_pieces(flags, emul_cases):
    groups, want = emul_cases
    assert sum(len(g[4]) for g in groups) >= 20000
    stem = os.path.join(tempfile.gettempdir(), "fz_cuts_emul_%d_%d" % (os.getpid(), len(flags)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + [os.path.join(HERE, "cuts_emul.cpp"), "-o", stem])
    try:
        with open(stem + ".cases", "wb") as f:
            for w3, w5, stop, rate, reads, pad in groups:
                f.write(cc.emul_group(w3, w5, cc.flags_of(stop, stop, rate), rate, reads, pad))
        out = subprocess.run([stem, stem + ".cases"], capture_output=True, text=True, timeout=300)
    finally:
        for path in (stem, stem + ".cases"):
            if os.path.exists(path):
                os.unlink(path)
    assert out.returncode == 0, out.stderr
    rows = np.array(out.stdout.split(), dtype=np.int64).reshape(-1, 4)
    at = cut = crossed = 0
    seen = set()
    for (w3, w5, stop, rate, reads, pad), (start, end) in zip(groups, want):
        got = rows[at:at + len(reads)]
        at += len(reads)
        lens = np.array([len(r) for r in reads])
        what = "sides %d%d stop %s rate %s pad %#x" % (w3 is not None, w5 is not None, stop, rate, pad)
        assert_same((got[:, 0], got[:, 1]), (start, end), what)
        assert_same((got[:, 2], got[:, 3]), (start, end), what + ", unbounded")
        moved = (start > 0) | (end < lens)
        cut += int(moved.sum())
        crossed += int(((lens > 0) & (start == 0) & (end == 0) & (w3 is not None and w5 is not None)).sum())
        first = np.concatenate([[0], np.cumsum(lens)[:-1]])
        seen |= set(zip((first[moved] % 4).tolist(), (np.minimum(lens[moved], 2 * cc.PIECE + 1) // cc.PIECE).tolist()))
    assert at == len(rows) and cut >= 5000 and crossed >= 50, (at, cut, crossed)
    assert seen == {(a, p) for a in range(4) for p in range(3)}, seen     # cuts at every start alignment, in reads of 1, 2 and 3 pieces


# ---- 3. the host twin of the call

def twin(w3, w5, reads, stop=True, rate=None, stop5=None):
    blob, _lens = cc.pack(reads)
    num, den = rate if rate is not None else (0, 1)
    flags = cc.flags_of(stop, stop if stop5 is None else stop5, rate)
    return cc.rows_arrays(_native.score_cuts_twin(w3, w5, flags, num, den, blob, cc.offsets(reads)))


@pytest.mark.parametrize("n_seqs", [1, 63, 64, 65, 257])
def test_twin_keeps_every_read_to_its_own_bytes(n_seqs):
    rng = cc.rng_of("twin", n_seqs)
    for top in (0x00, 0xff):
        alphabet = cc.ALPHABETS[2]
        w3, w5 = cc.rand_table(rng, alphabet, top=top), cc.rand_table(rng, alphabet, top=top)
        reads = cc.twin_batch(rng, n_seqs, w3, alphabet, top)
        for stop, rate in ((True, None), (False, None), (False, (1, 5))):
            for a, b in ((w3, None), (None, w5), (w3, w5)):
                assert_same(twin(a, b, reads, stop, rate), cm.score_cuts(reads, a, b, stop, stop, rate), "%d reads, stop %s, rate %s" % (n_seqs, stop, rate))
    # what the layout is about, stated once: reads whose neighbours are nothing but the highest score keep to themselves
    w = cm.poly_table()
    reads = [b"AAAA", b"CCCC", b"AAAA", b"", b"CA", b"AAAA"]
    start, end = twin(w, w, reads, False, None)
    assert (start.tolist(), end.tolist()) == ([0, 0, 0, 0, 0, 0], [0, 4, 0, 0, 1, 0])


def test_twin_carries_one_live_lane_over_many_pieces():
    rng = cc.rng_of("long")
    alphabet, top = cc.ALPHABETS[2], 0xff
    w3, w5 = cc.rand_table(rng, alphabet, top=top), cc.rand_table(rng, alphabet, top=top)
    reads = cc.twin_batch(rng, 90, w3, alphabet, top, long_at=41)
    assert len(reads[41]) == 70000 and max(len(r) for r in reads[:41] + reads[42:]) <= 20
    for stop, rate in ((True, None), (False, None), (False, (1, 5))):
        want = cm.score_cuts(reads, w3, w5, stop, stop, rate)
        assert_same(twin(w3, w5, reads, stop, rate), want, "long read, stop %s, rate %s" % (stop, rate))
        want3 = cm.score_cuts(reads, w3, None, stop, stop, rate)
        assert_same(twin(w3, None, reads, stop, rate), want3, "long read, 3' alone")
        assert want3[1][41] < 70000 - 10 * cc.PIECE           # the cut lies many pieces into the read
    # the two sides stop independently
    assert_same(twin(w3, w5, reads, True, (1, 5), stop5=False), cm.score_cuts(reads, w3, w5, True, False, (1, 5)), "stop on 3' only")


def test_twin_answers_without_a_positive_score_and_for_no_reads():
    reads = [b"ACGT", b"", b"AC"]
    assert [x.tolist() for x in twin([0] * 256, None, reads)] == [[0, 0, 0], [4, 0, 2]]
    assert [x.tolist() for x in twin(None, [-1] * 256, reads, False)] == [[0, 0, 0], [4, 0, 2]]
    # a side without a positive score cuts nothing, the other side still cuts: both asked for, so a read cut whole is (0, 0)
    got = twin([0] * 256, cm.poly_table(), [b"AAAA", b"AACC", b""], False)
    assert [x.tolist() for x in got] == [[0, 2, 0], [0, 4, 0]]
    assert all(len(x) == 0 for x in twin([1] * 256, None, []))


def test_the_32_bit_sums_are_refused_at_the_boundary():
    long_read = bytes(65537)
    for score in (32767, -32767):                            # 65537 * 32767 = 2 147 450 879 < 2^31: inside
        w = [0] * 256
        w[0] = score
        start, end = twin(w, None, [b"\x00", long_read, b""], False)
        assert (start.tolist(), end.tolist()) == ([0, 0, 0], [0, 0, 0] if score > 0 else [1, 65537, 0])
    w = [0] * 256
    w[7] = -32768                                            # 65537 * 32768 >= 2^31
    with pytest.raises(_native.UnsupportedSearch, match=r"longest sequence \(65537 bytes\) times the largest \|score\| \(32768\) is not below 2\^31"):
        twin(w, None, [b"\x00", long_read, b""], False)
    with pytest.raises(_native.UnsupportedSearch, match=r"\(65536 bytes\) times the largest \|score\| \(32768\)"):
        twin(None, w, [bytes(65536)], False)                 # = 2^31 exactly
    w[7], w[0] = 0, 1
    assert twin(None, w, [bytes(65535)], False)[0].tolist() == [65535]
    w[9] = -32768                                            # 65535 * 32768 = 2^31 - 32768
    assert twin(None, w, [bytes(65535)], False)[0].tolist() == [65535]


# ---- 4. refusals: the C-ABI's (through the twin, which runs the call's checks), then the public call's over a stub engine

def test_c_abi_refusals_by_code_and_text():
    reads, w = [b"ACGTACGT"], cm.poly_table()
    blob, offs = b"ACGTACGT", cc.offsets(reads)
    for exc, text, args in (
            (ValueError, "w3 and w5 are both null", (None, None, 0, 0, 1)),
            (ValueError, "rate_den must not be 0", (w, None, cc.RATE, 1, 0)),
            (ValueError, "flags 0x8 outside", (w, None, 8, 0, 1))):
        with pytest.raises(exc, match=text):
            _native.score_cuts_twin(*(args + (blob, offs)))
    assert _native.score_cuts_twin(w, None, 0, 1, 0, blob, offs)["end"].tolist() == [8]      # (a zero denominator without the flag is not looked at)
    lib = _native.load_library()
    out = _native.ctypes.c_void_p()
    tab = np.array(w, dtype=np.int16)
    assert lib.fz_batch_score_cuts(None, None, tab.ctypes.data, None, 0, 0, 1, _native.ctypes.byref(out)) == _native.FZ_EINVAL
    assert lib.fz_last_error() == b"bad ctx/seq handle" and out.value is None
    assert lib.fz_debug_cuts_ms(None, None) == _native.FZ_EINVAL
    with pytest.raises(ValueError, match="offsets must not decrease"):
        _native.score_cuts_twin(w, None, 0, 0, 1, b"ACGT", np.array([0, 4, 2], dtype=np.uint64))
    with pytest.raises(ValueError, match="256 entries"):
        _native.score_cuts_twin([1] * 255, None, 0, 0, 1, blob, offs)
    assert _native.cut_dtype().itemsize == 8 and _native.cut_dtype().names == ("start", "end")


class _StubHandle(object):
    n_seqs = 0

    def release(self):
        pass


class _StubEngine(object):
    """Logs what reaches it; a call that gets as far as the device answers rows that cut nothing."""

    def __init__(self, log, devices=(0,), comm=(0, -1, False)):
        self.log, self.devices, self.comm = log, list(devices), comm

    def comm_info(self):
        return self.comm

    def upload_batch(self, blob, offs):
        self.log.append(("upload", len(offs) - 1))
        h = _StubHandle()
        h.n_seqs, h.lengths = len(offs) - 1, np.diff(offs.astype(np.int64))
        return h

    def batch_score_cuts(self, batch, w3, w5, flags, rate_num=0, rate_den=1):
        self.log.append(("cuts", None if w3 is None else w3.tolist(), None if w5 is None else w5.tolist(), flags, rate_num, rate_den))
        rows = np.zeros(batch.n_seqs, dtype=_native.cut_dtype())
        rows["end"] = batch.lengths
        return rows


def test_public_call_refuses_before_anything_is_uploaded(monkeypatch):
    log = []
    monkeypatch.setattr(_native, "default_engine", lambda: _StubEngine(log))
    call, seqs, U = fa.find_score_cuts_batch, [b"ACGTACGTAC", b"TTTT"], _native.UnsupportedSearch
    ok = {b"A": 1, "default": -2}
    for exc, text, args, kw in (
            (ValueError, "no table given", (seqs,), {}),
            (ValueError, "256 entries, not 255", (seqs, [1] * 255), {}),
            (ValueError, "score of byte 65 is outside the int16 range: 32768", (seqs, {65: 32768}), {}),
            (ValueError, "score of byte 3 is outside the int16 range: -32769", (seqs, None, [0, 0, 0, -32769] + [0] * 252), {}),
            (TypeError, "score of byte 65 is not an integer", (seqs, {b"A": 1.5}), {}),
            (ValueError, "keyed by byte values", (seqs, {b"AC": 1}), {}),
            (ValueError, "keyed by byte values", (seqs, {256: 1}), {}),
            (TypeError, "pair of integers or a fractions.Fraction", (seqs, ok), dict(stop=False, max_miss_rate=(0.2, 1))),
            (ValueError, "num >= 0 and den > 0", (seqs, ok), dict(stop=False, max_miss_rate=(1, 0))),
            (ValueError, "below 2\\^32", (seqs, ok), dict(stop=False, max_miss_rate=(1, 1 << 32))),
            (U, "bytes-like sequences of one kind", (["ACGT", "TTTT"], ok), {}),
            (U, "bytes-like sequences of one kind", ([b"ACGT", "TTTT"], ok), {}),
            (U, "bytes-like sequences of one kind", ([[1, 2, 3]], ok), {})):
        with pytest.raises(exc, match=text):
            call(*args, **kw)
    with pytest.raises(ValueError, match="no cutoff given"):
        fa.quality_cuts(seqs, None)
    assert log == []
    for engine in (_StubEngine(log, devices=(0, 1)), _StubEngine(log, comm=(2, 0, True))):
        monkeypatch.setattr(_native, "default_engine", lambda engine=engine: engine)
        with pytest.raises(U, match="single-device, non-collective engines"):
            call(seqs, ok)
        held = fa.resident_batch(seqs, engine=engine)            # (such an engine keeps the list and uploads nothing)
        with pytest.raises(U, match="resident batch of bytes-like sequences"):
            call(held, ok)
        with pytest.raises(U, match="resident batch of bytes-like sequences"):
            held.score_cuts(ok)
    assert log == []
    text_batch = fa.resident_batch(["ACGT", "TTTT"], engine=_StubEngine(log))
    del log[:]
    with pytest.raises(U, match="resident batch of bytes-like sequences"):
        call(text_batch, ok)
    assert log == []


def test_public_call_reaches_the_engine_once_with_its_tables_and_flags(monkeypatch):
    log = []
    engine = _StubEngine(log)
    monkeypatch.setattr(_native, "default_engine", lambda: engine)
    seqs = [b"ACGTACGTAC", b"", b"TTTT"]
    res = fa.quality_cuts(seqs, 20)
    assert log == [("upload", 3), ("cuts", cm.quality_table(20), None, cc.STOP3 | cc.STOP5, 0, 1)]
    assert isinstance(res, fa.ScoreCuts) and len(res) == 3 and repr(res) == "ScoreCuts(3 sequences)"
    assert res.start.dtype == np.int64 and res.end.dtype == np.int64
    assert (res.start.tolist(), res.end.tolist()) == ([0, 0, 0], [10, 0, 4])
    del log[:]
    held = fa.resident_batch(seqs, engine=engine)
    fa.quality_cuts(held, 20, 15, base=64)
    fa.quality_cuts(held, None, 15)
    fa.poly_tail_cuts(held)
    fa.poly_tail_cuts(held, base=b"T", hit=2, miss=-3, max_miss_rate=Fraction(2, 10))
    held.score_cuts(scores_5p=bytes(range(100)) * 2 + bytes(56), stop=False)
    fa.find_score_cuts_batch(held, {0x41: 5}, stop=True, max_miss_rate=(1, 3))     # (with stop the rate is not in force)
    assert log == [("upload", 3),
                   ("cuts", cm.quality_table(20, 64), cm.quality_table(15, 64), cc.STOP3 | cc.STOP5, 0, 1),
                   ("cuts", None, cm.quality_table(15), cc.STOP3 | cc.STOP5, 0, 1),
                   ("cuts", cm.poly_table(), None, cc.RATE, 1, 5),
                   ("cuts", cm.poly_table(b"T", 2, -3), None, cc.RATE, 1, 5),
                   ("cuts", None, list(range(100)) * 2 + [0] * 56, 0, 0, 1),
                   ("cuts", [0] * 65 + [5] + [0] * 190, None, cc.STOP3 | cc.STOP5, 1, 3)]
    del log[:]
    assert len(fa.find_score_cuts_batch([], {b"A": 1})) == 0 and log == []
    rows = np.zeros(2, dtype=_native.cut_dtype())
    rows["start"], rows["end"] = [0, 4], [7, 4000000000]
    res = cuts._from_rows(rows)
    assert (res.start.tolist(), res.end.tolist()) == ([0, 4], [7, 4000000000])
