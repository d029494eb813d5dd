"""find_end_overlaps_batch, host side (CPU only): the model (tests/overlap_model.py) against a brute force over every suffix;
the kernel's per-lane functions compiled with g++ (tests/overlap_emul.cpp, a stand-alone program; once more under the host
sanitizers) against the model; the host twin of the call (fz_debug_end_overlaps) on packed batches with adversarial
neighbours; and every refusal of the C-ABI and of the public call over a stub engine."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, overlap
from tests import overlap_case as oc
from tests import overlap_model as om

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {om.LEV: "lev", om.SUBS: "subs"}


def assert_same(got, want, what=""):
    for name, g, w in zip(("pattern", "overlap", "dist", "start"), got, want):
        bad = np.flatnonzero(np.asarray(g) != np.asarray(w))
        assert bad.size == 0, "%s %s: read %d is %s, the model says %s" % (what, name, bad[0], g[bad[0]], w[bad[0]])


# ---- 1. the model is the definition

def test_model_equals_the_brute_force_over_every_suffix():
    rng = oc.rng_of("model")
    cases = found = 0
    edge = {"n0": 0, "n<o": 0, "i>n": 0, "k0": 0, "o>=m": 0}
    for mode in (om.LEV, om.SUBS):
        for t in range(600):
            alphabet = oc.ALPHABETS[t % 3]
            m = rng.randrange(1, 13)
            k = rng.randrange(0, min(m, 5))
            o = rng.randrange(1, 6) if t % 10 else m + rng.randrange(0, 2)
            p = oc.rand_bytes(rng, m, alphabet)
            roll = t % 6
            if roll == 0:
                r = b""
            elif roll == 1:
                r = oc.rand_bytes(rng, rng.randrange(0, o), alphabet)
            elif roll == 2 and m > 1:
                i = rng.randrange(1, m)                      # a prefix with deletions in a read shorter than the prefix
                r = oc.edited(rng, p[:i], rng.randrange(0, 3), alphabet, "d")[-rng.randrange(1, i + 1):]
            elif roll == 3 and m > 1:
                i = rng.randrange(1, m)
                r = oc.planted_read(rng, p, i, rng.randrange(0, k * i // m + 2), rng.randrange(0, 12), alphabet)
            else:
                r = oc.rand_bytes(rng, rng.randrange(0, 20), alphabet)
            want, got = om.brute_one(mode, p, r, k, o), om.overlap_one(mode, p, r, k, o)
            assert got == want, (MODES[mode], p, r, k, o)
            cases += 1
            found += got is not None
            edge["n0"] += not r
            edge["n<o"] += len(r) < o
            edge["i>n"] += got is not None and got[0] > len(r)
            edge["k0"] += k == 0
            edge["o>=m"] += o >= m
    assert cases >= 1000 and found >= 200 and all(edge.values()), (cases, found, edge)


# ---- 2. the kernel's per-lane functions, compiled for the host

def emul_groups():
    """(mode, k, o, patterns, reads, pad byte) of the emulator run: patterns of 1, 2, 31, 32, 33, 63 and 64 bytes at every
    budget 0 .. 16 below their length, both modes, three alphabets (two of them with 0x00 and 0xff, which is also what lies
    behind the data), panels that take more than one launch, reads of every length from 0 on: every end alignment."""
    rng = oc.rng_of("emul")
    groups = []
    for m in (1, 2, 31, 32, 33, 63, 64):
        for k in range(0, min(16, m - 1) + 1):
            for mode in (om.LEV, om.SUBS):
                alphabet = oc.ALPHABETS[(m + k + mode) % 3]
                patterns = [oc.rand_bytes(rng, m, alphabet)]
                if k % 4 == 1:                               # a panel: other lengths ride along, one pattern twice
                    extra = 9 if mode == om.LEV else 66
                    patterns += [oc.rand_bytes(rng, rng.randrange(k + 1, 65), alphabet) for _ in range(extra)] + [patterns[0]]
                o = rng.choice((1, 2, 3, 5, m - 1 if m > 1 else 1, m))
                count = 130 if len(patterns) == 1 else 40
                reads = oc.mixed_reads(rng, patterns, k, count, alphabet)
                reads += [oc.rand_bytes(rng, n, alphabet) for n in range(0, 9)]
                groups.append((mode, k, o, patterns, reads, rng.choice((0x00, 0xff))))
    return groups


@pytest.fixture(scope="module")
def emul_cases():
    groups = emul_groups()
    want = [om.end_overlaps(mode, patterns, reads, k, o) for mode, k, o, patterns, reads, _pad in groups]
    return groups, want


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_lane_functions_equal_the_model_over_the_dword_staged_window(flags, emul_cases):
    groups, want = emul_cases
    assert sum(len(g[4]) for g in groups) >= 20000
    stem = os.path.join(tempfile.gettempdir(), "fz_overlap_emul_%d_%d" % (os.getpid(), len(flags)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + [os.path.join(HERE, "overlap_emul.cpp"), "-o", stem])
    try:
        with open(stem + ".cases", "wb") as f:
            for mode, k, o, patterns, reads, pad in groups:
                f.write(oc.emul_group(mode, k, o, patterns, reads, pad))
        out = subprocess.run([stem, stem + ".cases"], capture_output=True, text=True, timeout=300)
    finally:
        for path in (stem, stem + ".cases"):
            if os.path.exists(path):
                os.unlink(path)
    assert out.returncode == 0, out.stderr
    rows = np.array(out.stdout.split(), dtype=np.int64).reshape(-1, 4)
    at = found = 0
    ends_mod_4 = set()
    for (mode, k, o, patterns, reads, _pad), (pattern, overlap_, dist, start) in zip(groups, want):
        got = rows[at:at + len(reads)]
        at += len(reads)
        none = got[:, 0] == 0xffff
        what = "%s m=%d k=%d o=%d" % (MODES[mode], len(patterns[0]), k, o)
        assert_same((np.where(none, -1, got[:, 0]), got[:, 1], np.where(none, -1, got[:, 2]), got[:, 3]), (pattern, overlap_, dist, start), what)
        found += int((~none).sum())
        ends_mod_4 |= set(int(x) % 4 for x in np.cumsum([len(r) for r in reads])[~none])
    assert at == len(rows) and found >= 3000 and ends_mod_4 == {0, 1, 2, 3}, (at, found, ends_mod_4)


# ---- 3. the host twin of the call

def twin(mode, patterns, reads, k, o):
    blob, _lens = oc.pack(reads)
    return oc.rows_arrays(_native.end_overlaps_twin(mode, patterns, k, o, blob, oc.offsets(reads)))


@pytest.mark.parametrize("mode", sorted(MODES), ids=lambda m: MODES[m])
def test_twin_keeps_every_read_to_its_own_bytes(mode):
    rng = oc.rng_of("twin", mode)
    for o in (1, 2, 3, 4):
        for alphabet, filler in ((b"ACGT", b"T"), (bytes([0x00, 0xff]), b"\x00"), (bytes([0x00, 0xff]), b"\xff")):
            p = oc.rand_bytes(rng, 20, alphabet)
            reads = oc.adversarial_neighbours(p, o, filler)
            assert_same(twin(mode, [p], reads, 2, o), om.end_overlaps(mode, [p], reads, 2, o), "%s o=%d" % (MODES[mode], o))
    # what the layout is about, stated once: the read in front of an empty read keeps its prefix, the empty read has none
    p = b"ACGTTGCAAGCCTAGGATCC"
    reads = oc.adversarial_neighbours(p, 3)
    pattern, overlap_, dist, start = twin(mode, [p], reads, 2, 3)
    assert (pattern[2], overlap_[2], dist[2], start[2]) == (0, 11, 0, 7) and (pattern[3], start[3]) == (-1, 0)
    assert (pattern[0], overlap_[0]) == (0, 10) and pattern[1] == -1


@pytest.mark.parametrize("mode", sorted(MODES), ids=lambda m: MODES[m])
def test_twin_chooses_between_patterns_by_matched_then_distance_then_position(mode):
    reads = [oc.TIE_READ, b"GGGG" + oc.TIE_X[:7], b"", oc.TIE_Y[:12]]
    for patterns in ([oc.TIE_Y, oc.TIE_X], [oc.TIE_X, oc.TIE_Y], [oc.TIE_Y, oc.TIE_X, oc.TIE_X], [oc.TIE_X] * 3):
        assert_same(twin(mode, patterns, reads, 2, 3), om.end_overlaps(mode, patterns, reads, 2, 3), MODES[mode])
    # the tie itself, in Levenshtein mode: both reach 10 matched bytes, X without an edit
    assert om.overlap_one(om.LEV, oc.TIE_X, oc.TIE_READ, 2, 3)[:2] == (10, 0) and om.overlap_one(om.LEV, oc.TIE_Y, oc.TIE_READ, 2, 3)[:2] == (11, 1)
    pattern, _overlap, dist, _start = twin(om.LEV, [oc.TIE_Y, oc.TIE_X, oc.TIE_X], reads, 2, 3)
    assert (pattern[0], dist[0]) == (1, 0)                   # the smaller distance beats the lower position; the first of a duplicate answers
    rng = oc.rng_of("panel", mode)
    patterns = [oc.rand_bytes(rng, rng.randrange(4, 65)) for _ in range(70)]
    patterns[40] = patterns[3]
    reads = oc.mixed_reads(rng, patterns, 3, 300)
    assert_same(twin(mode, patterns, reads, 3, 2), om.end_overlaps(mode, patterns, reads, 3, 2), "panel")


def test_twin_answers_for_no_patterns_and_no_reads():
    got = twin(om.LEV, [], [b"ACGT", b"", b"AC"], 1, 3)
    assert [x.tolist() for x in got] == [[-1, -1, -1], [0, 0, 0], [-1, -1, -1], [4, 0, 2]]
    assert all(len(x) == 0 for x in twin(om.SUBS, [b"ACGT"], [], 1, 3))


# ---- 4. refusals: the C-ABI's (through the twin, which runs the call's checks), then the public call's over a stub engine

def test_c_abi_refusals_by_code_and_text():
    reads = [b"ACGTACGT"]
    for exc, text, args in (
            (_native.UnsupportedSearch, "mode must be Levenshtein or substitutions-only", (0, [b"ACGT"], 1, 3)),
            (ValueError, "min_overlap must be at least 1", (om.LEV, [b"ACGT"], 1, 0)),
            (_native.UnsupportedSearch, "budgets up to 16", (om.LEV, [b"A" * 40], 17, 3)),
            (ValueError, "pattern 1 is empty", (om.SUBS, [b"ACGT", b""], 1, 3)),
            (_native.UnsupportedSearch, "pattern 2 is longer than 64 bytes", (om.LEV, [b"ACGT", b"ACGT", b"A" * 65], 1, 3)),
            (_native.UnsupportedSearch, "pattern 1 is not longer than the budget 4", (om.LEV, [b"ACGTACGT", b"ACGT"], 4, 3)),
            (_native.UnsupportedSearch, "at most 65534 patterns", (om.SUBS, [b"ACGT"] * 65535, 1, 3))):
        with pytest.raises(exc, match=text):
            twin(args[0], args[1], reads, args[2], args[3])
    lib = _native.load_library()
    out = _native.ctypes.c_void_p()
    assert lib.fz_batch_end_overlaps(None, None, om.LEV, b"ACGT", (_native.ctypes.c_uint64 * 2)(0, 4), 1, 1, 3, _native.ctypes.byref(out)) == _native.FZ_EINVAL
    assert lib.fz_last_error() == b"bad ctx/seq handle" and out.value is None
    with pytest.raises(ValueError, match="offsets must not decrease"):
        _native.end_overlaps_twin(om.LEV, [b"ACGT"], 1, 3, b"ACGT", np.array([0, 4, 2], dtype=np.uint64))
    for mode, patterns, k, o in ((om.LEV, [b"A" * 64], 16, 64), (om.SUBS, [b"A"], 0, 1), (om.LEV, [b"AC"] * 65534, 1, 1)):
        assert twin(mode, patterns, reads, k, o)[0].tolist() == [-1]    # the domain's corners are inside


class _StubHandle(object):
    n_seqs = 0

    def release(self):
        pass


class _StubEngine(object):
    """Logs what reaches it; a call that gets as far as the device answers rows of none."""

    def __init__(self, log, devices=(0,), comm=(0, -1, False)):
        self.log, self.devices, self.comm = log, list(devices), comm

    def comm_info(self):
        return self.comm

    def upload_batch(self, blob, offs):
        self.log.append(("upload", len(offs) - 1))
        h = _StubHandle()
        h.n_seqs, h.lengths = len(offs) - 1, np.diff(offs.astype(np.int64))
        return h

    def batch_end_overlaps(self, batch, mode, patterns, k, min_overlap):
        self.log.append(("overlaps", mode, list(patterns), k, min_overlap))
        rows = np.zeros(batch.n_seqs, dtype=_native.overlap_dtype())
        rows["pattern"], rows["start"] = 0xffff, batch.lengths
        return rows


def test_public_call_refuses_before_anything_is_uploaded(monkeypatch):
    log = []
    monkeypatch.setattr(_native, "default_engine", lambda: _StubEngine(log))
    call, seqs, U = fa.find_end_overlaps_batch, [b"ACGTACGTAC", b"TTTT"], _native.UnsupportedSearch
    for exc, text, args, kw in (
            (ValueError, "No limitations given", ([b"ACGTACGT"], seqs), {}),
            (TypeError, "positive integers or None", ([b"ACGTACGT"], seqs), dict(max_l_dist=-1)),
            (ValueError, "must be limited", ([b"ACGTACGT"], seqs), dict(max_substitutions=1)),
            (TypeError, "min_overlap must be an integer", ([b"ACGTACGT"], seqs), dict(max_l_dist=1, min_overlap=2.5)),
            (ValueError, "min_overlap must be at least 1", ([b"ACGTACGT"], seqs), dict(max_l_dist=1, min_overlap=0)),
            (U, "separate substitution / insertion / deletion limits are not supported", ([b"ACGTACGT"], seqs),
             dict(max_substitutions=1, max_insertions=1, max_deletions=0)),
            (U, "separate substitution", ([b"ACGTACGT"], seqs), dict(max_substitutions=0, max_l_dist=2)),
            (U, "budgets up to 16", ([b"A" * 40], seqs), dict(max_l_dist=17)),
            (U, "subsequence 1 is not bytes-like", ([b"ACGTACGT", "ACGTACGT"], seqs), dict(max_l_dist=1)),
            (ValueError, "subsequence 1 is empty", ([b"ACGTACGT", b""], seqs), dict(max_l_dist=1)),
            (U, "subsequence 0 is longer than 64 bytes", ([b"A" * 65], seqs), dict(max_l_dist=1)),
            (U, "subsequence 1 is not longer than the budget 4", ([b"ACGTACGT", b"ACGT"], seqs), dict(max_l_dist=4)),
            (U, "at most 65534 subsequences", ([b"ACGT"] * 65535, seqs), dict(max_l_dist=1)),
            (U, "bytes-like sequences of one kind", ([b"ACGTACGT"], ["ACGT", "TTTT"]), dict(max_l_dist=1)),
            (U, "bytes-like sequences of one kind", ([b"ACGTACGT"], [b"ACGT", "TTTT"]), dict(max_l_dist=1)),
            (U, "bytes-like sequences of one kind", ([b"ACGTACGT"], [[1, 2, 3]]), dict(max_l_dist=1))):
        with pytest.raises(exc, match=text):
            call(*args, **kw)
    assert log == []
    for engine in (_StubEngine(log, devices=(0, 1)), _StubEngine(log, comm=(2, 0, True))):
        monkeypatch.setattr(_native, "default_engine", lambda engine=engine: engine)
        with pytest.raises(U, match="single-device, non-collective engines"):
            call([b"ACGTACGT"], seqs, max_l_dist=1)
        held = fa.resident_batch(seqs, engine=engine)            # (such an engine keeps the list and uploads nothing)
        with pytest.raises(U, match="resident batch of bytes-like sequences"):
            call([b"ACGTACGT"], held, max_l_dist=1)
    assert log == []
    text_batch = fa.resident_batch(["ACGT", "TTTT"], engine=_StubEngine(log))
    del log[:]
    with pytest.raises(U, match="resident batch of bytes-like sequences"):
        call([b"ACGTACGT"], text_batch, max_l_dist=1)
    assert log == []


def test_public_call_reaches_the_engine_once_with_the_classified_limits(monkeypatch):
    log = []
    engine = _StubEngine(log)
    monkeypatch.setattr(_native, "default_engine", lambda: engine)
    seqs = [b"ACGTACGTAC", b"", b"TTTT"]
    res = fa.find_end_overlaps_batch(b"ACGTACGT", seqs, max_l_dist=2)
    assert log == [("upload", 3), ("overlaps", _native.MODE_LEV, [b"ACGTACGT"], 2, 3)]
    assert isinstance(res, fa.EndOverlaps) and len(res) == 3 and repr(res) == "EndOverlaps(3 sequences, 0 found)"
    assert res.pattern.dtype == np.int32 and res.overlap.dtype == np.int32 and res.dist.dtype == np.int32 and res.start.dtype == np.int64
    assert (res.pattern.tolist(), res.overlap.tolist(), res.dist.tolist(), res.start.tolist()) == ([-1] * 3, [0] * 3, [-1] * 3, [10, 0, 4])
    del log[:]
    held = fa.resident_batch(seqs, engine=engine)
    fa.find_end_overlaps_batch([bytearray(b"ACGTACGT"), memoryview(b"ACGTA")], held, max_substitutions=1, max_insertions=0, max_deletions=0, min_overlap=1)
    fa.find_end_overlaps_batch([b"ACGTACGT"], held, max_l_dist=0)
    assert log == [("upload", 3), ("overlaps", _native.MODE_SUBS, [b"ACGTACGT", b"ACGTA"], 1, 1), ("overlaps", _native.MODE_SUBS, [b"ACGTACGT"], 0, 3)]
    del log[:]
    assert len(fa.find_end_overlaps_batch([b"ACGTACGT"], [], max_l_dist=1)) == 0 and log == []
    rows = np.zeros(2, dtype=_native.overlap_dtype())
    rows["pattern"], rows["start"], rows["overlap"], rows["dist"] = [0xffff, 4], [7, 2], [0, 5], [0, 1]
    res = overlap._from_rows(rows)
    assert (res.pattern.tolist(), res.overlap.tolist(), res.dist.tolist(), res.start.tolist()) == ([-1, 4], [0, 5], [-1, 1], [7, 2])
    assert repr(res) == "EndOverlaps(2 sequences, 1 found)"
