"""Symbol classes on the multi-pattern pass, the parts that need no GPU: a whole class group run on the host by the functions
the kernels run (fz_device.h compiled with g++: tests/mp_cls_emul.cpp) against a brute-force model, the planner of a class
call (fz_debug_multi_plan_cls) and the argument handling of the three public calls with ``classes``."""
import ctypes
import itertools
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, assign, batch, classes, engine, multi, multi_batch
from tests import classes_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
IUPAC = fa.IUPAC_DNA
TABLES = classes.class_tables(IUPAC)
A_IUPAC = model.accept_table(IUPAC)
LETTERS = b"RYSWKMBDHVN"
ODD = b"Nacgt\n\x00\xff"                                   # sequence bytes that are no base symbol
SUBS = {"max_insertions": 0, "max_deletions": 0}


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(tempfile.gettempdir(), "fz_mp_cls_emul_%d.so" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "mp_cls_emul.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.mp_cls_emul_group.restype = ctypes.c_longlong
    L.mp_cls_emul_group.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint8,
                                    ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_uint32)]
    L.mp_cls_emul_block_hashes.restype = ctypes.c_uint32
    L.mp_cls_emul_block_hashes.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32]
    L.mp_cls_emul_hash.restype = ctypes.c_uint32
    L.mp_cls_emul_hash.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    yield L
    os.remove(out)


def _group_rows(L_, pats, k, L, text, tables=TABLES, pad=0):
    """-> (per pattern the rows (start, end, dist, block) of the host model of the group in the order they were produced,
    the group's table entries)."""
    blob, offs = _native.pack_patterns(pats)
    cap = 1 << 18
    out = (ctypes.c_int64 * (5 * cap))()
    nent = ctypes.c_uint32(0)
    c = L_.mp_cls_emul_group(blob, offs, len(pats), k, L, tables[0], tables[1], text, len(text), pad, out, cap, ctypes.byref(nent))
    assert 0 <= c <= cap, c
    per = [[] for _ in pats]
    for i in range(c):
        per[out[5 * i]].append((out[5 * i + 2], out[5 * i + 3], out[5 * i + 4], out[5 * i + 1]))
    return per, nent.value


def _check_group(L_, pats, k, text, A=A_IUPAC, tables=TABLES, pad=0):
    L = len(pats[0]) // (k + 1)
    got, _ = _group_rows(L_, pats, k, L, text, tables, pad)
    n = 0
    for p, g in zip(pats, got):
        want = model.raw_rows(p, text, k, A)
        assert len(set(g)) == len(g), ("a row twice", p, k)
        assert sorted(g, key=lambda r: (r[3], r[0])) == want, (p, k, len(text))
        n += len(want)
    return n


def _degenerate(rnd, m, where):
    """A DNA pattern of m bytes with IUPAC letters at the positions `where`."""
    p = bytearray(rnd.choice(b"ACGT") for _ in range(m))
    for q in where:
        p[q] = rnd.choice(LETTERS)
    return bytes(p)


def _spell(rnd, p, classes_=IUPAC):
    """One concrete spelling of p: every class letter replaced by a member of its set."""
    return bytes(rnd.choice(classes_[c]) if c in classes_ else c for c in p)


def _plant(rnd, text, p, k, nsub, at=None):
    """A spelling of p with nsub substitutions that no class forgives (a byte outside every set involved), at `at`."""
    q = bytearray(_spell(rnd, p))
    for pos in rnd.sample(range(len(p)), nsub):
        q[pos] = rnd.choice([t for t in b"ACGT" if not A_IUPAC[p[pos], t]] or ODD)
    at = rnd.randint(0, len(text) - len(q)) if at is None else at
    text[at:at + len(q)] = q
    return at


def _text(rnd, n, pats, k):
    text = bytearray(rnd.choice(b"ACGT") for _ in range(n))
    for _ in range(n // 50):
        text[rnd.randrange(n)] = rnd.choice(ODD)
    for p in pats:
        for nsub in (0, k, k + 1, rnd.randint(0, k)):
            if len(p) <= n:
                at = _plant(rnd, text, p, k, nsub)
                if rnd.random() < 0.5 and at + len(p) < n:
                    text[at + len(p)] = rnd.choice(ODD)    # a non-base byte right behind a planted site
    return bytes(text)


# (m, k): L = 4 (hash windows overlap), 5, 7, 8 (byte 4 unhashed), 10 (offsets 8, 9 unhashed), with and without a tail
SHAPES = [(12, 2), (23, 3), (20, 3), (15, 1), (16, 1), (24, 2), (40, 3), (43, 3), (61, 8), (128, 8)]


def _positions(m, k):
    """Class positions the issue names: pattern position 0, the last one, inside a block's hashed bytes, at block offset >= 8
    (where L > 8) and in the tail behind the last block (where there is one)."""
    L = m // (k + 1)
    tail = list(range((m // L) * L, m))
    out = {"first": [0], "last": [m - 1], "hashed": [L + 1, L + min(L, 8) - 1], "two blocks": [2, L + 2]}
    if L > 8:
        out["offset >= 8"] = [8, L + L - 1]
    if L >= 8:
        out["byte 4"] = [4, L + 4]
    if tail:
        out["tail"] = tail[-3:]
    return out


def test_group_model_equals_brute_force(emul):
    rnd = random.Random(41)
    rows = 0
    for m, k in SHAPES:
        for name, where in sorted(_positions(m, k).items()):
            pats = [_degenerate(rnd, m, where) for _ in range(3)] + [_degenerate(rnd, m, [])]
            pats.append(pats[0])                                                  # the same pattern twice: rows for both
            for n in (0, m - 1, m, 777, 4001):
                text = _text(rnd, n, pats, k) if n >= m else bytes(rnd.choice(b"ACGT") for _ in range(n))
                rows += _check_group(emul, pats, k, text)
    print("class group model: %d rows" % rows)
    assert rows > 2000


def test_every_window_alignment_and_the_bytes_behind_the_text(emul):
    """The four alignments of the window against the staged dwords, the window flush with the end of the text, and padding
    behind it that IS a base symbol: a class position in the pattern's last bytes must not match it."""
    rnd = random.Random(42)
    for m, k in ((12, 2), (23, 3), (41, 3), (18, 1)):
        L = m // (k + 1)
        pats = [_degenerate(rnd, m, [0, m - 1]), _degenerate(rnd, m, [m - 3, m - 2, m - 1]), _degenerate(rnd, m, [0, 1, L])]
        for align in range(4):
            for short in (0, 1, 2, 3):
                parts = [bytes(rnd.choice(b"ACGT") for _ in range(align))]
                for p in pats:
                    parts.append(_spell(rnd, p))
                    parts.append(bytes(rnd.choice(b"ACGT") for _ in range(rnd.randint(0, 3))))
                parts[-1] = b""
                # the last window ends with the text, or is `short` bytes too short to be a window at all
                text = b"".join(parts) + _spell(rnd, pats[1])[:m - short]
                for pad in (0, ord("A"), ord("N")):
                    assert _check_group(emul, pats, k, text, pad=pad) >= len(pats)


def test_text_bytes_are_never_classes(emul):
    """A sequence N matches a pattern N (equality) and no pattern A; lower case is no base symbol under IUPAC_DNA and is one
    under a case-folding table whose keys are base symbols themselves."""
    p = b"ACGTNCGTACGTACGTACGA"                                                    # m = 20, k = 3: L = 5
    text = b"TT" + b"ACGTNCGTACGTACGTACGA" + b"G" + b"NCGTNCGTACGTACGTACGA" + b"acgtacgtacgtacgtacga"
    got, _ = _group_rows(emul, [p], 3, 5, text)
    assert sorted(set((r[0], r[2]) for r in got[0])) == [(2, 0), (23, 1)] == model.windows_within(p, text, 3, A_IUPAC)
    fold = {ord(c): bytes([ord(c), ord(c.lower())]) for c in "ACGT"}
    tables = classes.class_tables(fold)
    q = b"ACGTACGTACGTACGTACGA"
    got, _ = _group_rows(emul, [q], 3, 5, text, tables)
    want = model.windows_within(q, text, 3, model.accept_table(fold))
    assert sorted(set((r[0], r[2]) for r in got[0])) == want and (43, 0) in want and (2, 1) in want


# ---- planner

def _entries_model(emul, p, k, classes_=IUPAC):
    """Distinct hashes over the spellings of the hashed bytes of every block, spelled out in Python."""
    m = len(p)
    L = m // (k + 1)
    H = min(L, 8)
    A = model.accept_table(classes_)
    total = 0
    for s in range(0, m - L + 1, L):
        alts = [[t for t in range(256) if A[c, t]] for c in p[s:s + H]]
        hashes = set(emul.mp_cls_emul_hash(bytes(sp) + p[s + H:s + L], L) for sp in itertools.product(*alts))
        total += len(hashes)
    return total


def test_plan_entries_are_the_distinct_hashes_of_the_spellings(emul):
    rnd = random.Random(43)
    for m, k in SHAPES:
        for where in _positions(m, k).values():
            p = _degenerate(rnd, m, where)
            group_of, per_pat, per_group = _native.multi_plan_classes([p], k, TABLES)
            assert group_of == [0] and per_group == per_pat
            assert per_pat[0] == _entries_model(emul, p, k), (m, k, where)
    # a plain pattern: one entry per block; an N in a hashed byte: itself and its four bases
    assert _native.multi_plan_classes([b"ACGT" * 5], 3, TABLES)[1] == [4]
    assert _native.multi_plan_classes([b"NCGT" + b"ACGT" * 4], 3, TABLES)[1] == [4 + 4]
    # class bytes that no hash covers are free: the NGG tail of a 23-mer at k = 3, block offsets >= 8, byte 4 of an L = 8 block
    guide = b"ACGTTGCAACGTTGCAACGT" + b"NGG"
    assert _native.multi_plan_classes([guide], 3, TABLES)[1] == [4]
    assert _native.multi_plan_classes([b"ACGTACGTNN" * 4], 3, TABLES)[1] == [4]
    assert _native.multi_plan_classes([b"ACGTNCGT" * 3], 2, TABLES)[1] == [3]
    # two spellings, one hash: a key whose set holds the key itself spells it once
    tables = classes.class_tables({ord("A"): b"Aa"})
    assert _native.multi_plan_classes([b"ACGTC" * 4], 3, tables)[1] == [2 * 4]


def test_plan_groups_close_at_256_entries_or_64_patterns():
    rnd = random.Random(44)
    dna = lambda m: bytes(rnd.choice(b"ACGT") for _ in range(m))
    plain = [dna(20) for _ in range(70)]                                           # 4 entries each: 64 patterns close the group
    group_of, per_pat, per_group = _native.multi_plan_classes(plain, 3, TABLES)
    assert group_of == [0] * 64 + [1] * 6 and per_group == [256, 24] and per_pat == [4] * 70
    # one N in a hashed byte of one block: 5 + 3 = 8 entries; 32 of them fill a table, the 33rd opens the next group
    deg = [b"N" + dna(19) for _ in range(40)]
    group_of, per_pat, per_group = _native.multi_plan_classes(deg, 3, TABLES)
    assert per_pat == [8] * 40 and group_of == [0] * 32 + [1] * 8 and per_group == [256, 64]
    # groups are per n-gram length, numbered by their first pattern; a list of one is a group
    assert _native.multi_plan_classes([dna(20), dna(24), dna(21)], 3, TABLES)[0] == [0, 1, 0]
    assert _native.multi_plan_classes([dna(23)], 3, TABLES) == ([0], [4], [4])
    assert _native.multi_plan_classes([], 3, TABLES) == ([], [], [])


def test_plan_refuses_by_position():
    rnd = random.Random(45)
    dna = lambda m: bytes(rnd.choice(b"ACGT") for _ in range(m))
    # NNNN in a block's first bytes at L = 4: 5^4 spellings in one block
    with pytest.raises(fa.UnsupportedSearch) as e:
        _native.multi_plan_classes([dna(20), b"NNNN" + dna(16)], 3, TABLES)
    assert "pattern 1" in str(e.value)
    # ... and four two-base letters: 3^4 = 81 + 3 fit
    assert _native.multi_plan_classes([b"RYSW" + dna(16)], 3, TABLES)[1] == [84]
    for pats, k in (([dna(20), dna(11)], 2), ([dna(20), dna(129)], 2), ([dna(90)], 9), ([dna(20)], 0)):
        with pytest.raises(fa.UnsupportedSearch) as e:
            _native.multi_plan_classes(pats, k, TABLES)
        assert "pattern %d" % (len(pats) - 1) in str(e.value)
    with pytest.raises(ValueError):
        _native.multi_plan_classes([dna(20)], 3, (TABLES[0], b"\x03" + TABLES[1][1:]))


def test_plan_is_a_function_of_the_arguments():
    rnd = random.Random(46)
    lists = []
    for _ in range(20):
        m, k = rnd.choice(SHAPES)
        lists.append(([_degenerate(rnd, m, rnd.sample(range(m), rnd.randint(0, 2))) for _ in range(rnd.randint(1, 80))], k))
    first = [_native.multi_plan_classes(p, k, TABLES) for p, k in lists]
    order = list(range(len(lists)))
    for _ in range(3):
        rnd.shuffle(order)
        for j in order:
            assert _native.multi_plan_classes(lists[j][0], lists[j][1], TABLES) == first[j]


# ---- arguments

def test_iupac_dna_and_the_tables():
    assert "IUPAC_DNA" in fa.__all__
    want = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
    assert {chr(c): v.decode() for c, v in IUPAC.items()} == want
    pmask, tmask = TABLES
    assert len(pmask) == len(tmask) == 256
    assert sorted(t for t in range(256) if tmask[t]) == sorted(b"ACGT") and sorted(tmask[t] for t in b"ACGT") == [1, 2, 4, 8]
    for c in range(256):
        assert pmask[c] == sum(tmask[t] for t in IUPAC.get(c, b""))
    assert classes.class_tables({b"N": bytearray(b"ACGT"), ord("R"): memoryview(b"AG")}) == classes.class_tables({ord("N"): b"ACGT", ord("R"): b"AG"})
    with pytest.raises(ValueError, match="9 distinct"):
        classes.class_tables({ord("X"): b"ABCDEFGHI"})
    with pytest.raises(ValueError, match="empty"):
        classes.class_tables({ord("X"): b""})
    with pytest.raises(ValueError, match="256"):
        classes.class_tables({256: b"A"})
    with pytest.raises(ValueError):
        classes.class_tables({b"NN": b"A"})
    with pytest.raises(TypeError):
        classes.class_tables({"N": b"ACGT"})
    assert len(classes.class_tables({ord("X"): b"ABCDEFGH"})[0]) == 256


def test_exports():
    names = {"fz_subs_ngrams_multi_cls", "fz_subs_ngrams_multi_best_cls", "fz_batch_search_multi_cls", "fz_batch_assign_cls",
             "fz_debug_multi_plan_cls"}
    assert names <= set(_native.EXPORTED_SYMBOLS)
    lib = _native.load_library()
    for name in names:
        assert getattr(lib, name) is not None
    assert {"subs_ngrams_multi_classes", "multi_rows_call_classes", "batch_multi_rows_call_classes", "batch_search_multi_classes",
            "batch_assign_classes"} <= set(dir(_native.Engine))


class _NoRows(object):
    n, address = 0, 0

    def release(self):
        pass

    def to_array(self):
        return np.empty(0, dtype=_native._match_dtype())


class _StubHandle(object):
    n_seqs = 0

    def release(self):
        pass


class _StubEngine(object):
    """Logs which entry point a call reaches; every search finds nothing."""
    devices = [0]

    def __init__(self, log):
        self.log = log

    def comm_info(self):
        return 0, -1, False

    def upload_batch(self, blob, offs):
        self.log.append(("upload",))
        h = _StubHandle()
        h.n_seqs = len(offs) - 1
        return h

    def multi_rows_call(self, handle, patterns, k, mode=_native.MODE_LEV):
        self.log.append(("multi", list(patterns), k, mode))
        return _NoRows(), [0] * (len(patterns) + 1)

    def multi_rows_call_classes(self, handle, patterns, k, tables):
        self.log.append(("multi_classes", list(patterns), k, tables))
        return _NoRows(), [0] * (len(patterns) + 1)

    def batch_multi_rows_call(self, handle, mode, patterns, k, reduced=True):
        self.log.append(("batch", mode, list(patterns), k, reduced))
        return _NoRows(), np.empty(0, dtype=np.uint32), [0] * (len(patterns) + 1)

    def batch_multi_rows_call_classes(self, handle, patterns, k, tables, reduced=True):
        self.log.append(("batch_classes", list(patterns), k, tables, reduced))
        return _NoRows(), np.empty(0, dtype=np.uint32), [0] * (len(patterns) + 1)

    def batch_assign(self, handle, mode, patterns, k):
        self.log.append(("assign", mode, list(patterns), k))
        rows = np.zeros(handle.n_seqs, dtype=_native.assign_dtype())
        rows["pattern"] = -1
        return rows

    def batch_assign_classes(self, handle, patterns, k, tables):
        self.log.append(("assign_classes", list(patterns), k, tables))
        rows = np.zeros(handle.n_seqs, dtype=_native.assign_dtype())
        rows["pattern"] = -1
        return rows


def _stub_sequence(log, original):
    seq = engine.DeviceSequence.__new__(engine.DeviceSequence)
    seq.original, seq.engine, seq.byteslike, seq.handle = original, _StubEngine(log), not isinstance(original, str), _StubHandle()
    return seq


PATS = [b"ACGTACGTACGTACGTACGTNGG", b"ACGTTGCAACGTTGCAACGTNGG"]                       # m = 23


def test_none_reaches_the_existing_entry_points_and_a_mapping_the_class_ones():
    log = []
    seq = _stub_sequence(log, b"ACGT" * 10)
    held = batch.BatchSequences([b"ACGT" * 10, b"", b"TTTT"], engine=_StubEngine(log))
    kw = dict(max_substitutions=3, **SUBS)
    del log[:]
    assert multi.find_near_matches_multi(PATS, seq, classes=None, **kw) == multi.find_near_matches_multi(PATS, seq, **kw) == [[], []]
    assert multi_batch.find_near_matches_multi_batch(PATS, held, classes=None, **kw) == [[[], [], []]] * 2
    assert list(assign.find_best_matches_batch(PATS, held, classes=None, **kw).pattern) == [-1] * 3
    assert [e[0] for e in log] == ["multi", "multi", "batch", "assign"]
    assert log[0] == log[1] == ("multi", PATS, 3, _native.MODE_SUBS)           # (the reduced substitutions entry, named by its mode)
    assert log[2][1] == log[3][1] == _native.MODE_SUBS
    del log[:]
    assert multi.find_near_matches_multi(PATS, seq, classes=IUPAC, **kw) == [[], []]
    assert multi_batch.find_near_matches_multi_batch(PATS, held, classes=IUPAC, **kw) == [[[], [], []]] * 2
    assert list(assign.find_best_matches_batch(PATS, held, classes=IUPAC, **kw).pattern) == [-1] * 3
    assert [e[0] for e in log] == ["multi_classes", "batch_classes", "assign_classes"]
    assert all(e[-2 if e[0] == "batch_classes" else -1] == TABLES for e in log) and all(e[1] == PATS and e[2] == 3 for e in log)
    # a list of one, and a list without any class byte, ride the class entry points too: the loop cannot answer
    del log[:]
    multi.find_near_matches_multi([b"ACGT" * 5], seq, classes=IUPAC, max_substitutions=2, max_l_dist=1, **SUBS)
    assert log == [("multi_classes", [b"ACGT" * 5], 1, TABLES)]
    del log[:]
    assert multi.find_near_matches_multi([], seq, classes=IUPAC, **kw) == []
    assert multi_batch.find_near_matches_multi_batch([], held, classes=IUPAC, **kw) == []
    assert multi_batch.find_near_matches_multi_batch(PATS, [], classes=IUPAC, **kw) == [[], []]
    assert len(assign.find_best_matches_batch([], held, classes=IUPAC, **kw)) == 3
    assert log == []


CALLS = [lambda pats, seqs, **kw: multi.find_near_matches_multi(pats, seqs[0], **kw),
         lambda pats, seqs, **kw: multi_batch.find_near_matches_multi_batch(pats, seqs, **kw),
         lambda pats, seqs, **kw: assign.find_best_matches_batch(pats, seqs, **kw)]


@pytest.mark.parametrize("call", CALLS, ids=["multi", "multi_batch", "best"])
def test_refusals_come_before_any_search(monkeypatch, call):
    def no_engine(*a, **kw):
        raise AssertionError("a refused call reached the engine")
    monkeypatch.setattr(_native, "default_engine", no_engine)
    seqs = [b"ACGT" * 10, b"TTTT"]
    kw = dict(max_substitutions=3, classes=IUPAC, **SUBS)
    with pytest.raises(ValueError):
        call(PATS, seqs, max_substitutions=3, classes={ord("X"): b"ABCDEFGHI"}, **SUBS)
    with pytest.raises(ValueError):
        call(PATS, seqs, max_substitutions=3, classes={ord("X"): b""}, **SUBS)
    with pytest.raises(ValueError):
        call(PATS, seqs, max_substitutions=3, classes={256: b"A"}, **SUBS)
    with pytest.raises(ValueError, match="must be limited"):
        call(PATS, seqs, max_substitutions=3, classes=IUPAC)
    with pytest.raises(TypeError):
        call(PATS, seqs, max_substitutions=-1, classes=IUPAC, **SUBS)
    for limits in ({"max_l_dist": 2}, {"max_l_dist": 2, "max_insertions": 0}, {"max_substitutions": 1, "max_insertions": 1, "max_deletions": 0}):
        with pytest.raises(fa.UnsupportedSearch, match="mismatch-only"):
            call(PATS, seqs, classes=IUPAC, **limits)
    with pytest.raises(fa.UnsupportedSearch, match="at least one substitution"):
        call(PATS, seqs, max_substitutions=0, classes=IUPAC, **SUBS)
    with pytest.raises(fa.UnsupportedSearch, match="bytes-like sequences"):
        call(PATS, ["ACGT" * 10, "TTTT"], **kw)
    with pytest.raises(fa.UnsupportedSearch, match="subsequence 1 is not bytes-like"):
        call([PATS[0], "ACGTACGTACGTACGTACGTNGG"], seqs, **kw)
    for bad in (b"ACGTACGTACGTNGG", b"A" * 129, b""):                                # L = 3; m > 128; empty
        with pytest.raises(fa.UnsupportedSearch, match="subsequence 2 "):
            call(PATS + [bad], seqs, **kw)
    with pytest.raises(fa.UnsupportedSearch, match="subsequence 0 "):
        call([b"ACGT" * 30], seqs, max_substitutions=9, classes=IUPAC, **SUBS)      # k = 9
    with pytest.raises(fa.UnsupportedSearch, match="pattern 2"):
        call(PATS + [b"NNNN" + b"ACGT" * 4 + b"ACG"], seqs, **kw)                     # 625 spellings of one block
