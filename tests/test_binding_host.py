"""The ctypes binding against the header it binds: CPU only, no device.

_native.PROTOTYPES is the one statement of the C-ABI on the Python side.  A wrong entry truncates a 64-bit argument or
misplaces a pointer without any error, so every line is held against its prototype in include/fzhip.h here; the other
tests are about what stands around the table: what load_library() declares, what a build without an optional entry
point answers, and who frees a result buffer."""
import ctypes
import gc
import os
import re
import threading

import numpy as np
import pytest

from fuzzysearch_amd import _native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fzhip.h")
INT_CLASS = {"double": "f64", "uint64_t": "i64", "int64_t": "i64", "uint32_t": "i32", "int32_t": "i32", "int": "int"}
RETURN_CLASS = dict(INT_CLASS, void="void")
RETURN_CLASS["uint64_t"], RETURN_CLASS["uint32_t"] = "u64", "u32"


def header_prototypes():
    """include/fzhip.h without its comments -> {name: (return class, [parameter classes])} of every fz_*(...); prototype."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(fz_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        ret = " ".join(ret.replace("*", " * ").split())
        ret_class = "str" if ret == "const char *" else RETURN_CLASS[ret]
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        classes = []
        for p in params:
            if "*" in p:
                classes.append("ptr")
            else:
                words = [w for w in p.split() if w != "const"]
                assert len(words) == 2, (name, p)                 # one type word, one declarator
                classes.append(INT_CLASS[words[0]])
        protos[name] = (ret_class, classes)
    return protos


def ctype_class(t, returned=False):
    if t is None:
        return "void"
    if t is ctypes.c_char_p and returned:
        return "str"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    if returned and t in (ctypes.c_uint64, ctypes.c_uint32):
        return "u64" if t is ctypes.c_uint64 else "u32"
    return {ctypes.c_double: "f64", ctypes.c_uint64: "i64", ctypes.c_int64: "i64", ctypes.c_uint32: "i32", ctypes.c_int: "int"}[t]


def disagreements(table, protos):
    """Every way `table` differs from the header's prototypes, as readable strings."""
    bad = ["only in the header: %s" % n for n in sorted(set(protos) - set(table))]
    bad += ["only in the table: %s" % n for n in sorted(set(table) - set(protos))]
    for name in sorted(set(table) & set(protos)):
        restype, argtypes = table[name]
        want_ret, want = protos[name]
        if ctype_class(restype, returned=True) != want_ret:
            bad.append("%s returns %s, the table says %s" % (name, want_ret, ctype_class(restype, returned=True)))
        got = [ctype_class(t) for t in argtypes]
        if len(got) != len(want):
            bad.append("%s takes %d arguments, the table has %d" % (name, len(want), len(got)))
        else:
            bad += ["%s argument %d is %s, the table says %s" % (name, i, w, g) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    return bad


def test_the_prototype_table_is_the_header():
    protos = header_prototypes()
    assert len(protos) > 90 and protos["fz_free"] == ("void", ["ptr"]) and protos["fz_last_error"] == ("str", [])
    assert protos["fz_seq_add_shard"] == ("int", ["ptr", "int", "ptr", "i64", "i64", "i64", "i64"])
    assert protos["fz_debug_scan_regions"][1] == ["i64", "i64", "i32", "int", "f64", "int", "ptr", "ptr"]
    assert protos["fz_seq_len"][0] == "u64" and protos["fz_debug_scan_items"] == ("u32", [])
    assert disagreements(_native.PROTOTYPES, protos) == []
    assert list(_native.PROTOTYPES) == list(protos), "the table is kept in the header's order"
    assert _native.EXPORTED_SYMBOLS == tuple(_native.PROTOTYPES) and _native.OPTIONAL <= set(_native.PROTOTYPES)
    # the comparison sees a narrowed integer and two swapped neighbours: one mutation each, on a copy
    narrowed = dict(_native.PROTOTYPES)
    restype, args = narrowed["fz_seq_upload"]
    assert args[2] is ctypes.c_uint64
    narrowed["fz_seq_upload"] = (restype, args[:2] + (ctypes.c_uint32,) + args[3:])
    assert disagreements(narrowed, protos) == ["fz_seq_upload argument 2 is i64, the table says i32"]
    swapped = dict(_native.PROTOTYPES)
    restype, args = swapped["fz_batch_search"]
    assert (args[5], args[6]) == (ctypes.c_uint32, ctypes.c_int)                      # k, reduced
    swapped["fz_batch_search"] = (restype, args[:5] + (args[6], args[5]) + args[7:])
    assert disagreements(swapped, protos) == ["fz_batch_search argument 5 is i32, the table says int",
                                              "fz_batch_search argument 6 is int, the table says i32"]
    shorter = dict(_native.PROTOTYPES)
    shorter["fz_free"] = (ctypes.c_int, ())
    assert len(disagreements(shorter, protos)) == 2


def test_load_library_declares_the_table():
    lib = _native.load_library()
    for name, (restype, argtypes) in _native.PROTOTYPES.items():
        assert hasattr(lib, name), name                          # (the tree's own build has the optional ones too)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name


class _Without(object):
    """The loaded library with one symbol hidden: what an older build looks like to the binding."""

    def __init__(self, lib, hidden):
        self._lib, self._hidden = lib, hidden

    def __getattr__(self, name):
        if name == self._hidden:
            raise AttributeError(name)
        return getattr(self._lib, name)


def test_a_build_without_an_optional_entry_point_refuses_the_call(monkeypatch):
    lib = _native.load_library()
    for name in sorted(_native.OPTIONAL):
        with pytest.raises(_native.UnsupportedSearch, match=r"\b%s\b" % name):
            _native._entry(_Without(lib, name), name)
        assert _native._entry(_Without(lib, "fz_free"), name) is getattr(lib, name)
    # ... through the callers: module functions, and Engine methods before they touch the context
    host_calls = {"fz_debug_scan_items": lambda: _native.scan_items(),
                  "fz_debug_fasta_src": lambda: _native.fasta_src(0, 60, 61, 5),
                  "fz_debug_records_split": lambda: _native.records_split(b"ACGT\n", 1, 0, 0),
                  "fz_debug_multi_plan_cls": lambda: _native.multi_plan_classes([b"ACGT" * 5], 3, (bytes(256), bytes(256)))}
    for name, call in host_calls.items():
        monkeypatch.setattr(_native, "load_library", lambda name=name: _Without(lib, name))
        with pytest.raises(_native.UnsupportedSearch, match=name):
            call()
    monkeypatch.undo()
    eng = _native.Engine.__new__(_native.Engine)                 # no context: the refusal comes before the call
    eng._h, eng._lock = None, threading.RLock()
    handle = _native.ResidentSequence(eng, None, 0)
    handle.n_seqs = 0
    tables = (bytes(256), bytes(256))
    engine_calls = {"fz_mem_info": lambda: eng.mem_info(),
                    "fz_batch_search_multi": lambda: eng.batch_search_multi(handle, _native.MODE_LEV, [b"ACGT"], 1),
                    "fz_batch_search_multi_cls": lambda: eng.batch_search_multi_classes(handle, [b"ACGT"], 1, tables),
                    "fz_batch_assign": lambda: eng.batch_assign(handle, _native.MODE_SUBS, [b"ACGT"], 1),
                    "fz_batch_assign_cls": lambda: eng.batch_assign_classes(handle, [b"ACGT"], 1, tables),
                    "fz_subs_ngrams_multi_best_cls": lambda: eng.multi_rows_call_classes(handle, [b"ACGT"], 1, tables),
                    "fz_subs_ngrams_multi_cls": lambda: eng.subs_ngrams_multi_classes(handle, [b"ACGT"], 1, tables),
                    "fz_batch_upload_records": lambda: eng.upload_records(b"ACGT\n", 1, 0, 0)}
    for name, call in engine_calls.items():
        eng._lib = _Without(lib, name)
        with pytest.raises(_native.UnsupportedSearch, match=r"\b%s\b" % name):
            call()
    eng._lib = lib
    with pytest.raises(ValueError, match="substitutions mode"):  # the class entry points count mismatches only
        eng.batch_assign(handle, _native.MODE_LEV, [b"ACGT"], 1, tables)


class _CountingLib(object):
    """fz_free of the loaded library, with the addresses it was given written down."""

    def __init__(self, lib):
        self._lib, self.freed = lib, []

    def fz_free(self, p):
        self.freed.append(ctypes.cast(p, ctypes.c_void_p).value)
        self._lib.fz_free(p)


def _library_buffer(n):
    """A buffer of the library's own with n fz_match rows (fz_consolidate of n matches that do not overlap: host only)
    -> (pointer, its address, its bytes)."""
    lib = _native.load_library()
    rows = np.zeros(n, dtype=_native._match_dtype())
    rows["start"] = np.arange(n) * 100
    rows["end"] = rows["start"] + 20
    rows["dist"] = np.arange(n) % 3
    rows["block"] = -1
    ptr, cnt = ctypes.POINTER(_native.FzMatch)(), ctypes.c_uint64(0)
    _native._check(lib.fz_consolidate(ctypes.cast(rows.ctypes.data, ctypes.POINTER(_native.FzMatch)), n, ctypes.byref(ptr), ctypes.byref(cnt)))
    assert cnt.value == n
    addr = ctypes.cast(ptr, ctypes.c_void_p).value
    return ptr, addr, ctypes.string_at(addr, n * 24)


VIEW_BYTES = 256 << 10
# (dtype, rows of the dtype): on both sides of the 256 KiB rule, and at the rule itself where the row size divides it
TAKE_CASES = [("match", 100), ("match", VIEW_BYTES // 24), ("match", VIEW_BYTES // 24 + 1), ("match", 20000),
              ("assign", 150), ("assign", VIEW_BYTES // 16 - 1), ("assign", VIEW_BYTES // 16), ("assign", 30000)]


@pytest.mark.parametrize("kind,n", TAKE_CASES)
@pytest.mark.parametrize("by_address", [False, True])
def test_take_rows_copies_small_buffers_and_views_large_ones(kind, n, by_address):
    dtype = _native._match_dtype() if kind == "match" else _native.assign_dtype()
    nbytes = n * dtype.itemsize
    ptr, addr, content = _library_buffer(-(-nbytes // 24))
    lib = _CountingLib(_native.load_library())
    arr = _native._take_rows(lib, addr if by_address else ptr, n, dtype)
    assert arr.dtype == dtype and arr.shape == (n,) and arr.tobytes() == content[:nbytes]
    if nbytes < VIEW_BYTES:
        assert lib.freed == [addr] and arr.ctypes.data != addr and arr.flags.owndata
        del arr
        gc.collect()
        assert lib.freed == [addr]
        return
    assert lib.freed == [] and arr.ctypes.data == addr and not arr.flags.owndata
    tail = arr[n // 2:]
    del arr
    gc.collect()
    assert lib.freed == [] and tail.tobytes() == content[(n // 2) * dtype.itemsize:nbytes]
    del tail
    gc.collect()
    assert lib.freed == [addr]


def test_the_named_takers_are_take_rows():
    for n in (7, 20000):
        ptr, addr, content = _library_buffer(n)
        lib = _CountingLib(_native.load_library())
        got = _native._take_matches_array(lib, ptr, n)
        assert got.dtype == _native._match_dtype() and got.tobytes() == content
        del got
        gc.collect()
        assert lib.freed == [addr]
        ptr, addr, content = _library_buffer(n)
        got = _native._take_assign_array(lib, addr, n)
        assert got.dtype == _native.assign_dtype() and got.tobytes() == content[:n * 16]
        del got
        gc.collect()
        assert lib.freed[1:] == [addr]
    ptr, addr, content = _library_buffer(5)
    lib = _CountingLib(_native.load_library())
    assert _native._take_matches(lib, ptr, 5) == [(i * 100, i * 100 + 20, i % 3, -1) for i in range(5)] and lib.freed == [addr]
