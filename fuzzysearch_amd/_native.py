"""ctypes binding of libfzhip.so (include/fzhip.h).  No PyTorch, no CPU fallback.

The library is built in-tree by ``fuzzysearch_amd/build.py`` (hipcc, gfx950).  If it is missing or
there is no MI355X, every search raises — this package never computes matches on the CPU.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# FUZZYSEARCH_HIP_LIB: another build of the same C-ABI (A/B benchmarking of kernel versions)
LIB_PATH = os.environ.get("FUZZYSEARCH_HIP_LIB") or os.path.join(_HERE, "libfzhip.so")

FZ_OK, FZ_EINVAL, FZ_ENOMEM, FZ_EDEVICE, FZ_EUNSUPPORTED, FZ_EHALO, FZ_ETIMEOUT = 0, -1, -2, -3, -4, -5, -6
UINT64_MAX = (1 << 64) - 1


class FzMatch(ctypes.Structure):
    _fields_ = [("start", ctypes.c_int64), ("end", ctypes.c_int64),
                ("dist", ctypes.c_int32), ("block", ctypes.c_int32)]


class FzRecordsInfo(ctypes.Structure):
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_seqs", ctypes.c_uint64), ("packed_bytes", ctypes.c_uint64),
                ("bad_record", ctypes.c_uint64), ("bad_reason", ctypes.c_uint32)]


class FzDeriveInfo(ctypes.Structure):
    _fields_ = [("n_out", ctypes.c_uint64), ("packed_bytes", ctypes.c_uint64), ("longest", ctypes.c_uint64),
                ("bad_item", ctypes.c_uint64), ("bad_reason", ctypes.c_uint32)]


class FzFormatInfo(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64), ("longest_record", ctypes.c_uint64),
                ("bad_record", ctypes.c_uint64), ("bad_reason", ctypes.c_uint32)]


class FzStats(ctypes.Structure):
    _fields_ = [("bytes_scanned", ctypes.c_uint64), ("ngram_hits", ctypes.c_uint64),
                ("raw_matches", ctypes.c_uint64), ("filter_ms", ctypes.c_double),
                ("verify_ms", ctypes.c_double), ("device_ms", ctypes.c_double),
                ("filter_launches", ctypes.c_uint32), ("n_devices", ctypes.c_uint32),
                ("verify_form", ctypes.c_uint32), ("reserved_", ctypes.c_uint32)]


# FzStats.verify_form (include/fzhip.h: FZ_FORM_*)
FORM_NONE, FORM_FUSED_BAND, FORM_FUSED_CELLS, FORM_FUSED_BITS1, FORM_FUSED_BITS2, FORM_KERNEL, FORM_FUSED_BITS32 = range(7)


class HipEngineError(RuntimeError):
    """libfzhip.so missing / no usable gfx950 device / HIP runtime failure."""


class CollectiveTimeout(HipEngineError):
    """A collective of the context's communicator did not complete within FZ_COMM_TIMEOUT_MS (a rank never arrived)."""


# The C types of the prototypes.  vp: a handle or any untyped pointer; bp: bytes (a bytes object, an address or None).
vp = bp = ctypes.c_void_p
u32, u64, i64, ci, f64, cs = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_char_p
vpp, cip, f64p = ctypes.POINTER(vp), ctypes.POINTER(ci), ctypes.POINTER(f64)
u32p, u64p, mp = ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(FzMatch)
u32pp, u64pp, mpp = ctypes.POINTER(u32p), ctypes.POINTER(u64p), ctypes.POINTER(mp)
rip, dip, stp = ctypes.POINTER(FzRecordsInfo), ctypes.POINTER(FzDeriveInfo), ctypes.POINTER(FzStats)
fip = ctypes.POINTER(FzFormatInfo)

_SEARCH = (ci, (vp, vp, bp, u32, u32, mpp, u64p))                          # (ctx, seq, p, m, k, &rows, &n)
_GENERIC = (ci, (vp, vp, bp, u32, u32, u32, u32, u32, mpp, u64p))          # (ctx, seq, p, m, subs, ins, dels, l, &rows, &n)
_BEGIN = (ci, (vp, vp, bp, u32, u32))
_END = (ci, (vp, mpp, u64p))
_ANY = (ci, (vp, vp, bp, u32, u32, cip))
_MULTI = (ci, (vp, vp, bp, u64p, u32, u32, mpp, u64pp))                    # (ctx, seq, pats, offs, n_pats, k, &rows, &offsets)
_MULTI_CLS = (ci, (vp, vp, bp, u64p, u32, u32, bp, bp, mpp, u64pp))        # ... with pmask, tmask behind k
_REDUCE = (ci, (mp, u64, mpp, u64p))

# Every symbol include/fzhip.h declares, in its order: name -> (restype, argtypes).  load_library() declares exactly
# these; tests/test_binding_host.py holds every line against the header's prototype.
PROTOTYPES = {
    "fz_abi_version": (ci, ()),
    "fz_last_error": (cs, ()),
    "fz_device_count": (ci, (cip,)),
    "fz_create": (ci, (cip, ci, vpp)),
    "fz_destroy": (None, (vp,)),
    "fz_seq_upload": (ci, (vp, bp, u64, vpp)),
    "fz_seq_upload_shard": (ci, (vp, bp, u64, u64, u64, u64, u64, vpp)),
    "fz_seq_new": (ci, (vp, u64, vpp)),
    "fz_seq_add_shard": (ci, (vp, ci, bp, u64, u64, u64, u64)),
    "fz_seq_len": (u64, (vp,)),
    "fz_seq_release": (None, (vp,)),
    "fz_search_exact": (ci, (vp, vp, bp, u32, u64, u64, u64pp, u64p)),
    "fz_lev_ngrams": _SEARCH,
    "fz_lev_ngrams_begin": _BEGIN,
    "fz_lev_ngrams_end": _END,
    "fz_subs_ngrams_begin": _BEGIN,
    "fz_generic_ngrams_begin": (ci, (vp, vp, bp, u32, u32, u32, u32, u32, ci)),
    "fz_search_end": _END,
    "fz_subs_ngrams": _SEARCH,
    "fz_generic_ngrams": _GENERIC,
    "fz_generic_ngrams_consolidated": _GENERIC,
    "fz_lev_ngrams_consolidated": _SEARCH,
    "fz_subs_ngrams_best": _SEARCH,
    "fz_lev_ngrams_multi": _MULTI,
    "fz_lev_ngrams_multi_consolidated": _MULTI,
    "fz_debug_multi_plan": (ci, (bp, u64p, u32, u32, u32p, u32p)),
    "fz_subs_ngrams_multi": _MULTI,
    "fz_subs_ngrams_multi_best": _MULTI,
    "fz_debug_multi_plan_mode": (ci, (u32, bp, u64p, u32, u32, u32p, u32p)),
    "fz_batch_upload": (ci, (vp, bp, u64p, u64, vpp)),
    "fz_batch_search": (ci, (vp, vp, u32, bp, u32, u32, ci, mpp, u32pp, u64p)),
    "fz_batch_search_multi": (ci, (vp, vp, u32, bp, u64p, u32, u32, ci, mpp, u32pp, u64pp)),
    "fz_batch_assign": (ci, (vp, vp, u32, bp, u64p, u32, u32, vpp)),
    "fz_debug_assign_fold": (ci, (vp, u64, vp, u64, u32, vp, u32, vp, u32, u32, vp)),
    "fz_batch_end_overlaps": (ci, (vp, vp, u32, bp, u64p, u32, u32, u32, vpp)),
    "fz_debug_end_overlaps": (ci, (u32, bp, u64p, u32, u32, u32, bp, vp, u64, vp)),
    "fz_debug_overlap_ms": (ci, (vp, f64p)),
    "fz_batch_score_cuts": (ci, (vp, vp, vp, vp, u32, u32, u32, vpp)),
    "fz_debug_score_cuts": (ci, (vp, vp, u32, u32, u32, bp, vp, u64, vp)),
    "fz_debug_cuts_ms": (ci, (vp, f64p)),
    "fz_subs_ngrams_multi_cls": _MULTI_CLS,
    "fz_subs_ngrams_multi_best_cls": _MULTI_CLS,
    "fz_batch_search_multi_cls": (ci, (vp, vp, bp, u64p, u32, u32, bp, bp, ci, mpp, u32pp, u64pp)),
    "fz_batch_assign_cls": (ci, (vp, vp, bp, u64p, u32, u32, bp, bp, vpp)),
    "fz_debug_multi_plan_cls": (ci, (bp, u64p, u32, u32, bp, bp, u32p, u32p, u32p, u32p)),
    "fz_debug_batch_segment": (ci, (u64p, u64, u64, u64p, u64p, u64p)),
    "fz_batch_upload_records": (ci, (vp, bp, u64, u32, u32, u32, vpp, rip)),
    "fz_batch_tables": (ci, (vp, vp, vp)),
    "fz_debug_batch_bytes": (ci, (vp, vp, u64)),
    "fz_debug_records_split": (ci, (bp, u64, u32, u32, u32, vpp, vpp, vpp, rip)),
    "fz_debug_scan_items": (u32, ()),
    "fz_debug_records_ms": (ci, (vp, f64p)),
    "fz_batch_upload_fasta": (ci, (vp, bp, u64, u32, vpp, rip)),
    "fz_batch_fasta_index": (ci, (vp, vp)),
    "fz_debug_fasta_split": (ci, (bp, u64, u32, vpp, vpp, vpp, rip)),
    "fz_debug_fasta_upper4": (u32, (u32,)),
    "fz_debug_fasta_src": (u64, (u64, u64, u64, u64)),
    "fz_batch_derive": (ci, (vp, vp, vp, vp, vp, u64, u32, bp, vpp, dip)),
    "fz_debug_derive_plan": (ci, (vp, u64, vp, vp, vp, u64, vp, vp, dip)),
    "fz_debug_derive_ms": (ci, (vp, f64p)),
    "fz_batch_upload_records_lines": (ci, (vp, bp, u64, u32, vp, u32, u32, vpp, rip)),
    "fz_batch_format": (ci, (vp, vp, u32, bp, vp, u32, u32, vp, u64, fip)),
    "fz_debug_format_plan": (ci, (vp, u32, u64, vp, u32, u32, vp, fip)),
    "fz_debug_format_ms": (ci, (vp, f64p)),
    "fz_subs_ngrams_any": _ANY,
    "fz_subs_lp_any": _ANY,
    "fz_generic_ngrams_any": (ci, (vp, vp, bp, u32, u32, u32, u32, u32, cip)),
    "fz_lev_lp": _SEARCH,
    "fz_subs_lp": _SEARCH,
    "fz_generic_lp": _GENERIC,
    "fz_comm_unique_id": (ci, (vp, u64)),
    "fz_comm_init_rank": (ci, (vp, vp, ci, ci)),
    "fz_comm_init_all": (ci, (vp,)),
    "fz_comm_info": (ci, (vp, cip, cip, cip)),
    "fz_comm_set_collective": (ci, (vp, ci)),
    "fz_comm_allgather": (ci, (vp, vp, u64, vp)),
    "fz_comm_max_f64": (ci, (vp, f64p)),
    "fz_comm_barrier": (ci, (vp,)),
    "fz_comm_destroy": (None, (vp,)),
    "fz_comm_gather_ms": (ci, (vp, f64p)),
    "fz_comm_backend": (ci, ()),
    "fz_consolidate": _REDUCE,
    "fz_group_best": _REDUCE,
    "fz_merge_ranks": (ci, (vp, vp, vp, u32, u32, vp)),
    "fz_wire_pack": (ci, (vp, u64, u64, vp)),
    "fz_wire_merge": (ci, (vp, u32, u64, u64, vp, u64, u64p, u64p)),
    "fz_stream_open": (ci, (vp, u32, bp, u32, u32, u32, u32, u32, u64, u32, u32, u64, vpp)),
    "fz_stream_buffer": (ci, (vp, vpp, u64p)),
    "fz_stream_submit": (ci, (vp, u64, ci)),
    "fz_stream_read_fd": (ci, (vp, ci, i64, ci, u64p)),
    "fz_stream_finish": (ci, (vp, mpp, u32pp, u64p)),
    "fz_stream_close": (None, (vp,)),
    "fz_debug_reload_switches": (None, ()),
    "fz_debug_launch_plan": (ci, (bp, u32, u32, u32p, u32, u32p)),
    "fz_debug_order_records": (ci, (vp, u64, u32, mpp, u64p)),
    "fz_debug_order_records_bounded": (ci, (vp, u64, u32, u64, u32, mpp, u64p)),
    "fz_debug_order_segments": (ci, (vp, vp, u32, u32, mpp, u64p)),
    "fz_debug_scan_regions": (ci, (u64, u64, u32, ci, f64, ci, u32p, vp)),
    "fz_debug_scan_plan": (ci, (cs, u32, u32, u64, u32, ci, u32p, u32p, cip, u32p, vp)),
    "fz_debug_scan_instance": (ci, (u32, cs, u32, u32, u64, u32, u32p, u32p, u32p)),
    "fz_debug_scan_walk": (ci, (u64, u32, u32, vp, u32, u32, ci, u64p)),
    "fz_debug_scan_direction": (ci, (vp, vp, cip, u64p)),
    "fz_debug_gather_merge": (ci, (vp, u32, u64, vp, u32, mpp, u64p, u64p)),
    "fz_stats": (ci, (vp, stp)),
    "fz_mem_info": (ci, (vp, u64p, u64p)),
    "fz_set_timing": (ci, (vp, ci)),
    "fz_set_streams": (ci, (vp, ci)),
    "fz_set_scan_direction": (ci, (vp, ci)),
    "fz_device_ms": (ci, (vp, f64p, ci)),
    "fz_free": (None, (vp,)),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

# Entry points that may be missing: a build of an earlier state of the library, named by FUZZYSEARCH_HIP_LIB for an A/B
# run, lacks them.  load_library() passes over an absent one and _entry() refuses the call that needs it; every other
# symbol is mandatory at load time.
OPTIONAL = frozenset((
    "fz_batch_search_multi", "fz_batch_assign", "fz_debug_assign_fold",
    "fz_batch_end_overlaps", "fz_debug_end_overlaps", "fz_debug_overlap_ms",
    "fz_batch_score_cuts", "fz_debug_score_cuts", "fz_debug_cuts_ms",
    "fz_subs_ngrams_multi_cls", "fz_subs_ngrams_multi_best_cls", "fz_batch_search_multi_cls", "fz_batch_assign_cls",
    "fz_debug_multi_plan_cls",
    "fz_batch_upload_records", "fz_batch_tables", "fz_debug_batch_bytes", "fz_debug_records_split", "fz_debug_scan_items",
    "fz_debug_records_ms",
    "fz_batch_upload_fasta", "fz_batch_fasta_index", "fz_debug_fasta_split", "fz_debug_fasta_upper4", "fz_debug_fasta_src",
    "fz_batch_derive", "fz_debug_derive_plan", "fz_debug_derive_ms",
    "fz_batch_upload_records_lines", "fz_batch_format", "fz_debug_format_plan", "fz_debug_format_ms",
    "fz_debug_scan_plan", "fz_mem_info", "fz_debug_scan_instance",
    "fz_debug_scan_walk", "fz_debug_scan_direction", "fz_set_scan_direction",
))

_lib = None
_lib_lock = threading.Lock()


def load_library():
    """Load libfzhip.so and declare the C-ABI (PROTOTYPES).  Raises HipEngineError if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipEngineError(
                "fuzzysearch_amd: %s is missing. Build it with `python -m fuzzysearch_amd.build` "
                "(hipcc, --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            if name in OPTIONAL and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.fz_abi_version() != 1:
            raise HipEngineError("libfzhip.so ABI version mismatch")
        _lib = L
        return L


class UnsupportedSearch(NotImplementedError):
    """The search is outside what the GPU engine supports: a subsequence of more than 65 535 items, a Levenshtein
    budget above 1 023, a generic search (separate limits) or a linear-programming route with max_l_dist above 255,
    more than 255 distinct symbols in a subsequence that is neither bytes nor latin-1 text, automaton candidate sets
    beyond 2^18 entries.  Nothing was searched and there is no CPU fallback: a caller that needs such a search
    catches this and routes it to the reference implementation."""


def _entry(lib, name):
    """Entry point `name` of the loaded library.  A build without it (OPTIONAL) cannot make the call: there is no fallback."""
    fn = getattr(lib, name, None)
    if fn is None:
        raise UnsupportedSearch("this libfzhip.so has no %s: it was built before that entry point existed" % name)
    return fn


def _raise(rc):
    msg = (load_library().fz_last_error() or b"").decode("utf-8", "replace")
    if rc == FZ_EINVAL:
        raise ValueError(msg)
    if rc == FZ_ENOMEM:
        raise MemoryError(msg)
    if rc == FZ_EUNSUPPORTED:
        raise UnsupportedSearch(msg)
    if rc == FZ_ETIMEOUT:
        raise CollectiveTimeout("libfzhip error %d: %s" % (rc, msg))
    raise HipEngineError("libfzhip error %d: %s" % (rc, msg))


def _check(rc):
    if rc != FZ_OK:
        _raise(rc)


def _buffer_address(data):
    """-> (address, nbytes, keepalive) of a C-contiguous 1-byte-item buffer, zero-copy where the
    buffer protocol allows (bytes, bytearray, memoryview, numpy uint8 ...).  Same acceptance rule
    as the reference's is_simple_buffer (_c_ext_base.h:27-34)."""
    mv = memoryview(data)
    if mv.itemsize != 1 or mv.ndim != 1 or not mv.c_contiguous:
        raise TypeError("only contiguous sequences of single-byte values are supported")
    n = mv.nbytes
    if n == 0:
        return None, 0, mv
    if mv.readonly:
        # ctypes cannot wrap a read-only buffer without a copy unless it is a bytes object
        obj = mv.obj
        if isinstance(obj, bytes):
            return ctypes.cast(ctypes.c_char_p(obj), ctypes.c_void_p).value + _mv_offset(mv, obj), n, (mv, obj)
        import numpy as np
        arr = np.frombuffer(mv, dtype=np.uint8)
        return arr.ctypes.data, n, (mv, arr)
    c = (ctypes.c_char * n).from_buffer(mv)
    return ctypes.addressof(c), n, (mv, c)


def _mv_offset(mv, obj):
    # offset of a memoryview slice into its bytes object (memoryview(b)[a:b])
    if len(mv) == len(obj):
        return 0
    import numpy as np
    base = np.frombuffer(obj, dtype=np.uint8).ctypes.data
    return np.frombuffer(mv, dtype=np.uint8).ctypes.data - base


def matches_to_array(raw):
    """(start, end, dist[, block]) rows, or an fz_match structured array -> (address-able buffer, n)."""
    import numpy as np
    if isinstance(raw, np.ndarray) and raw.dtype == _match_dtype():
        arr = np.ascontiguousarray(raw)
        return arr, len(arr)
    n = len(raw)
    arr = np.empty(n, dtype=_match_dtype())
    if n:
        rows = np.asarray([tuple(r[:3]) for r in raw], dtype=np.int64).reshape(n, 3)
        arr["start"], arr["end"], arr["dist"] = rows[:, 0], rows[:, 1], rows[:, 2]
        arr["block"] = [r[3] if len(r) > 3 else -1 for r in raw]
    return arr, n


_MATCH_DTYPE = None


def _match_dtype():
    global _MATCH_DTYPE
    if _MATCH_DTYPE is None:
        import numpy as np
        _MATCH_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("dist", "<i4"), ("block", "<i4")])
    return _MATCH_DTYPE


class _ResultBuffer(object):
    """Owner of a C-ABI result buffer that a numpy array views in place; fz_free when the last view is gone."""
    __slots__ = ('_lib', '_addr')

    def __init__(self, lib, addr):
        self._lib, self._addr = lib, addr

    def __del__(self):
        lib, addr = self._lib, self._addr
        self._addr = None
        if addr and lib is not None:
            try:
                lib.fz_free(ctypes.c_void_p(addr))
            except Exception:                                   # interpreter shutdown
                pass


def _take_rows(lib, addr, n, dtype=None):
    """A result buffer of the library (its address or a ctypes pointer; n rows of `dtype`, None: fz_match rows) -> numpy
    structured array.  Small results: one memcpy, then the C buffer is freed.  Large ones (>= 256 KiB: e.g. the 2.1e5 rows
    of a generic search over 1 GiB of text) are viewed in place — no second 5 MB buffer to fault in and fill — and handed
    back to the library (which recycles such buffers) when the last view dies."""
    import numpy as np
    if dtype is None:
        dtype = _match_dtype()
    nbytes = n * dtype.itemsize
    if nbytes >= (256 << 10):
        addr = ctypes.cast(addr, ctypes.c_void_p).value
        raw = (ctypes.c_char * nbytes).from_address(addr)
        raw._owner = _ResultBuffer(lib, addr)                   # lives as long as the ctypes view numpy holds on to
        return np.frombuffer(raw, dtype=dtype, count=n)
    arr = np.empty(n, dtype=dtype)
    if n:
        ctypes.memmove(arr.ctypes.data, addr, nbytes)
    lib.fz_free(addr)
    return arr


def _take_matches_array(L, ptr, n):
    """-> numpy structured array (start, end, dist, block) over or from the library's buffer (_take_rows)."""
    return _take_rows(L, ptr, n)


def _take_matches(L, ptr, n):
    return _take_rows(L, ptr, n).tolist()


def _take_copy(lib, ptr, n, dtype):
    """The library's buffer of n plain items -> a numpy array of its own; the buffer is freed."""
    import numpy as np
    arr = np.empty(n, dtype=dtype)
    if n:
        ctypes.memmove(arr.ctypes.data, ptr, n * arr.itemsize)
    lib.fz_free(ptr)
    return arr


def _take_bounds(lib, optr, n_pats):
    """The library's per-pattern row offsets (n_pats + 1 entries) -> a list; the buffer is freed."""
    bounds = optr[:n_pats + 1]
    lib.fz_free(optr)
    return bounds


def _struct_dict(s):
    return {name: getattr(s, name) for name, _ in s._fields_}


def _array_call(name, raw):
    L = load_library()
    arr, n = matches_to_array(raw)
    ptr, cnt = mp(), u64(0)
    _check(getattr(L, name)(ctypes.cast(arr.ctypes.data, mp), n, ctypes.byref(ptr), ctypes.byref(cnt)))
    return _take_rows(L, ptr, cnt.value)


def consolidate_array(raw):
    """consolidate_overlapping_matches (common.py:185-189) on an fz_match array (or rows) -> fz_match array;
    no per-record Python work."""
    return _array_call("fz_consolidate", raw)


def group_best_array(raw):
    """[get_best_match_in_group(g) for g in group_matches(ms)] in group-list order
    (substitutions_only.py:279-282) on an fz_match array (or rows) -> fz_match array."""
    return _array_call("fz_group_best", raw)


def consolidate(raw):
    """consolidate_overlapping_matches on (start, end, dist[, block]) tuples -> list of tuples."""
    return consolidate_array(raw).tolist()


def group_best(raw):
    return group_best_array(raw).tolist()


def pack_patterns(patterns):
    """Byte patterns -> (the patterns back to back, uint64 offsets array of len + 1 entries) as fz_lev_ngrams_multi takes them."""
    parts = [bytes(memoryview(p)) if not isinstance(p, bytes) else p for p in patterns]
    offs = (ctypes.c_uint64 * (len(parts) + 1))()
    at = 0
    for i, p in enumerate(parts):
        offs[i] = at
        at += len(p)
    offs[len(parts)] = at
    return b"".join(parts) or b"\0", offs


MODE_EXACT, MODE_LEV, MODE_SUBS = 0, 1, 2          # fz_batch_search's mode (FzMode of csrc/fz_device.h)


def multi_plan(patterns, k, mode=MODE_LEV):
    """fz_debug_multi_plan_mode (no device): -> (group of every pattern, None = the single-pattern route; number of groups)
    for the Levenshtein (MODE_LEV) or the substitutions-only (MODE_SUBS) multi-pattern search."""
    L = load_library()
    blob, offs = pack_patterns(patterns)
    n = len(patterns)
    group_of = (ctypes.c_uint32 * max(1, n))()
    ng = ctypes.c_uint32(0)
    _check(L.fz_debug_multi_plan_mode(mode, blob, offs, n, k, group_of, ctypes.byref(ng)))
    return [None if group_of[i] == 0xffffffff else group_of[i] for i in range(n)], ng.value


def multi_plan_classes(patterns, k, tables):
    """fz_debug_multi_plan_cls (no device): -> (group of every pattern, table entries of every pattern, entries of every
    group) of a class call with tables = (pmask, tmask), two bytes objects of 256.  Raises what the class calls raise."""
    L = load_library()
    blob, offs = pack_patterns(patterns)
    n = len(patterns)
    group_of, per_pat, per_group = ((ctypes.c_uint32 * max(1, n))() for _ in range(3))
    ng = ctypes.c_uint32(0)
    _check(_entry(L, "fz_debug_multi_plan_cls")(blob, offs, n, k, tables[0], tables[1], group_of, ctypes.byref(ng), per_pat, per_group))
    return list(group_of[:n]), list(per_pat[:n]), list(per_group[:ng.value])


def _class_tables(mode, tables):
    """-> (pmask, tmask) of a class call; the class entry points take no mode because they count mismatches only."""
    if mode != MODE_SUBS:
        raise ValueError("symbol classes are searched in substitutions mode (MODE_SUBS) only")
    return tables[0], tables[1]


def batch_segment(offs, idx):
    """fz_debug_batch_segment (no device): -> (sequence number, start, end) of position idx of a batch whose sequences
    lie at offs[j] .. offs[j + 1].  `offs`: a C-contiguous numpy uint64 array (kept by the caller across calls)."""
    L = load_library()
    j, sa, se = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(L.fz_debug_batch_segment(offs.ctypes.data_as(u64p), len(offs) - 1, idx,
                                    ctypes.byref(j), ctypes.byref(sa), ctypes.byref(se)))
    return j.value, sa.value, se.value


_ASSIGN_DTYPE = None


REC_FASTQ_CHECKS = 1                              # FZ_REC_FASTQ_CHECKS
# format -> (lines per record, the sequence's line, flags) of fz_batch_upload_records
RECORD_FORMATS = {'fastq': (4, 1, REC_FASTQ_CHECKS), 'lines': (1, 0, 0)}


def scan_items():
    """fz_debug_scan_items: the items one workgroup of the device's exclusive scan handles."""
    return int(_entry(load_library(), 'fz_debug_scan_items')())


def records_split(text, lines_per_record, sequence_line, flags):
    """fz_debug_records_split (no device): the split of fz_batch_upload_records on the host, through the functions its
    kernels run -> (src_starts, ends, packed bytes, info dict).  A malformed text raises ValueError as the upload does;
    the exception carries the info dict as ``.info``."""
    import numpy as np
    return _split_twin('fz_debug_records_split', text, (lines_per_record, sequence_line, flags), np.dtype(np.uint64))


FA_UPPER = 1                                      # FZ_FA_UPPER
_FASTA_DTYPE = None


def fasta_dtype():
    """The numpy dtype of an fz_fasta_row (include/fzhip.h)."""
    global _FASTA_DTYPE
    if _FASTA_DTYPE is None:
        import numpy as np
        _FASTA_DTYPE = np.dtype([(name, "<u8") for name in ("header_start", "header_len", "length", "offset", "linebases", "linewidth")])
    return _FASTA_DTYPE


def fasta_split(text, flags=0):
    """fz_debug_fasta_split (no device): the split of fz_batch_upload_fasta on the host, through the functions its kernels run
    -> (rows: structured array of fasta_dtype(), ends, packed bytes, info dict).  A malformed text raises ValueError as the
    upload does; the exception carries the info dict as ``.info``."""
    return _split_twin('fz_debug_fasta_split', text, (flags,), fasta_dtype())


def fasta_upper4(w):
    """fz_debug_fasta_upper4: the gather's fold of four bytes (a 32-bit word)."""
    return int(_entry(load_library(), 'fz_debug_fasta_upper4')(w))


def fasta_src(offset, linebases, linewidth, q):
    """fz_debug_fasta_src: where base q of a record with that offset, linebases and linewidth lies in the text."""
    return int(_entry(load_library(), 'fz_debug_fasta_src')(offset, linebases, linewidth, q))


def _split_twin(entry, text, args, row_dtype):
    """One host twin of a text upload: entry(text, n, *args, &rows, &ends, &packed, &info) -> (rows of row_dtype, ends,
    packed bytes, info dict), the library's arrays copied and freed."""
    import numpy as np
    L = load_library()
    addr, n, keep = _buffer_address(text)
    pr, pe, pp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    info = FzRecordsInfo()
    rc = _entry(L, entry)(addr, n, *args, ctypes.byref(pr), ctypes.byref(pe), ctypes.byref(pp), ctypes.byref(info))
    del keep
    d = _struct_dict(info)
    if rc != FZ_OK:
        _raise_records(rc, d)
    ns = d['n_seqs']
    rows = np.frombuffer(ctypes.string_at(pr, ns * row_dtype.itemsize), dtype=row_dtype).copy()
    ends = np.frombuffer(ctypes.string_at(pe, ns * 8), dtype=np.uint64).copy()
    packed = ctypes.string_at(pp, d['packed_bytes'])
    for p in (pr, pe, pp):
        L.fz_free(p)
    return rows, ends, packed, d


def _raise_records(rc, info):
    try:
        _raise(rc)
    except ValueError as e:
        e.info = info
        raise


DERIVE_REVERSE = 1                                # FZ_DERIVE_REVERSE


def _raise_derive(rc, info):
    """A bad item raises as Python's own indexing would: reason 1 (no such sequence) IndexError, 2 and 3 ValueError; the
    info dict rides on the exception as ``.info``."""
    try:
        _raise(rc)
    except ValueError as e:
        if info['bad_reason'] == 1:
            e = IndexError(str(e))
        e.info = info
        raise e


def _derive_tables(index, starts, ends, n_out):
    """The three optional tables as contiguous arrays of the C-ABI's types -> (arrays, their addresses or None)."""
    import numpy as np
    arrs = [None if t is None else np.ascontiguousarray(t, dtype=dt) for t, dt in ((index, np.uint32), (starts, np.uint64), (ends, np.uint64))]
    for a in arrs:
        if a is not None and a.shape != (n_out,):
            raise ValueError('a table of %d entries for %d outputs' % (a.size, n_out))
    return arrs, [None if a is None else a.ctypes.data for a in arrs]


def derive_plan(offs, index, starts, ends, n_out):
    """fz_debug_derive_plan (no device): the measure step and the scan of fz_batch_derive on the host, through the function
    its kernel runs.  offs: the parent's len + 1 offsets -> (src, at, info dict); a bad item raises as derive does."""
    import numpy as np
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    keep, addrs = _derive_tables(index, starts, ends, n_out)
    src = np.zeros(n_out, dtype=np.uint64)
    at = np.zeros(n_out + 1, dtype=np.uint64)
    info = FzDeriveInfo()
    rc = _entry(load_library(), 'fz_debug_derive_plan')(offs.ctypes.data, len(offs) - 1, addrs[0], addrs[1], addrs[2], n_out,
                                                        src.ctypes.data, at.ctypes.data, ctypes.byref(info))
    del keep
    d = _struct_dict(info)
    if rc != FZ_OK:
        _raise_derive(rc, d)
    return src, at, d


FORMAT_MAX_COLUMNS, FORMAT_MAX_LITERAL, FORMAT_NO_CHECK = 8, 255, 0xffffffff     # FZ_FORMAT_*
# preset -> (the C + 1 literals, the pair of columns whose sequences must be of one length in every record or None)
FORMAT_PRESETS = {'lines': ((b'', b'\n'), None),
                  'fastq': ((b'', b'\n', b'\n+\n', b'\n'), (1, 2)),
                  'fasta': ((b'>', b'\n', b'\n'), None)}


def _raise_format(rc, info):
    try:
        _raise(rc)
    except ValueError as e:
        e.info = info
        raise


def _format_literals(literals, equal):
    """-> (the literals back to back, their uint32 lengths, equal_a, equal_b) as fz_batch_format takes them."""
    import numpy as np
    lens = np.array([len(l) for l in literals], dtype=np.uint32)
    a, b = (FORMAT_NO_CHECK, FORMAT_NO_CHECK) if equal is None else equal
    return b''.join(literals) or b'\0', lens, a, b


def format_plan(offs, literal_lens, equal=None):
    """fz_debug_format_plan (no device): the measure step and the scan of fz_batch_format on the host, through the function
    its kernel runs.  offs: per column its len + 1 offsets (the same array twice: a column twice) -> (at, info dict); a bad
    record raises ValueError as format_batch does."""
    import numpy as np
    cols, seen = [], {}
    for o in offs:
        if id(o) not in seen:
            seen[id(o)] = np.ascontiguousarray(o, dtype=np.uint64)
        cols.append(seen[id(o)])
    n = len(cols[0]) - 1 if cols else 0
    for c in cols:
        if len(c) != n + 1:
            raise ValueError('the columns have different numbers of sequences')
    ptrs = (ctypes.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
    lens = np.ascontiguousarray(literal_lens, dtype=np.uint32)
    if len(lens) != len(cols) + 1:
        raise ValueError('%d literals for %d columns' % (len(lens), len(cols)))
    a, b = (FORMAT_NO_CHECK, FORMAT_NO_CHECK) if equal is None else equal
    at = np.zeros(n + 1, dtype=np.uint64)
    info = FzFormatInfo()
    rc = _entry(load_library(), 'fz_debug_format_plan')(ptrs, len(cols), n, lens.ctypes.data, a, b, at.ctypes.data, ctypes.byref(info))
    d = _struct_dict(info)
    if rc != FZ_OK:
        _raise_format(rc, d)
    return at, d


def assign_dtype():
    """The numpy dtype of an fz_assign row (include/fzhip.h): pattern (-1: nothing matched), dist, tied, start, end."""
    global _ASSIGN_DTYPE
    if _ASSIGN_DTYPE is None:
        import numpy as np
        _ASSIGN_DTYPE = np.dtype([("pattern", "<i4"), ("dist", "<u2"), ("tied", "<u2"), ("start", "<u4"), ("end", "<u4")])
    return _ASSIGN_DTYPE


def _take_assign_array(L, addr, n):
    """-> numpy structured array of fz_assign rows over or from the library's buffer (_take_rows)."""
    return _take_rows(L, addr, n, assign_dtype())


def assign_fold(offs, recs, L, pat_table, pat_m, k):
    """fz_debug_assign_fold (no device): the fold of fz_batch_assign on the host, through the functions its kernels run.
    offs: numpy uint64 offsets (n_seqs + 1); recs: numpy array of 24-byte records (u64 key, u32 l, r, dist, aux);
    pat_table: numpy uint32 array of shape (n, 2) = {pattern index, m} per aux; pat_m: the patterns' lengths.
    -> fz_assign structured array of n_seqs rows."""
    import numpy as np
    lib = load_library()
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    recs = np.ascontiguousarray(recs)
    assert recs.dtype.itemsize == 24
    pat_table = np.ascontiguousarray(pat_table, dtype=np.uint32).reshape(-1, 2)
    pat_m = np.ascontiguousarray(pat_m, dtype=np.uint32)
    out = np.empty(len(offs) - 1, dtype=assign_dtype())
    _check(_entry(lib, 'fz_debug_assign_fold')(offs.ctypes.data, len(offs) - 1, recs.ctypes.data, len(recs), L, pat_table.ctypes.data,
                                               len(pat_table), pat_m.ctypes.data, len(pat_m), k, out.ctypes.data))
    return out


_OVERLAP_DTYPE = None


def overlap_dtype():
    """The numpy dtype of an fz_overlap row (include/fzhip.h): start, pattern (0xffff: none, then start = the length), overlap, dist."""
    global _OVERLAP_DTYPE
    if _OVERLAP_DTYPE is None:
        import numpy as np
        _OVERLAP_DTYPE = np.dtype([("start", "<u4"), ("pattern", "<u2"), ("overlap", "u1"), ("dist", "u1")])
    return _OVERLAP_DTYPE


def end_overlaps_twin(mode, patterns, k, min_overlap, blob, offs):
    """fz_debug_end_overlaps (no device): fz_batch_end_overlaps on the host, through the functions its kernels' lanes run and
    with its refusals.  blob: the packed sequences; offs: their n_seqs + 1 offsets -> fz_overlap structured array of n_seqs rows."""
    import numpy as np
    lib = load_library()
    pats, poffs = pack_patterns(list(patterns))
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    blob = bytes(blob)
    out = np.empty(len(offs) - 1, dtype=overlap_dtype())
    _check(_entry(lib, 'fz_debug_end_overlaps')(mode, pats, poffs, len(patterns), k, min_overlap, blob, offs[1:].ctypes.data, len(offs) - 1,
                                                out.ctypes.data))
    return out


CUT_STOP3, CUT_STOP5, CUT_RATE = 1, 2, 4          # fz_batch_score_cuts' flags (include/fzhip.h: FZ_CUT_*)
_CUT_DTYPE = None


def cut_dtype():
    """The numpy dtype of an fz_cut row (include/fzhip.h): start, end."""
    global _CUT_DTYPE
    if _CUT_DTYPE is None:
        import numpy as np
        _CUT_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4")])
    return _CUT_DTYPE


def _cut_table(w):
    """A table of 256 scores, or None -> (a contiguous int16 array that stays alive over the call or None, its address or None)"""
    if w is None:
        return None, None
    import numpy as np
    w = np.ascontiguousarray(w, dtype=np.int16)
    if w.shape != (256,):
        raise ValueError("a score table has 256 entries")
    return w, w.ctypes.data


def score_cuts_twin(w3, w5, flags, rate_num, rate_den, blob, offs):
    """fz_debug_score_cuts (no device): fz_batch_score_cuts on the host, through the functions its kernel's lanes run and with
    its refusals.  w3 / w5: 256 int16 scores or None; blob: the packed sequences; offs: their n_seqs + 1 offsets -> fz_cut
    structured array of n_seqs rows."""
    import numpy as np
    lib = load_library()
    w3, a3 = _cut_table(w3)
    w5, a5 = _cut_table(w5)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    blob = bytes(blob)
    out = np.empty(len(offs) - 1, dtype=cut_dtype())
    _check(_entry(lib, 'fz_debug_score_cuts')(a3, a5, flags, rate_num, rate_den, blob, offs[1:].ctypes.data, len(offs) - 1, out.ctypes.data))
    return out


class OwnedRows(object):
    """A C-ABI result buffer (fz_match rows) that has not been copied anywhere: address, n, and fz_free on release."""
    __slots__ = ('_lib', '_ptr', 'n')

    def __init__(self, lib, ptr, n):
        self._lib, self._ptr, self.n = lib, ptr, n

    @property
    def address(self):
        return ctypes.cast(self._ptr, ctypes.c_void_p).value or 0

    def to_array(self):
        ptr, self._ptr = self._ptr, None
        return _take_matches_array(self._lib, ptr, self.n)

    def release(self):
        ptr, self._ptr = self._ptr, None
        if ptr is not None:
            self._lib.fz_free(ptr)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class FileStream(object):
    """fz_stream: the chunks of a file searched in batches (include/fzhip.h)."""

    def __init__(self, engine, mode, pattern, limits, k, seg_stride, seg_pre, seg_post, batch_bytes):
        self.engine = engine
        self._lib = engine._lib
        self._h = None
        paddr, m, keep = _buffer_address(pattern)
        h = ctypes.c_void_p()
        ms, mi, md = limits
        with engine._lock:
            _check(self._lib.fz_stream_open(engine._h, mode, paddr, m, ms, mi, md, k, seg_stride, seg_pre, seg_post,
                                            batch_bytes, ctypes.byref(h)))
        del keep
        self._h = h

    def buffer(self):
        """-> writable memoryview of the free part of the current pinned staging buffer."""
        ptr = ctypes.c_void_p()
        cap = ctypes.c_uint64(0)
        _check(self._lib.fz_stream_buffer(self._h, ctypes.byref(ptr), ctypes.byref(cap)))
        if cap.value == 0:
            return memoryview(bytearray(0))
        return memoryview((ctypes.c_char * cap.value).from_address(ptr.value)).cast('B')

    def submit(self, nbytes, last=False):
        with self.engine._lock:
            _check(self._lib.fz_stream_submit(self._h, nbytes, 1 if last else 0))

    def read_fd(self, fd, offset, threads=0):
        total = ctypes.c_uint64(0)
        with self.engine._lock:
            _check(self._lib.fz_stream_read_fd(self._h, fd, offset, threads, ctypes.byref(total)))
        return total.value

    def finish(self):
        """-> (fz_match structured array in the reference's order, uint32 chunk number per record)."""
        ptr, seg, cnt = mp(), u32p(), u64(0)
        with self.engine._lock:
            _check(self._lib.fz_stream_finish(self._h, ctypes.byref(ptr), ctypes.byref(seg), ctypes.byref(cnt)))
        segs = _take_copy(self._lib, seg, cnt.value, 'uint32')
        return _take_matches_array(self._lib, ptr, cnt.value), segs

    def close(self):
        with self.engine._lock:                    # the engine may be closed (fz_destroy) by another thread: test under the lock
            if self._h is not None and self.engine._h is not None:
                self._lib.fz_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentSequence(object):
    """A sequence resident in HBM (fz_seq).  Keeps the engine alive; release() or GC frees it."""

    def __init__(self, engine, handle, nbytes):
        self.engine = engine
        self._h = handle
        self.nbytes = nbytes

    def __len__(self):
        return self.nbytes

    def release(self):
        with self.engine._lock:                    # fz_destroy frees live sequences: test the engine under its lock
            if self._h is not None and self.engine._h is not None:
                self.engine._lib.fz_seq_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Engine(object):
    """One fz_ctx: HIP streams, hit/record buffers and the resident sequences of one host thread."""

    def __init__(self, devices=None):
        self._lib = load_library()
        self._h = None
        h = ctypes.c_void_p()
        if devices:
            ids = (ctypes.c_int * len(devices))(*devices)
            rc = self._lib.fz_create(ids, len(devices), ctypes.byref(h))
        else:
            rc = self._lib.fz_create(None, 0, ctypes.byref(h))
        _check(rc)
        self._h = h
        self.devices = list(devices) if devices else [0]
        # a fz_ctx is not internally locked and ctypes drops the GIL during calls: serialise per engine
        # re-entrant: the cyclic GC may finalize a ResidentSequence (-> release()) on a thread that already holds it
        self._lock = threading.RLock()
        self._st = FzStats()
        self._st_ref = ctypes.byref(self._st)

    def close(self):
        """Destroy the context.  Sequences that are still resident are freed with it (fz_destroy); their
        ResidentSequence handles become inert (release() checks the engine)."""
        if self._h is not None:
            with self._lock:
                self._lib.fz_destroy(self._h)
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- residency ---------------------------------------------------------------------------
    def upload(self, data):
        addr, n, keep = _buffer_address(data)
        h = ctypes.c_void_p()
        with self._lock:
            _check(self._lib.fz_seq_upload(self._h, addr, n, ctypes.byref(h)))
        del keep
        return ResidentSequence(self, h, n)

    def upload_batch(self, data, offs):
        """fz_batch_upload: `data` = the sequences back to back (bytes-like), `offs` = numpy uint64 array of their
        len + 1 offsets.  -> a ResidentSequence that only batch_search accepts."""
        import numpy as np
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        addr, n, keep = _buffer_address(data)
        h = ctypes.c_void_p()
        with self._lock:
            _check(self._lib.fz_batch_upload(self._h, addr, offs.ctypes.data_as(u64p),
                                             len(offs) - 1, ctypes.byref(h)))
        del keep
        seq = ResidentSequence(self, h, n)
        seq.n_seqs = len(offs) - 1
        return seq

    def upload_records(self, text, lines_per_record=4, sequence_line=1, flags=REC_FASTQ_CHECKS):
        """fz_batch_upload_records: `text` (bytes-like: a FASTQ file, a file of lines) is copied to the device once and split
        there into a batch -> a ResidentSequence like upload_batch's, with `.n_seqs` and `.info` (n_lines, n_seqs,
        packed_bytes).  A malformed text raises ValueError naming the record (`.info` on the exception: bad_record, bad_reason)."""
        return self._upload_text(_entry(self._lib, 'fz_batch_upload_records'), text, lines_per_record, sequence_line, flags)

    def upload_fasta(self, text, flags=0):
        """fz_batch_upload_fasta: `text` (bytes-like: a FASTA file) is copied to the device once and split there into a batch of
        its contigs -> a ResidentSequence like upload_records'.  A malformed text raises ValueError naming the record."""
        return self._upload_text(_entry(self._lib, 'fz_batch_upload_fasta'), text, flags)

    def _upload_text(self, entry, text, *args):
        """entry(ctx, text, n, *args, &handle, &info) -> the batch handle with `.n_seqs` and `.info`; a refusal raises with
        the info dict as `.info`."""
        addr, n, keep = _buffer_address(text)
        h = ctypes.c_void_p()
        info = FzRecordsInfo()
        with self._lock:
            rc = entry(self._h, addr, n, *args, ctypes.byref(h), ctypes.byref(info))
        del keep
        d = _struct_dict(info)
        if rc != FZ_OK:
            _raise_records(rc, d)
        seq = ResidentSequence(self, h, d['packed_bytes'])
        seq.n_seqs = d['n_seqs']
        seq.info = d
        return seq

    def fasta_index(self, batch):
        """fz_batch_fasta_index -> the rows of an upload_fasta handle: a structured array of fasta_dtype()."""
        import numpy as np
        rows = np.zeros(batch.n_seqs, dtype=fasta_dtype())
        with self._lock:
            _check(_entry(self._lib, 'fz_batch_fasta_index')(batch._h, rows.ctypes.data))
        return rows

    def batch_tables(self, batch):
        """fz_batch_tables -> (src_starts, ends): numpy uint64 arrays of the batch's n_seqs sequences — where each one starts
        in the text it was cut from (upload_batch: its offset in the packed bytes) and where it ends in the packed bytes."""
        import numpy as np
        starts = np.zeros(batch.n_seqs, dtype=np.uint64)
        ends = np.zeros(batch.n_seqs, dtype=np.uint64)
        with self._lock:
            _check(_entry(self._lib, 'fz_batch_tables')(batch._h, starts.ctypes.data, ends.ctypes.data))
        return starts, ends

    def batch_bytes(self, batch):
        """fz_debug_batch_bytes: the packed bytes of a batch handle, back from the device."""
        buf = ctypes.create_string_buffer(max(1, batch.nbytes))
        with self._lock:
            _check(_entry(self._lib, 'fz_debug_batch_bytes')(batch._h, buf, batch.nbytes))
        return buf.raw[:batch.nbytes]

    def derive_batch(self, batch, index=None, starts=None, ends=None, n_out=None, reverse=False, translate=None):
        """fz_batch_derive: out[j] = X(batch[index[j]][starts[j]:ends[j]]) made on the device from a batch handle of this
        engine -> a ResidentSequence like upload_records', with `.n_seqs` and `.info` (n_out, packed_bytes, longest).
        index: uint32, starts / ends: uint64 arrays of n_out entries, or None for the defaults; translate: 256 bytes or None.
        A bad item raises IndexError (no such sequence) or ValueError naming it (`.info`: bad_item, bad_reason)."""
        if getattr(batch, '_h', None) is None or getattr(batch, 'n_seqs', None) is None:
            raise ValueError('derive_batch takes a batch handle that has not been released')
        if n_out is None:
            n_out = batch.n_seqs if index is None else len(index)
        keep, addrs = _derive_tables(index, starts, ends, n_out)
        taddr = None
        if translate is not None:
            taddr, tn, tkeep = _buffer_address(translate)
            if tn != 256:
                raise ValueError('translate is a table of 256 bytes')
        h = ctypes.c_void_p()
        info = FzDeriveInfo()
        with self._lock:
            rc = _entry(self._lib, 'fz_batch_derive')(self._h, batch._h, addrs[0], addrs[1], addrs[2], n_out,
                                                      DERIVE_REVERSE if reverse else 0, taddr, ctypes.byref(h), ctypes.byref(info))
        del keep
        d = _struct_dict(info)
        if rc != FZ_OK:
            _raise_derive(rc, d)
        seq = ResidentSequence(self, h, d['packed_bytes'])
        seq.n_seqs = d['n_out']
        seq.info = d
        return seq

    def upload_records_lines(self, text, lines_per_record, lines, flags):
        """fz_batch_upload_records_lines: upload_records for several lines of every record from one copy of the text and one
        line table -> a list of batch handles, one per entry of `lines`, each with `.n_seqs` and `.info` (the call's info;
        packed_bytes: the handle's own).  A malformed text raises as upload_records does; no handle is left."""
        import numpy as np
        entry = _entry(self._lib, 'fz_batch_upload_records_lines')
        kept = np.ascontiguousarray(lines, dtype=np.uint32)
        addr, n, keep = _buffer_address(text)
        hs = (ctypes.c_void_p * max(1, len(kept)))()
        info = FzRecordsInfo()
        with self._lock:
            rc = entry(self._h, addr, n, lines_per_record, kept.ctypes.data, len(kept), flags, hs, ctypes.byref(info))
        del keep
        d = _struct_dict(info)
        if rc != FZ_OK:
            _raise_records(rc, d)
        out = []
        for i in range(len(kept)):
            h = ctypes.c_void_p(hs[i])
            seq = ResidentSequence(self, h, int(self._lib.fz_seq_len(h)))
            seq.n_seqs = d['n_seqs']
            seq.info = dict(d, packed_bytes=seq.nbytes)
            out.append(seq)
        return out

    def format_batch(self, columns, literals, equal=None, out=None):
        """fz_batch_format: the text  join_j(lit[0] + col[0][j] + lit[1] + ... + col[C-1][j] + lit[C])  of C batch handles of
        this engine, assembled on the device -> a numpy uint8 array of exactly the text (a view of `out`, a writable
        C-contiguous numpy uint8 array of at least the text's size, when one is given).  equal = (a, b): columns whose
        sequences must be of one length in every record.  A bad record raises ValueError naming it (`.info`: bad_record,
        bad_reason) and leaves `out` as it was."""
        import numpy as np
        entry = _entry(self._lib, 'fz_batch_format')
        columns = list(columns)
        for c in columns:
            if getattr(c, '_h', None) is None or getattr(c, 'n_seqs', None) is None:
                raise ValueError('format_batch takes batch handles that have not been released')
        if len(literals) != len(columns) + 1:
            raise ValueError('%d literals for %d columns' % (len(literals), len(columns)))
        blob, lens, a, b = _format_literals(literals, equal)
        size = sum(c.nbytes for c in columns) + (columns[0].n_seqs if columns else 0) * int(lens.sum())
        if out is None:
            out = np.empty(size, dtype=np.uint8)
        hs = (ctypes.c_void_p * max(1, len(columns)))(*[c._h.value for c in columns])
        info = FzFormatInfo()
        with self._lock:
            rc = entry(self._h, hs, len(columns), blob, lens.ctypes.data, a, b, out.ctypes.data if out.size else None, out.size,
                       ctypes.byref(info))
        d = _struct_dict(info)
        if rc != FZ_OK:
            _raise_format(rc, d)
        return out[:d['text_bytes']]

    def format_ms(self):
        """fz_debug_format_ms: {desc_h2d, measure_scan, gather, text_d2h, call} milliseconds of this engine's last format_batch."""
        ms = (ctypes.c_double * 5)()
        with self._lock:
            _check(_entry(self._lib, 'fz_debug_format_ms')(self._h, ms))
        return {'desc_h2d': ms[0], 'measure_scan': ms[1], 'gather': ms[2], 'text_d2h': ms[3], 'call': ms[4]}

    def derive_ms(self):
        """fz_debug_derive_ms: {tables_h2d, measure_scan, gather, ends_d2h, call} milliseconds of this engine's last derive_batch."""
        ms = (ctypes.c_double * 5)()
        with self._lock:
            _check(_entry(self._lib, 'fz_debug_derive_ms')(self._h, ms))
        return {'tables_h2d': ms[0], 'measure_scan': ms[1], 'gather': ms[2], 'ends_d2h': ms[3], 'call': ms[4]}

    def records_ms(self):
        """fz_debug_records_ms: {h2d, kernels, ends_d2h, call} milliseconds of this engine's last upload_records / upload_fasta."""
        ms = (ctypes.c_double * 4)()
        with self._lock:
            _check(_entry(self._lib, 'fz_debug_records_ms')(self._h, ms))
        return {'h2d': ms[0], 'kernels': ms[1], 'ends_d2h': ms[2], 'call': ms[3]}

    def _batch_call(self, batch, mode, pattern, k, reduced):
        paddr, m, keep = (pattern, len(pattern), None) if type(pattern) is bytes else _buffer_address(pattern)
        ptr, sptr, cnt = mp(), u32p(), u64(0)
        with self._lock:
            _check(self._lib.fz_batch_search(self._h, batch._h, mode, paddr, m, k, 1 if reduced else 0,
                                             ctypes.byref(ptr), ctypes.byref(sptr), ctypes.byref(cnt)))
        return ptr, _take_copy(self._lib, sptr, cnt.value, 'uint32'), cnt.value

    def batch_search(self, batch, mode, pattern, k, reduced=False):
        """fz_batch_search -> (rows, seq_of): an fz_match structured array in the local coordinates of the rows' sequences,
        ordered by sequence, and the uint32 array of their sequence numbers."""
        ptr, seq_of, n = self._batch_call(batch, mode, pattern, k, reduced)
        return _take_matches_array(self._lib, ptr, n), seq_of

    def batch_rows_call(self, batch, mode, pattern, k, reduced=True):
        """The same as (OwnedRows, seq_of array), for callers that build Match objects in C straight from the result buffer."""
        ptr, seq_of, n = self._batch_call(batch, mode, pattern, k, reduced)
        return OwnedRows(self._lib, ptr, n), seq_of

    def _batch_multi_call(self, batch, mode, patterns, k, reduced, tables=None):
        """-> (rows pointer, seq_of array, per-pattern row offsets) of one fz_batch_search_multi call; the caller owns the pointer.
        tables = (pmask, tmask): fz_batch_search_multi_cls, which has no mode and takes the masks in front of `reduced`."""
        blob, offs = pack_patterns(patterns)
        n, red = len(patterns), 1 if reduced else 0
        if tables is None:
            fn, args = _entry(self._lib, "fz_batch_search_multi"), (mode, blob, offs, n, k, red)
        else:
            pmask, tmask = _class_tables(mode, tables)
            fn, args = _entry(self._lib, "fz_batch_search_multi_cls"), (blob, offs, n, k, pmask, tmask, red)
        ptr, sptr, optr = mp(), u32p(), u64p()
        with self._lock:
            _check(fn(self._h, batch._h, *args, ctypes.byref(ptr), ctypes.byref(sptr), ctypes.byref(optr)))
        bounds = _take_bounds(self._lib, optr, n)
        return ptr, _take_copy(self._lib, sptr, bounds[-1], 'uint32'), bounds

    def batch_search_multi(self, batch, mode, patterns, k, reduced=False, tables=None):
        """[batch_search(batch, mode, p, k, reduced) for p in patterns] in as few passes over the batch as the patterns
        allow (fz_batch_search_multi; with tables, under the class distance): a list of (rows, seq_of) per pattern."""
        patterns = list(patterns)
        ptr, seq_of, bounds = self._batch_multi_call(batch, mode, patterns, k, reduced, tables)
        rows = _take_matches_array(self._lib, ptr, bounds[-1])
        return [(rows[bounds[i]:bounds[i + 1]], seq_of[bounds[i]:bounds[i + 1]]) for i in range(len(patterns))]

    def batch_multi_rows_call(self, batch, mode, patterns, k, reduced=True, tables=None):
        """The same as (OwnedRows of all patterns' rows, seq_of array, row offsets per pattern), for callers that build Match
        objects in C straight from the result buffer: P x S lists are not a form for millions of reads."""
        patterns = list(patterns)
        ptr, seq_of, bounds = self._batch_multi_call(batch, mode, patterns, k, reduced, tables)
        return OwnedRows(self._lib, ptr, bounds[-1]), seq_of, bounds

    def batch_assign(self, batch, mode, patterns, k, tables=None):
        """fz_batch_assign: the best pattern of the list per sequence of the batch -> a structured array (assign_dtype) of
        one row per sequence over the library's buffer: pattern (-1: none), dist, tied, start, end (local coordinates).
        tables = (pmask, tmask): fz_batch_assign_cls, the same under the class distance; it has no mode."""
        patterns = list(patterns)
        blob, offs = pack_patterns(patterns)
        if tables is None:
            fn, args = _entry(self._lib, "fz_batch_assign"), (mode, blob, offs, len(patterns), k)
        else:
            pmask, tmask = _class_tables(mode, tables)
            fn, args = _entry(self._lib, "fz_batch_assign_cls"), (blob, offs, len(patterns), k, pmask, tmask)
        ptr = ctypes.c_void_p()
        with self._lock:
            _check(fn(self._h, batch._h, *args, ctypes.byref(ptr)))
        return _take_assign_array(self._lib, ptr.value, batch.n_seqs)     # (a plain handle was refused above)

    def batch_end_overlaps(self, batch, mode, patterns, k, min_overlap):
        """fz_batch_end_overlaps: per sequence of the batch the pattern whose strictly partial prefix ends it -> a structured
        array (overlap_dtype) of one row per sequence over the library's buffer: start, pattern (0xffff: none), overlap, dist."""
        patterns = list(patterns)
        blob, offs = pack_patterns(patterns)
        fn = _entry(self._lib, "fz_batch_end_overlaps")
        ptr = ctypes.c_void_p()
        with self._lock:
            _check(fn(self._h, batch._h, mode, blob, offs, len(patterns), k, min_overlap, ctypes.byref(ptr)))
        return _take_rows(self._lib, ptr.value, batch.n_seqs, overlap_dtype())

    def overlap_ms(self):
        """fz_debug_overlap_ms: {tables_h2d, kernels, rows_d2h, call} milliseconds of this engine's last batch_end_overlaps."""
        ms = (ctypes.c_double * 4)()
        with self._lock:
            _check(_entry(self._lib, 'fz_debug_overlap_ms')(self._h, ms))
        return {'tables_h2d': ms[0], 'kernels': ms[1], 'rows_d2h': ms[2], 'call': ms[3]}

    def batch_score_cuts(self, batch, w3, w5, flags, rate_num=0, rate_den=1):
        """fz_batch_score_cuts: per sequence of the batch where the running sum of the 3' table w3 and / or the 5' table w5 (256
        int16 scores each, or None) peaks -> a structured array (cut_dtype) of one row per sequence over the library's buffer:
        start, end.  flags: CUT_STOP3 | CUT_STOP5 | CUT_RATE."""
        w3, a3 = _cut_table(w3)
        w5, a5 = _cut_table(w5)
        fn = _entry(self._lib, "fz_batch_score_cuts")
        ptr = ctypes.c_void_p()
        with self._lock:
            _check(fn(self._h, batch._h, a3, a5, flags, rate_num, rate_den, ctypes.byref(ptr)))
        return _take_rows(self._lib, ptr.value, batch.n_seqs, cut_dtype())

    def cuts_ms(self):
        """fz_debug_cuts_ms: {tables_h2d, kernels, rows_d2h, call} milliseconds of this engine's last batch_score_cuts."""
        ms = (ctypes.c_double * 4)()
        with self._lock:
            _check(_entry(self._lib, 'fz_debug_cuts_ms')(self._h, ms))
        return {'tables_h2d': ms[0], 'kernels': ms[1], 'rows_d2h': ms[2], 'call': ms[3]}

    # the class calls by their names of old: substitutions mode, tables = (pmask, tmask) of classes.class_tables
    def batch_multi_rows_call_classes(self, batch, patterns, k, tables, reduced=True):
        return self.batch_multi_rows_call(batch, MODE_SUBS, patterns, k, reduced, tables)

    def batch_search_multi_classes(self, batch, patterns, k, tables, reduced=False):
        return self.batch_search_multi(batch, MODE_SUBS, patterns, k, reduced, tables)

    def batch_assign_classes(self, batch, patterns, k, tables):
        return self.batch_assign(batch, MODE_SUBS, patterns, k, tables)

    def upload_shard(self, data, buf_global_off, own_lo, own_hi, global_n):
        addr, n, keep = _buffer_address(data)
        h = ctypes.c_void_p()
        with self._lock:
            _check(self._lib.fz_seq_upload_shard(self._h, addr, n, buf_global_off, own_lo, own_hi,
                                                  global_n, ctypes.byref(h)))
        del keep
        return ResidentSequence(self, h, global_n)

    def new_sequence(self, global_n):
        """An empty sharded sequence of global_n bytes; fill it with add_shard() (one shard per device of the engine)."""
        h = ctypes.c_void_p()
        with self._lock:
            _check(self._lib.fz_seq_new(self._h, global_n, ctypes.byref(h)))
        return ResidentSequence(self, h, global_n)

    def add_shard(self, seq, dev_index, data, buf_global_off, own_lo, own_hi):
        """Upload bytes [buf_global_off, +len(data)) to device number dev_index of this engine; it owns the n-gram
        hits in [own_lo, own_hi) and needs (m + k) halo bytes on both sides (fz_seq_add_shard)."""
        addr, n, keep = _buffer_address(data)
        with self._lock:
            _check(self._lib.fz_seq_add_shard(seq._h, dev_index, addr, n, buf_global_off, own_lo, own_hi))
        del keep

    def device_ms(self):
        """Scan-kernel hipEvent span of the search collected last, one value per device of the engine."""
        n = len(self.devices)
        out = (ctypes.c_double * n)()
        with self._lock:                           # resolves the event spans: mutates the context
            rc = self._lib.fz_device_ms(self._h, out, n)
        if rc < 0:
            _raise(rc)
        return list(out)

    # -- RCCL without PyTorch (fz_comm_*) -----------------------------------------------------
    COMM_ID_BYTES = 128

    def comm_unique_id(self):
        """ncclGetUniqueId -> 128 bytes that rank 0 hands to the other ranks (file, socket, ...)."""
        buf = ctypes.create_string_buffer(self.COMM_ID_BYTES)
        _check(self._lib.fz_comm_unique_id(buf, self.COMM_ID_BYTES))
        return buf.raw

    def comm_init_rank(self, unique_id, world, rank):
        """One process per GPU: this (single-device) engine becomes rank `rank` of `world`.  From now on its
        lev_ngrams / lev_ngrams_begin / _end are COLLECTIVE and deliver the merged stream of all ranks."""
        if len(unique_id) != self.COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % self.COMM_ID_BYTES)
        with self._lock:
            _check(self._lib.fz_comm_init_rank(self._h, ctypes.c_char_p(bytes(unique_id)), world, rank))

    def comm_init_all(self):
        """One process, several GPUs: every device of the engine becomes one rank (ncclCommInitAll)."""
        with self._lock:
            _check(self._lib.fz_comm_init_all(self._h))

    def comm_info(self):
        """-> (world, rank of device 0, collective searches on?); world == 0: no communicator."""
        w, r, c = ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_int(0)
        _check(self._lib.fz_comm_info(self._h, ctypes.byref(w), ctypes.byref(r), ctypes.byref(c)))
        return w.value, r.value, bool(c.value)

    def comm_set_collective(self, on):
        with self._lock:
            _check(self._lib.fz_comm_set_collective(self._h, 1 if on else 0))

    def comm_allgather(self, data):
        """Equal-sized bytes from every rank -> list of bytes in rank order (ncclAllGather through device buffers)."""
        data = bytes(data)
        world = self.comm_info()[0]
        out = ctypes.create_string_buffer(max(1, world * len(data)))
        with self._lock:
            _check(self._lib.fz_comm_allgather(self._h, ctypes.c_char_p(data), len(data), out))
        raw = out.raw
        return [raw[i * len(data):(i + 1) * len(data)] for i in range(world)]

    def comm_max(self, value):
        v = ctypes.c_double(value)
        with self._lock:
            _check(self._lib.fz_comm_max_f64(self._h, ctypes.byref(v)))
        return v.value

    def comm_gather_ms(self):
        """Host milliseconds of the exchange step (all-gather + D2H + parse) of the collective search collected last."""
        v = ctypes.c_double(0.0)
        _check(self._lib.fz_comm_gather_ms(self._h, ctypes.byref(v)))
        return v.value

    @staticmethod
    def comm_backend():
        """'rccl', 'stand-in' (tests/mock_rccl.cpp through FZ_RCCL_LIB) or None when no collective library loads."""
        return {0: None, 1: "rccl", 2: "stand-in"}[load_library().fz_comm_backend()]

    def comm_barrier(self):
        with self._lock:
            _check(self._lib.fz_comm_barrier(self._h))

    def comm_destroy(self):
        with self._lock:
            if self._h is not None:
                self._lib.fz_comm_destroy(self._h)

    # -- searches (raw streams, tuples (start, end, dist, block)) ------------------------------
    def search_exact(self, seq, pattern, lo=0, hi=None, as_array=False):
        """Ascending start indices of every occurrence: a list of ints, or (as_array=True) a numpy int64 array."""
        paddr, m, keep = _buffer_address(pattern)
        ptr, cnt = u64p(), u64(0)
        with self._lock:
            _check(self._lib.fz_search_exact(self._h, seq._h, paddr, m, max(0, lo),
                                             UINT64_MAX if hi is None else max(0, hi),
                                             ctypes.byref(ptr), ctypes.byref(cnt)))
        arr = _take_copy(self._lib, ptr, cnt.value, 'int64')
        return arr if as_array else arr.tolist()

    def rows_call(self, fn, seq, pattern, *ints, take=OwnedRows):
        """One C-ABI search -> take(library, rows pointer, row count).  OwnedRows: the library's result buffer itself, for
        callers that turn the rows into Match objects in C (common.matches_from_rows) — no numpy array, no second copy;
        _take_rows: a structured array; _take_matches: a list of tuples."""
        # (ctypes passes a bytes object as a pointer to its buffer; spelt out per method: a helper would be one more frame
        # in the calls the benchmark times)
        paddr, m, keep = (pattern, len(pattern), None) if type(pattern) is bytes else _buffer_address(pattern)
        ptr = mp()
        cnt = ctypes.c_uint64(0)
        with self._lock:
            _check(fn(self._h, seq._h, paddr, m, *ints, ctypes.byref(ptr), ctypes.byref(cnt)))
        return take(self._lib, ptr, cnt.value)

    def lev_ngrams_consolidated(self, seq, pattern, k, as_array=False):
        """consolidate_overlapping_matches(find_near_matches_levenshtein_ngrams(...)) in one call (fz_lev_ngrams_consolidated)."""
        return self.rows_call(self._lib.fz_lev_ngrams_consolidated, seq, pattern, k, take=_take_rows if as_array else _take_matches)

    def subs_ngrams_best(self, seq, pattern, k, as_array=False):
        """Best match of every overlap group of the substitutions-only n-gram stream, group-list order (fz_subs_ngrams_best)."""
        return self.rows_call(self._lib.fz_subs_ngrams_best, seq, pattern, k, take=_take_rows if as_array else _take_matches)

    def lev_ngrams(self, seq, pattern, k, as_array=False):
        """Raw stream of find_near_matches_levenshtein_ngrams: list of (start, end, dist, block)
        tuples, or a numpy structured array with those fields (as_array=True, no per-record
        Python objects)."""
        return self.rows_call(self._lib.fz_lev_ngrams, seq, pattern, k, take=_take_rows if as_array else _take_matches)

    def _multi_call(self, name, seq, patterns, k, tables=None):
        """One multi-pattern call on a plain sequence -> (rows pointer, per-pattern row offsets); the caller owns the pointer.
        tables = (pmask, tmask): the class form of entry point `name`, `name`_cls, which takes the masks behind k."""
        blob, offs = pack_patterns(patterns)
        if tables is None:
            fn, masks = getattr(self._lib, name), ()
        else:
            fn, masks = _entry(self._lib, name + "_cls"), (tables[0], tables[1])
        ptr, optr = mp(), u64p()
        with self._lock:
            _check(fn(self._h, seq._h, blob, offs, len(patterns), k, *masks, ctypes.byref(ptr), ctypes.byref(optr)))
        return ptr, _take_bounds(self._lib, optr, len(patterns))

    def _multi(self, name, seq, patterns, k, as_array, tables=None):
        patterns = list(patterns)
        ptr, bounds = self._multi_call(name, seq, patterns, k, tables)
        rows = _take_matches_array(self._lib, ptr, bounds[-1])
        out = [rows[bounds[i]:bounds[i + 1]] for i in range(len(patterns))]
        return out if as_array else [r.tolist() for r in out]

    def lev_ngrams_multi(self, seq, patterns, k, as_array=False):
        """[lev_ngrams(seq, p, k) for p in patterns] in as few passes over the sequence as the patterns allow
        (fz_lev_ngrams_multi): a list with one raw stream per pattern, in the shapes lev_ngrams returns."""
        return self._multi("fz_lev_ngrams_multi", seq, patterns, k, as_array)

    def lev_ngrams_multi_consolidated(self, seq, patterns, k, as_array=False):
        """[lev_ngrams_consolidated(seq, p, k) for p in patterns] (fz_lev_ngrams_multi_consolidated)."""
        return self._multi("fz_lev_ngrams_multi_consolidated", seq, patterns, k, as_array)

    def subs_ngrams_multi(self, seq, patterns, k, as_array=False, tables=None):
        """[subs_ngrams(seq, p, k) for p in patterns] in as few passes over the sequence as the patterns allow
        (fz_subs_ngrams_multi): a list with one raw stream per pattern.  tables = (pmask, tmask): under their class distance."""
        return self._multi("fz_subs_ngrams_multi", seq, patterns, k, as_array, tables)

    def subs_ngrams_multi_best(self, seq, patterns, k, as_array=False, tables=None):
        """[subs_ngrams_best(seq, p, k) for p in patterns] (fz_subs_ngrams_multi_best)."""
        return self._multi("fz_subs_ngrams_multi_best", seq, patterns, k, as_array, tables)

    def multi_rows_call(self, seq, patterns, k, mode=MODE_LEV, tables=None):
        """fz_lev_ngrams_multi_consolidated (MODE_LEV) or fz_subs_ngrams_multi_best (MODE_SUBS; with tables, its class form)
        -> (OwnedRows of all patterns' rows, row offsets per pattern), for callers that build Match objects in C straight
        from the result buffer."""
        patterns = list(patterns)
        name = "fz_subs_ngrams_multi_best" if mode == MODE_SUBS else "fz_lev_ngrams_multi_consolidated"
        ptr, bounds = self._multi_call(name, seq, patterns, k, tables)
        return OwnedRows(self._lib, ptr, bounds[-1]), bounds

    # the class calls by their names of old: tables = (pmask, tmask) of classes.class_tables
    def subs_ngrams_multi_classes(self, seq, patterns, k, tables, best=False, as_array=False):
        return (self.subs_ngrams_multi_best if best else self.subs_ngrams_multi)(seq, patterns, k, as_array, tables)

    def multi_rows_call_classes(self, seq, patterns, k, tables):
        return self.multi_rows_call(seq, patterns, k, MODE_SUBS, tables)

    def lev_ngrams_begin(self, seq, pattern, k):
        """Launch lev_ngrams and return; lev_ngrams_end() delivers the result of the OLDEST search in flight.
        Up to two searches may be in flight per engine (the scan of search i + 1 runs while the host orders
        and consumes the records of search i); the host and other streams (a collective, a copy) can work
        meanwhile."""
        paddr, m, keep = (pattern, len(pattern), None) if type(pattern) is bytes else _buffer_address(pattern)
        with self._lock:
            _check(self._lib.fz_lev_ngrams_begin(self._h, seq._h, paddr, m, k))

    def subs_ngrams_begin(self, seq, pattern, k):
        """subs_ngrams launched, not collected: search_end() delivers it (same two-deep pipeline as lev_ngrams_begin)."""
        paddr, m, keep = (pattern, len(pattern), None) if type(pattern) is bytes else _buffer_address(pattern)
        with self._lock:
            _check(self._lib.fz_subs_ngrams_begin(self._h, seq._h, paddr, m, k))

    def generic_ngrams_begin(self, seq, pattern, max_subs, max_ins, max_dels, max_l, consolidated=False):
        """generic_ngrams (or generic_ngrams_consolidated) launched, not collected.  Two generic searches in flight run
        on two lanes: the younger one's scan next to the older one's automaton kernel."""
        paddr, m, keep = (pattern, len(pattern), None) if type(pattern) is bytes else _buffer_address(pattern)
        with self._lock:
            _check(self._lib.fz_generic_ngrams_begin(self._h, seq._h, paddr, m, max_subs, max_ins, max_dels, max_l,
                                                     1 if consolidated else 0))

    def search_end(self, as_array=False):
        """The result of the OLDEST search in flight (lev / subs / generic begin), as its synchronous call returns it."""
        return self.lev_ngrams_end(as_array=as_array)

    def lev_ngrams_end(self, as_array=False):
        ptr = mp()
        cnt = ctypes.c_uint64(0)
        with self._lock:
            _check(self._lib.fz_lev_ngrams_end(self._h, ctypes.byref(ptr), ctypes.byref(cnt)))
        if as_array:
            return _take_rows(self._lib, ptr, cnt.value)
        return _take_matches(self._lib, ptr, cnt.value)

    def subs_ngrams(self, seq, pattern, k, as_array=False):
        return self.rows_call(self._lib.fz_subs_ngrams, seq, pattern, k, take=_take_rows if as_array else _take_matches)

    def generic_ngrams(self, seq, pattern, max_subs, max_ins, max_dels, max_l, as_array=False):
        return self.rows_call(self._lib.fz_generic_ngrams, seq, pattern, max_subs, max_ins, max_dels, max_l,
                              take=_take_rows if as_array else _take_matches)

    def generic_ngrams_consolidated(self, seq, pattern, max_subs, max_ins, max_dels, max_l, as_array=False):
        """consolidate_overlapping_matches(find_near_matches_generic_ngrams(...)) with the first stage of the consolidation
        on the device (fz_generic_ngrams_consolidated): rows (start, end, dist, block) sorted by (start, end, dist)."""
        return self.rows_call(self._lib.fz_generic_ngrams_consolidated, seq, pattern, max_subs, max_ins, max_dels, max_l,
                              take=_take_rows if as_array else _take_matches)

    def lev_lp(self, seq, pattern, k, as_array=False):
        return self.rows_call(self._lib.fz_lev_lp, seq, pattern, k, take=_take_rows if as_array else _take_matches)

    def subs_lp(self, seq, pattern, k, as_array=False):
        return self.rows_call(self._lib.fz_subs_lp, seq, pattern, k, take=_take_rows if as_array else _take_matches)

    def generic_lp(self, seq, pattern, max_subs, max_ins, max_dels, max_l, as_array=False):
        return self.rows_call(self._lib.fz_generic_lp, seq, pattern, max_subs, max_ins, max_dels, max_l,
                              take=_take_rows if as_array else _take_matches)

    def _any_call(self, fn, seq, pattern, *ints):
        paddr, m, keep = _buffer_address(pattern)
        found = ctypes.c_int(0)
        with self._lock:
            _check(fn(self._h, seq._h, paddr, m, *ints, ctypes.byref(found)))
        del keep
        return bool(found.value)

    def subs_ngrams_any(self, seq, pattern, k):
        """has_near_match_substitutions_ngrams: is the raw stream of subs_ngrams non-empty? (flag only, early exit)"""
        return self._any_call(self._lib.fz_subs_ngrams_any, seq, pattern, k)

    def subs_lp_any(self, seq, pattern, k):
        return self._any_call(self._lib.fz_subs_lp_any, seq, pattern, k)

    def generic_ngrams_any(self, seq, pattern, max_subs, max_ins, max_dels, max_l):
        return self._any_call(self._lib.fz_generic_ngrams_any, seq, pattern, max_subs, max_ins, max_dels, max_l)

    def set_timing(self, on):
        """hipEvent timing of the kernels (stats()["filter_ms"] ...): on by default; off saves a few us per call."""
        with self._lock:
            _check(self._lib.fz_set_timing(self._h, 1 if on else 0))

    def set_streams(self, n):
        """2 (default with one device) or 1 stream per device for the two-deep pipeline of fused searches (fz_set_streams)."""
        with self._lock:
            _check(self._lib.fz_set_streams(self._h, n))

    def set_scan_direction(self, mode):
        """0 (default): every whole scan of a resident sequence starts where the last one ended, so directions alternate;
        1: always forward; 2: always reversed (fz_set_scan_direction).  The rows never depend on it."""
        with self._lock:
            _check(_entry(self._lib, "fz_set_scan_direction")(self._h, mode))

    def scan_direction(self, seq=None):
        """(the next eligible scan launch on `seq` would be reversed, reversed launches of this engine so far)
        (fz_debug_scan_direction)."""
        nxt, cnt = ci(0), u64(0)
        with self._lock:
            _check(_entry(self._lib, "fz_debug_scan_direction")(self._h, seq._h if seq is not None else None,
                                                                 ctypes.byref(nxt), ctypes.byref(cnt)))
        return bool(nxt.value), cnt.value

    def stats(self):
        st = FzStats()
        with self._lock:                           # fz_stats resolves the event spans: it mutates the context
            _check(self._lib.fz_stats(self._h, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in FzStats._fields_}

    def mem_info(self):
        """(free, total) device memory in bytes: the minimum over the engine's devices."""
        f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with self._lock:
            _check(_entry(self._lib, 'fz_mem_info')(self._h, ctypes.byref(f), ctypes.byref(t)))
        return f.value, t.value

    def kernel_ms(self):
        """(filter_ms, verify_ms, device_ms) of the last call: the cheap subset of stats()."""
        with self._lock:
            st = self._st
            _check(self._lib.fz_stats(self._h, self._st_ref))
            return st.filter_ms, st.verify_ms, st.device_ms


_default_engine = None
_default_lock = threading.Lock()


def default_engine():
    """Process-wide engine.  FUZZYSEARCH_HIP_DEVICES="0,1,..." selects the devices."""
    global _default_engine
    with _default_lock:
        if _default_engine is None:
            env = os.environ.get("FUZZYSEARCH_HIP_DEVICES", "").strip()
            devices = [int(x) for x in env.split(",") if x.strip()] if env else None
            _default_engine = Engine(devices)
        return _default_engine
