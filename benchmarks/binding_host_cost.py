"""CPU-only: the Python frames of the binding's timed methods (what bench.py calls per step) around a library call that
does nothing — the entry points are Python callables that return FZ_OK and leave the out-parameters NULL / 0 — so that a
change to fuzzysearch_amd/_native.py can be held against its parent without a GPU.  api_host_cost.py times the layers
above the binding; this times the binding itself.
    python benchmarks/binding_host_cost.py"""
import os, sys, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fuzzysearch_amd import _native


class _Lib(object):
    @staticmethod
    def fz_free(p):
        pass

    @staticmethod
    def fz_lev_ngrams(*a):
        return 0
    fz_lev_ngrams_consolidated = fz_lev_ngrams_begin = fz_lev_ngrams_end = fz_lev_ngrams


class _Handle(object):
    _h = None


eng = _native.Engine.__new__(_native.Engine)
eng._lib, eng._h, eng._lock = _Lib, None, threading.RLock()
h, p = _Handle(), b"ACGTACGTACGTACGTACGT"


def timed(fn, reps=20000):
    best = 1e9
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best * 1e6


def pair():
    eng.lev_ngrams_begin(h, p, 2)
    eng.lev_ngrams_end(as_array=True)


print("lev_ngrams(as_array) %.3f  lev_ngrams(list) %.3f  lev_ngrams_consolidated(as_array) %.3f  rows_call %.3f  begin+end %.3f  "
      "search_end %.3f us per call" % (
          timed(lambda: eng.lev_ngrams(h, p, 2, as_array=True)), timed(lambda: eng.lev_ngrams(h, p, 2)),
          timed(lambda: eng.lev_ngrams_consolidated(h, p, 2, as_array=True)),
          timed(lambda: eng.rows_call(_Lib.fz_lev_ngrams_consolidated, h, p, 2).release()), timed(pair),
          timed(lambda: eng.search_end(as_array=True))))
