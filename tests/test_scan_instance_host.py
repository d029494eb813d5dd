"""fz_debug_scan_instance (no device): which instance of the in-memory register-band / Hamming-count scan a search's
launches run.  Lean (fz_lean_scan_kernel: no equal-n-gram slot sets, register bands for k <= 2 only) where nothing the full
instance carries on top can run; full for equal n-grams and for k = 3, 4 on the band.  A function of the search's arguments
and the switches."""
import ctypes

import pytest

from fuzzysearch_amd import _native
from tests import workloads
from tests.scan_instance_case import LEV, SUBS, REPEATED, reload_switches, scan_instance

FORM_FUSED_BAND = _native.FORM_FUSED_BAND


@pytest.fixture
def no_bits(monkeypatch):
    """The bit-vector forms switched off: Levenshtein budgets 3 and 4 stay on the register band."""
    monkeypatch.setenv("FZ_NO_BITS", "1")
    reload_switches()
    yield
    monkeypatch.delenv("FZ_NO_BITS")
    reload_switches()


def test_headline_search_runs_the_lean_instance():
    _, pattern, _ = workloads.cfg2(1 << 16, 4)
    for buf_len in (1 << 30, 4 << 30, 49157):
        assert scan_instance(LEV, pattern.tobytes(), 2, buf_len) == (1, [True], FORM_FUSED_BAND)


def test_budget_one_and_substitutions_with_distinct_ngrams_are_lean():
    assert scan_instance(LEV, workloads.dna(20, 1).tobytes(), 1) == (1, [True], FORM_FUSED_BAND)
    assert scan_instance(SUBS, workloads.text65(32, 33).tobytes(), 3) == (1, [True], FORM_FUSED_BAND)      # configs[2]
    assert scan_instance(SUBS, workloads.dna(32, 5).tobytes(), 3) == (1, [True], FORM_FUSED_BAND)


def test_equal_ngrams_take_the_full_instance():
    assert scan_instance(LEV, REPEATED, 2) == (1, [False], FORM_FUSED_BAND)
    assert scan_instance(SUBS, REPEATED, 2) == (1, [False], FORM_FUSED_BAND)
    # a pattern that repeats one n-gram among distinct ones is full as well
    assert scan_instance(LEV, b"ACGTAC" + b"TTGACA" + b"ACGTAC" + b"GG", 2) == (1, [False], FORM_FUSED_BAND)


def test_budgets_three_and_four_on_the_band_take_the_full_instance(no_bits):
    for m, k in ((24, 3), (40, 4)):
        assert scan_instance(LEV, workloads.dna(m, 7 + k).tobytes(), k) == (1, [False], FORM_FUSED_BAND)
    # the switch changes nothing below 3
    assert scan_instance(LEV, workloads.dna(20, 1).tobytes(), 2) == (1, [True], FORM_FUSED_BAND)


def test_other_forms_have_no_lean_instance():
    """Bit-vector columns (k >= 3 by default, dense short patterns), lane-per-cell and stand-alone verification: full."""
    for m, k in ((24, 3), (40, 4), (54, 8), (12, 2), (300, 40)):
        nl, lean, form = scan_instance(LEV, workloads.dna(m, 11).tobytes(), k)
        assert form != FORM_FUSED_BAND and lean == [False] * nl


def test_bad_arguments_are_refused():
    L = _native.load_library()
    out = ctypes.c_uint32(0)
    assert L.fz_debug_scan_instance(0, b"ACGT", 4, 0, 1 << 20, 256, ctypes.byref(out), ctypes.byref(out), ctypes.byref(out)) != 0
    assert L.fz_debug_scan_instance(LEV, b"ACGT", 4, 4, 1 << 20, 256, ctypes.byref(out), ctypes.byref(out), ctypes.byref(out)) != 0
