"""-m gpu: the RAGGED kernel instances (batch_scan_kernel, fz_batch_verify_kernel, fz_batch_verify_wf_kernel<16|32|64>,
fz_batch_verify_big_kernel<1|2|4|16|32>, the exact route's confirmation) at every seam between the sequences of a batch
(tests/batch_seam_case.py; its construction is checked on the CPU by tests/test_batch_seam_case.py).  One test per route; a
route uploads one batch per seam class and searches it twice (raw, reduced): the full ordered raw stream with its sequence
numbers, the reduced rows, stats()["raw_matches"] and stats()["verify_form"] against the oracle run on every sequence alone
and the form the plan hook names.  Noisy batches for the fused forms and for both record paths of
fz_batch_verify_wf_kernel, one public call per form, one assignment through a stand-alone kernel.  Each test prints what it
ran (pytest -s / -rP)."""
import os
import subprocess
import sys

import pytest

from tests import batch_seam_case as bc
from tests import gpu_cases
from tests.test_gpu_scan_seams import device_cus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one route per verification form / stand-alone instance goes through find_near_matches_batch as well
PUBLIC = ("exact-8", "subs-L6-k3", "subs-dense-20-4", "band-L6-k2", "bits32-20-4", "bits64-54-8", "bits128-65-10", "cells16-150-5",
          "cells32-dense-150-8", "kernel-140-34", "ring-band-300-2", "ring-subs-300-10", "wf32-150-8", "wf64-140-20", "big1-1030-2")


def _cases():
    """One test per route; the two routes with k >= 256, whose oracle costs 10^8 cells and more per copy: one per class."""
    out = []
    for r in bc.ROUTES:
        if not r.env:
            out += [(r, cls) for cls in bc.classes_of(r)] if bc.tier(r) == 2 else [(r, None)]
    return out


@pytest.mark.parametrize("r, cls", _cases(), ids=lambda x: x if isinstance(x, str) else "" if x is None else x.name)
def test_every_seam(engine, r, cls):
    line, n_search, n_rows = gpu_cases.run_batch_seam_route(engine, r, device_cus(), public=r.name in PUBLIC,
                                                            classes=(cls,) if cls else None)
    print("%s | %d searches, %d rows" % (line, n_search, n_rows))
    assert n_search >= 2 and n_rows > 0


@pytest.mark.parametrize("r", [r for r in bc.ROUTES if r.env], ids=lambda r: r.name)
def test_every_seam_under_a_switch(r):
    """The instances only a process-wide switch selects (FZ_NO_BITS: the register band at budgets 3 and 4; FZ_NO_WF_FUSE:
    fz_batch_verify_wf_kernel<16>; FZ_FORCE_BIG_VERIFY: fz_batch_verify_big_kernel<1 | 2 | 4 | 16> on short patterns), in a fresh
    interpreter."""
    e = dict(os.environ)
    e.update(r.env)
    res = subprocess.run([sys.executable, "-m", "tests.gpu_cases", "batch-seams", r.name, str(device_cus())], cwd=ROOT, env=e,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = res.stdout.decode()
    assert res.returncode == 0 and "OK " in out, out[-3000:]
    print(out.strip())


@pytest.mark.parametrize("name, tiles, side", bc.NOISY_ROUTES)
def test_noisy_batch(engine, name, tiles, side):
    """Reads over the pattern's own alphabet: the ragged lookups inside full queues, block-range passes and the slow-tile path
    of every fused form; fz_batch_verify_wf_kernel<64> with a hit list on either side of FZ_WF_COMPACT_MIN = 8192 (slotted
    records, appended records), by the oracle's count and by the device's."""
    rows, hits, on_device = gpu_cases.run_batch_noisy(engine, bc.route(name), device_cus(), tiles, side)
    print("noisy %s: %d rows, %d n-gram hits by the oracle, %d on the device" % (name, rows, hits, on_device))


def test_assignment_through_a_stand_alone_kernel(engine):
    """fz_batch_assign with ONE pattern of a stand-alone route (k <= 127: its records pass through assign_fold_host) on the
    `short` batch against the model of the definition over the oracle's rows."""
    from tests.test_assign_host import as_tuples, oracle_model
    r = bc.route("kernel-140-34")
    p = bc.sc.route_pattern(r)
    seqs, _plants, _cover = bc.build(r, "short", p)
    blob, offs = bc.pack(seqs)
    want = oracle_model(bc.LEV, [p], seqs, r.k, {})
    h = engine.upload_batch(blob, offs)
    try:
        got = engine.batch_assign(h, bc.LEV, [p], r.k)
        assert as_tuples(got) == want
    finally:
        h.release()
    assert sum(1 for w in want if w[0] == 0) >= 5
