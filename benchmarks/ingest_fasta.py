"""How a reference genome gets to the device: resident_fasta against stripping the file in Python
(the table of profiles/r17_ingest_fasta.txt).

    python benchmarks/ingest_fasta.py [--bases 1073741824] [--contigs 24] [--reps 5] [--base-reps 2] [--guides 64] [--trace-run]

Input: a synthetic genome of `--bases` bases of workloads.dna in `--contigs` contigs of unequal lengths, 30 % of the bases in
lower case, as a FASTA text of 60-column lines made here.
  (a) host    the route without resident_fasta: split on '>', replace(b'\\n', b''), upper(), then resident_batch(list)
  (b) bytes   resident_fasta(data, upper=True)
Each is one call that ends with the batch resident and its handle released again; 1 round of warm-up, then the median and
the min-max spread of the host clock over the rounds.  (b) is split, from the engine's own spans of the call
(Engine.records_ms: hipEvents around the copy and the kernels, the host clock around the D2H of ends[]), into the H2D copy,
the sum of the ingest kernels, the D2H of ends[] and the rest.  Before anything is timed the batch of (b) is compared with
the batch of (a): the same packed bytes and ends, and the index with the lengths and names of (a).
Then find_near_matches_multi_batch over the handle of (b): `--guides` guides of 20 + NGG, classes=IUPAC_DNA, 3 substitutions.
--trace-run: nothing but the input and two calls of (b), for a kernel trace of the second one.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fuzzysearch_amd import _native           # noqa: E402
from tests import workloads                   # noqa: E402


def make_fasta(flat, n_contigs, width=60):
    """bases -> (the FASTA text, the contigs' lengths): contig c holds a share proportional to n_contigs - c."""
    weights = np.arange(n_contigs, 0, -1, dtype=np.float64)
    cuts = np.floor(np.cumsum(weights) / weights.sum() * len(flat)).astype(np.int64)
    cuts[-1] = len(flat)
    parts, lo = [], 0
    for c, hi in enumerate(cuts.tolist()):
        seq = flat[lo:hi]
        full = len(seq) // width
        rec = np.empty((full, width + 1), dtype=np.uint8)
        rec[:, :width] = seq[:full * width].reshape(full, width)
        rec[:, width] = 10
        parts += [b'>chr%d synthetic contig %d\n' % (c + 1, c + 1), rec.tobytes()]
        if len(seq) > full * width:
            parts += [seq[full * width:].tobytes(), b'\n']
        lo = hi
    return b''.join(parts), np.diff(np.concatenate([[0], cuts]))


def host_route(data):
    seqs = []
    for part in data.split(b'>')[1:]:
        _head, _, body = part.partition(b'\n')
        seqs.append(body.replace(b'\n', b'').upper())
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1 << 30)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2)
    ap.add_argument("--guides", type=int, default=64)
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    import fuzzysearch_amd as fa
    flat = workloads.dna(a.bases, 20271019)
    rnd = np.random.default_rng(17)
    guides = [workloads.dna(20, 9300 + i) for i in range(a.guides)]
    for i, g in enumerate(guides):                                     # the protospacer and a PAM behind it, 8 times each
        site = np.concatenate([g, np.frombuffer(b'AGG', dtype=np.uint8)])
        workloads.plant_variants(flat, site, 8, 3300 + i)
    for lo in range(0, len(flat), 1 << 26):                            # 30 % lower case (soft masking), a piece at a time
        piece = flat[lo:lo + (1 << 26)]
        piece |= (rnd.random(len(piece)) < 0.3).astype(np.uint8) << 5
    data, lengths = make_fasta(flat, a.contigs)
    del flat
    eng = _native.default_engine()
    eng.set_timing(True)
    print("ingest: %d bases in %d contigs as FASTA of 60-column lines, 30 %% lower case (%.0f MB of text); %d rounds after 1 of warm-up "
          "(%d for the host route)" % (a.bases, a.contigs, len(data) / 1e6, a.reps, a.base_reps))
    sys.stdout.flush()

    def route_bytes():
        held = fa.resident_fasta(data, upper=True)
        held.release()

    if a.trace_run:
        route_bytes()
        route_bytes()
        return

    def route_host():
        held = fa.resident_batch(host_route(data))
        held.release()

    held = fa.resident_fasta(data, upper=True)
    seqs = host_route(data)
    listed = fa.resident_batch(seqs)
    assert len(held) == len(listed) == a.contigs and held.lengths.tolist() == lengths.tolist() == [len(s) for s in seqs]
    assert list(held.names) == [b'chr%d' % (c + 1) for c in range(a.contigs)]
    assert eng.batch_bytes(held.handle) == eng.batch_bytes(listed.handle), "the two batches differ"
    assert np.array_equal(eng.batch_tables(held.handle)[1], eng.batch_tables(listed.handle)[1])
    assert held.sequences[3][1000:1100] == seqs[3][1000:1100]
    listed.release()
    held.release()
    del seqs, listed

    t0 = time.perf_counter()
    route_host()
    base = []
    for _ in range(a.base_reps):
        t0 = time.perf_counter()
        route_host()
        base.append((time.perf_counter() - t0) * 1e3)
    s_med = float(np.median(base))
    print("(a) split + replace + upper + resident_batch  %10.1f ms [%9.1f, %9.1f]" % (s_med, min(base), max(base)))
    sys.stdout.flush()
    route_bytes()
    walls, spans = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        route_bytes()
        walls.append((time.perf_counter() - t0) * 1e3)
        spans.append(eng.records_ms())
    b_med = float(np.median(walls))
    print("(b) resident_fasta(bytes, upper=True)         %10.1f ms [%9.1f, %9.1f]   (a) / (b) = %.1f" % (b_med, min(walls), max(walls), s_med / b_med))
    for key, label in (("h2d", "H2D copy of the text"), ("kernels", "ingest kernels, summed"), ("ends_d2h", "D2H of ends[]"),
                       ("call", "the C-ABI call, whole")):
        v = [s[key] for s in spans]
        print("      %-28s %10.2f ms [%9.2f, %9.2f]" % (label, float(np.median(v)), min(v), max(v)))
    rest = [w - s["h2d"] - s["kernels"] - s["ends_d2h"] for w, s in zip(walls, spans)]
    print("      %-28s %10.2f ms [%9.2f, %9.2f]" % ("host remainder", float(np.median(rest)), min(rest), max(rest)))
    k_med, h_med = float(np.median([s["kernels"] for s in spans])), float(np.median([s["h2d"] for s in spans]))
    print("      kernels / H2D = %.3f (%.0f GB/s of text through the kernels, %.1f GB/s over PCIe); %.4f ns of kernels per packed byte"
          % (k_med / h_med, len(data) / k_med / 1e6, len(data) / h_med / 1e6, k_med * 1e6 / a.bases))
    sys.stdout.flush()

    held = fa.resident_fasta(data, upper=True)
    sites = [g.tobytes() + b'NGG' for g in guides]
    limits = dict(max_substitutions=3, max_insertions=0, max_deletions=0, classes=fa.IUPAC_DNA)
    hits = fa.find_near_matches_multi_batch(sites, held, **limits)
    n_hits = sum(len(per) for per_guide in hits for per in per_guide)
    pub = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fa.find_near_matches_multi_batch(sites, held, **limits)
        pub.append((time.perf_counter() - t0) * 1e3)
    print("find_near_matches_multi_batch over the handle, %d guides of 20 + NGG, classes=IUPAC_DNA, 3 substitutions (%d matches in "
          "contig coordinates): %.2f ms [%.2f, %.2f]" % (len(sites), n_hits, float(np.median(pub)), min(pub), max(pub)))
    g, c, m = next((g, c, per[0]) for g, per_guide in enumerate(hits) for c, per in enumerate(per_guide) if per)
    print("      e.g. guide %d: %s:%d-%d dist %d %r" % (g, held.names[c].decode(), m.start, m.end, m.dist, m.matched))
    held.release()


if __name__ == "__main__":
    main()
