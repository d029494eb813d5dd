"""What giving a result back as a file costs: format_records on the device against joining the reads in Python
(profiles/r21_format.txt).

    python benchmarks/egress_reads.py [--reads 4000000] [--read-len 150] [--reps 5] [--base-reps 2]

Input: the ingest benchmark's FASTQ text, `--reads` synthetic reads of `--read-len` bytes.
  (a) resident_records(lines=(0, 1, 3)), ONE upload and one line table for headers, bases and qualities, against three
      uploads of the text that keep one line each;
  (b) a trim and a selection of the three columns (derive), then format_records(cols, 'fastq') with the engine's own spans
      (Engine.format_ms: hipEvents on the stream around the descriptor's copy, measure + scan, the gather; the host clock
      around the D2H of the text, started once the gather has finished), into a numpy array and (write_records) into the
      mapping of a file, against the route without it: b''.join over the three `.sequences` views;
  (c) the gather's bytes read + written per second next to the plain derive gather's of the same session (the identity
      derive of the bases: fz_rec_gather_kernel), and the share of 16-byte pieces that take the byte path, counted on the
      host from the tables.
The formatted text is compared with the Python route's before anything is timed.  1 round of warm-up, then the median and
the min-max spread over `--reps` rounds (`--base-reps` for the Python route).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fuzzysearch_amd import _native           # noqa: E402
from tests import workloads                   # noqa: E402
from ingest_reads import make_fastq           # noqa: E402

PEAK_GBS = 8000.0


def stat(v):
    return float(np.median(v)), min(v), max(v)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stat(out)


def byte_path_share(cols, lits):
    """-> (pieces, pieces on the byte path) of the text of `cols` under `lits`, from the lengths alone: a piece is a plain
    16-byte copy when it lies wholly inside one sequence of one column."""
    lens = [c.lengths.astype(np.int64) for c in cols]
    rec = sum(lens) + sum(len(l) for l in lits)
    at = np.concatenate([[0], np.cumsum(rec)])
    total = int(at[-1])
    fast = 0
    pos = at[:-1] + len(lits[0])
    for c, ln in enumerate(lens):
        first = (pos + 15) // 16                            # the first piece that starts inside the segment
        last = (pos + ln - 16) // 16                        # the last one that ends inside it
        fast += int(np.maximum(last - first + 1, 0)[ln >= 16].sum())
        pos = pos + ln + len(lits[c + 1])
    pieces = (total + 15) // 16
    return pieces, pieces - fast


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2)
    a = ap.parse_args()
    import fuzzysearch_amd as fa
    dna = workloads.dna(a.reads * a.read_len, 20251019).reshape(a.reads, a.read_len)
    data = make_fastq(dna)
    eng = _native.default_engine()
    eng.set_timing(True)
    lits = _native.FORMAT_PRESETS["fastq"][0]
    print("egress: %d reads x %d bytes, a FASTQ text of %.0f MB; %d rounds after 1 of warm-up (%d for the Python route)"
          % (a.reads, a.read_len, len(data) / 1e6, a.reps, a.base_reps))

    # -- (a) one upload for three lines against three uploads
    def one_upload():
        for b in fa.resident_records(data, lines=(0, 1, 3)):
            b.release()

    def three_uploads():
        for line in (0, 1, 3):
            for b in fa.resident_records(data, lines=(line,)):
                b.release()

    one_upload()
    rec = []
    for _ in range(a.reps):
        one_upload()
        rec.append(eng.records_ms())
    print("(a) resident_records(lines=(0, 1, 3))   %9.1f ms [%9.1f, %9.1f]" % timed(one_upload, a.reps))
    print("      its spans: H2D %.1f ms, the kernels of all lines %.3f ms, ends[] back %.2f ms, the C-ABI call %.1f ms (medians)"
          % tuple(float(np.median([r[k] for r in rec])) for k in ("h2d", "kernels", "ends_d2h", "call")))
    three_uploads()
    print("    three uploads of one line each      %9.1f ms [%9.1f, %9.1f]" % timed(three_uploads, a.reps))
    sys.stdout.flush()

    # -- (b) trim, select, format
    heads, reads, quals = fa.resident_records(data, lines=(0, 1, 3))
    rnd = np.random.RandomState(21)
    ends = rnd.randint(a.read_len * 2 // 3, a.read_len + 1, size=a.reads).astype(np.uint64)
    keep = ends >= np.uint64(a.read_len * 3 // 4)
    cols = (heads.derive(index=keep), reads.derive(index=keep, ends=ends[keep]), quals.derive(index=keep, ends=ends[keep]))

    def python_route():
        parts = []
        for h, r, q in zip(cols[0].sequences, cols[1].sequences, cols[2].sequences):
            parts += (h, b"\n", r, b"\n+\n", q, b"\n")
        return b"".join(parts)

    want = python_route()
    got = fa.format_records(cols, "fastq")
    assert got.tobytes() == want
    size = len(want)
    print("(b) %d of %d reads kept and trimmed: a text of %.0f MB; format_records equals b''.join over the three .sequences views"
          % (int(keep.sum()), a.reads, size / 1e6))
    del got
    out = np.empty(size, dtype=np.uint8)
    fa.format_records(cols, "fastq", out=out)
    walls, spans = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fa.format_records(cols, "fastq", out=out)
        walls.append((time.perf_counter() - t0) * 1e3)
        spans.append(eng.format_ms())
    print("    format_records(cols, 'fastq', out=array)  %9.1f ms [%9.1f, %9.1f]" % stat(walls))
    for key, label in (("desc_h2d", "descriptor up (H2D)"), ("measure_scan", "measure + scan"), ("gather", "gather"),
                       ("text_d2h", "text back (D2H, host clock)"), ("call", "the C-ABI call, whole")):
        print("      %-32s %10.3f ms [%9.3f, %9.3f]" % ((label,) + stat([s[key] for s in spans])))
    d2h = float(np.median([s["text_d2h"] for s in spans]))
    print("      text back: %.1f GB/s into a pageable numpy array" % (size / d2h / 1e6))
    fresh = timed(lambda: fa.format_records(cols, "fastq"), a.reps)
    print("    format_records(cols, 'fastq')             %9.1f ms [%9.1f, %9.1f]   (a new array per call)" % fresh)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "trimmed.fastq")
        fa.write_records(path, cols, "fastq")
        with open(path, "rb") as f:
            assert f.read() == want
        wr, wspans = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fa.write_records(path, cols, "fastq")
            wr.append((time.perf_counter() - t0) * 1e3)
            wspans.append(eng.format_ms())
        wd = float(np.median([s["text_d2h"] for s in wspans]))
        print("    write_records(path, cols, 'fastq')        %9.1f ms [%9.1f, %9.1f]   text back into the file's mapping %.1f ms = %.1f GB/s"
              % (stat(wr) + (wd, size / wd / 1e6)))
    py = timed(python_route, a.base_reps)
    print("    b''.join over the three .sequences views  %9.1f ms [%9.1f, %9.1f]   ratio to format_records(out=array) %.0f, to write_records %.0f"
          % (py + (py[0] / stat(walls)[0], py[0] / stat(wr)[0])))
    sys.stdout.flush()

    # -- (c) the gather next to the plain derive gather of this session
    g = stat([s["gather"] for s in spans])
    eng.derive_batch(reads.handle).release()
    plain = []
    for _ in range(a.reps):
        h = eng.derive_batch(reads.handle)
        plain.append(eng.derive_ms()["gather"])
        packed = len(h)
        h.release()
    p = stat(plain)
    pieces, slow = byte_path_share(cols, lits)
    print("(c) fz_format_gather_kernel  %8.3f ms [%8.3f, %8.3f]  %6.0f GB/s of bytes read + written = %4.1f %% of %.0f GB/s"
          % (g + (2 * size / g[0] / 1e6, 2 * size / g[0] / 1e6 / PEAK_GBS * 100, PEAK_GBS)))
    print("    plain derive gather      %8.3f ms [%8.3f, %8.3f]  %6.0f GB/s (identity derive of the bases, %.0f MB, this session)"
          % (p + (2 * packed / p[0] / 1e6, packed / 1e6)))
    print("    the format gather runs at %.2f of the plain derive gather's rate; %d of %d pieces (%.1f %%) take the byte path"
          % ((2 * size / g[0]) / (2 * packed / p[0]), slow, pieces, 100.0 * slow / pieces))
    for b in cols + (heads, reads, quals):
        b.release()


if __name__ == "__main__":
    main()
