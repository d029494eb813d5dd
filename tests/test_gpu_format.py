"""-m gpu: format_records / fz_batch_format — batches become the text of a file on the device — against the three-line model
(tests/format_model.py), and resident_records(lines=...) / fz_batch_upload_records_lines against tests/records_model.py:
the round trip of a canonical FASTQ text, every seam of the gather at a tile edge of the destination, the scan's seams, the
degenerate cases, the verdict on bad records, every kind of column, the several-line upload, the pipeline, the refusals."""
import ctypes
import random

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native
from tests import format_model as fmod
from tests import records_model as rm
from tests import fasta_model as fm

pytestmark = pytest.mark.gpu

TILE = 16384
FASTQ_LITS, FASTQ_EQUAL = fmod.PRESETS["fastq"]


def upload(engine, seqs):
    return engine.upload_batch(b"".join(seqs), np.array(fmod.offsets(seqs), dtype=np.uint64))


def check(engine, cols, lits, equal=None):
    """The text of fz_batch_format over uploaded columns (a list object given twice: one handle twice) == the model's."""
    handles = {}
    for c in cols:
        if id(c) not in handles:
            handles[id(c)] = upload(engine, c)
    try:
        want = fmod.model(cols, lits)
        got = engine.format_batch([handles[id(c)] for c in cols], lits, equal)
        assert got.dtype == np.uint8 and len(got) == len(want)
        if got.tobytes() != want:
            g = np.frombuffer(want, dtype=np.uint8)
            first = int(np.flatnonzero(got != g)[0])
            raise AssertionError("first difference at byte %d of %d (tile %d + %d)" % (first, len(want), first // TILE, first % TILE))
        return want
    finally:
        for h in handles.values():
            h.release()


# ---- the round trip

def canonical_fastq(n, seed=20):
    heads, reads, quals = fmod.fastq_columns(fmod.rng(seed), n, max_len=170)
    return rm.fastq(reads, heads=heads, quals=quals), (heads, reads, quals)


def test_round_trip_of_a_canonical_fastq_text(engine):
    text, cols = canonical_fastq(3000)
    assert 300 << 10 < len(text) < 1 << 20
    h, r, q = fa.resident_records(text, engine=engine, lines=(0, 1, 3))
    try:
        assert (h.line, r.line, q.line) == (0, 1, 3) and len(h) == len(r) == len(q) == 3000
        assert [list(b.sequences) for b in (h, r, q)] == [list(c) for c in cols]
        got = fa.format_records((h, r, q), "fastq")
        assert got.tobytes() == text
    finally:
        for b in (h, r, q):
            b.release()
    lines = b"".join(s + b"\n" for s in cols[1])
    (only,) = fa.resident_records(lines, format="lines", engine=engine, lines=(0,))
    try:
        assert fa.format_records(only, "lines").tobytes() == lines
        assert only.format == "lines"                                       # (a RecordBatch keeps the name of its format there)
        trimmed = only.derive(ends=[len(s) // 2 for s in cols[1]])
        assert trimmed.format().tobytes() == b"".join(s[:len(s) // 2] + b"\n" for s in cols[1])       # BatchSequences.format: one column
        trimmed.release()
    finally:
        only.release()


# ---- the gather's seams

@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_every_alignment_pair(engine, C):
    """A few thousand records of sequence lengths 0 .. 33 in shuffled order: every (source mod 16, destination mod 16) pair."""
    rnd = fmod.rng(100 + C)
    cols = fmod.random_columns(rnd, C, 4000)
    lits = tuple(fmod.rnd_bytes(rnd, (0, 1, 3, 17, 2, 0, 5, 1, 4)[i]) for i in range(C + 1))
    at = fmod.starts(cols, lits)
    pairs = set()
    offs = fmod.offsets(cols[0])
    for j in range(len(cols[0])):
        if len(cols[0][j]) >= 16:
            pairs.add((offs[j] % 16, (at[j] + len(lits[0])) % 16))
    assert len(pairs) == 256
    check(engine, cols, lits)


def seam_sweep(C, seq_len, lit_len, deltas, rnd):
    """Records of C sequences of seq_len bytes between literals of lit_len bytes, placed so that every one of their 2C + 1
    seams (the record's start, every literal / sequence border) lies at tile edge + delta for every delta, one placement per
    tile edge; filler records (one long sequence in column 0) bring the text to the next placement."""
    lits = tuple(fmod.rnd_bytes(rnd, lit_len) for _ in range(C + 1))
    cols = [[] for _ in range(C)]
    seams = [0]
    for s in range(2 * C + 1):
        seams.append(seams[-1] + (lit_len if s % 2 == 0 else seq_len))
    seams = seams[:-1]                                                      # offsets of the 2C + 1 segment starts in a record
    cur, edge = 0, 0
    placed = []
    for s in seams:
        for d in deltas:
            edge += TILE
            start = edge + d - s
            gap = start - cur - lit_len * (C + 1)
            assert gap >= 0
            cols[0].append(fmod.rnd_bytes(rnd, gap))
            for c in range(1, C):
                cols[c].append(b"")
            for c in range(C):
                cols[c].append(fmod.rnd_bytes(rnd, seq_len))
            placed.append(start + s)
            cur = start + lit_len * (C + 1) + seq_len * C
    at = fmod.starts(cols, lits)
    assert set(p % TILE if p % TILE < TILE // 2 else p % TILE - TILE for p in placed) == set(deltas)
    assert at[-1] == cur
    return cols, lits, placed


@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_short_records_slide_across_a_tile_edge(engine, C):
    """Segments of 2 or 3 bytes: the whole record lies near the edge, and every seam of it — the record's, every column's,
    every literal's — stands at every offset from -17 to +17, one call of 35 tiles per seam; literals alone straddle the
    edge (no sequence bytes at all) and so do sequences alone (empty literals)."""
    rnd = fmod.rng(200 + C)
    for seq_len, lit_len in ([(2, 2), (3, 0), (0, 3)] if C < 3 else [(2, 2)]):
        for seam in range(2 * C + 1):
            check(engine, *seam_sweep_one(C, seq_len, lit_len, list(range(-17, 18)), seam, rnd))


def seam_sweep_one(C, seq_len, lit_len, deltas, seam, rnd):
    """seam_sweep for one of the 2C + 1 seams only."""
    lits = tuple(fmod.rnd_bytes(rnd, lit_len) for _ in range(C + 1))
    cols = [[] for _ in range(C)]
    s = sum(lit_len if i % 2 == 0 else seq_len for i in range(seam))
    cur, edge = 0, 0
    for d in deltas:
        edge += TILE
        start = edge + d - s
        cols[0].append(fmod.rnd_bytes(rnd, start - cur - lit_len * (C + 1)))
        for c in range(1, C):
            cols[c].append(b"")
        for c in range(C):
            cols[c].append(fmod.rnd_bytes(rnd, seq_len))
        cur = start + lit_len * (C + 1) + seq_len * C
    return cols, lits


@pytest.mark.parametrize("C", [1, 2, 3])
def test_long_segments_at_a_tile_edge(engine, C):
    """Sequences of 40 bytes (whole 16-byte pieces inside them) and literals of 3: every seam at the offsets where a piece
    starts, ends or straddles the edge."""
    rnd = fmod.rng(300 + C)
    cols, lits, _placed = seam_sweep(C, 40, 3, [-17, -16, -15, -1, 0, 1, 15, 16, 17], rnd)
    assert fmod.starts(cols, lits)[-1] < (1 << 20) + (64 << 10)
    check(engine, cols, lits)


def test_long_records_long_literals_and_the_text_s_end(engine):
    rnd = fmod.rng(400)
    # one record longer than two tiles, between short ones, in the last of three columns
    cols = fmod.random_columns(rnd, 3, 40)
    cols[2][17] = fmod.rnd_bytes(rnd, 2 * TILE + 4321)
    cols[0][30] = fmod.rnd_bytes(rnd, TILE + 5)
    check(engine, cols, (b"<", b"|", b"", b">\n"))
    # literals of 255 bytes: most tile edges fall inside a literal
    one = fmod.random_columns(rnd, 1, 200)
    check(engine, one, (fmod.rnd_bytes(rnd, 255), fmod.rnd_bytes(rnd, 255)))
    check(engine, one + one, (fmod.rnd_bytes(rnd, 255), b"", fmod.rnd_bytes(rnd, 250)))       # the same handle twice
    # a text that ends 1, 15, 16 and 17 bytes past a tile edge (and exactly on it)
    for past in (0, 1, 15, 16, 17):
        seqs = [fmod.rnd_bytes(rnd, k) for k in (33, 0, 16, 5)]
        fill = 2 * TILE + past - sum(map(len, seqs)) - 5
        want = check(engine, [seqs + [fmod.rnd_bytes(rnd, fill)]], (b"", b"\n"))
        assert len(want) == 2 * TILE + past


@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("blocks", [1, 2])
def test_scan_seams(engine, blocks, off):
    """n one below, at and one above the items of one and of two scan workgroups."""
    rnd = fmod.rng(10 * blocks + off)
    n = _native.scan_items() * blocks + off
    heads, reads, quals = fmod.fastq_columns(rnd, n, max_len=20)
    check(engine, [heads, reads, quals], FASTQ_LITS, FASTQ_EQUAL)


def test_degenerate_cases(engine):
    check(engine, [[]], (b"x", b"\n"))                                      # n = 0
    check(engine, [[], []], (b"", b"\t", b"\n"))
    assert check(engine, [[b""] * 70], (b"", b"")) == b""                   # all empty, empty literals: a text of 0 bytes
    check(engine, [[b""] * 70, [b""] * 70], (b">", b"\n", b"\n"))           # all empty, with literals
    check(engine, [[b"ACGT"]], (b"", b"\n"))                                # one record
    check(engine, [[b""]], (b"", b"\n"))
    check(engine, [[b"@r"], [b"A" * 100], [b"I" * 100]], FASTQ_LITS, FASTQ_EQUAL)
    cols = fa.resident_records(b"", engine=engine, lines=(0, 1, 3))         # n = 0 through the public calls
    assert [len(c) for c in cols] == [0, 0, 0] and fa.format_records(cols, "fastq").tobytes() == b""


def test_bad_records(engine):
    rnd = fmod.rng(5)
    n = 70010
    heads, reads, quals = fmod.fastq_columns(rnd, n, max_len=12)
    want = fmod.model([heads, reads, quals], FASTQ_LITS)
    hb, rb = fa.resident_batch(heads, engine=engine), fa.resident_batch(reads, engine=engine)
    try:
        for bad in ([0], [n - 1], [40000, 69999], [69999, 3]):
            q = list(quals)
            for j in bad:
                q[j] = q[j] + b"I"
            qb = fa.resident_batch(q, engine=engine)
            canary = np.full(len(want) + 64, 0xAB, dtype=np.uint8)
            with pytest.raises(ValueError, match=r"^format: record %d: the two columns checked for equal length differ in length$" % min(bad)) as e:
                fa.format_records((hb, rb, qb), "fastq", out=canary)
            assert (e.value.info["bad_record"], e.value.info["bad_reason"]) == (min(bad), 1)
            assert (canary == 0xAB).all()                                   # nothing was written
            got = fa.format_records((hb, rb, qb), literals=FASTQ_LITS)      # unchecked, the same columns are a text
            assert got.tobytes() == fmod.model([heads, reads, q], FASTQ_LITS)
            qb.release()
        qb = fa.resident_batch(quals, engine=engine)                        # the next call is correct
        assert fa.format_records((hb, rb, qb), "fastq").tobytes() == want
        qb.release()
    finally:
        hb.release()
        rb.release()


def test_every_kind_of_column(engine, tmp_path):
    rnd = fmod.rng(6)
    names = [b"chr%d" % i for i in range(12)]
    contigs = [fmod.rnd_bytes(rnd, rnd.choice([1, 59, 60, 61, 150, 400]), b"ACGTN") for _ in names]
    g = fa.resident_fasta(fm.fasta(contigs, width=60, heads=[b">" + n for n in names]), engine=engine)
    held_names = fa.resident_batch(list(g.names), engine=engine)
    reads = [fmod.rnd_bytes(rnd, rnd.randint(0, 90), b"ACGT") for _ in range(len(names))]
    plain = fa.resident_batch(reads, engine=engine)
    recs = fa.resident_records(b"".join(r + b"\n" for r in reads), format="lines", engine=engine)
    rc = plain.derive(reverse=True, translate=fa.DNA_COMPLEMENT)
    cut = plain.derive(index=list(range(len(reads)))[::-1], ends=[len(r) // 2 for r in reads[::-1]])
    parent = fa.resident_batch([r + b"TT" for r in reads], engine=engine)
    orphan = parent.derive(ends=[len(r) for r in reads])
    parent.release()                                                        # a released parent of a derived column
    try:
        fasta = fa.format_records((held_names, g), "fasta").tobytes()
        assert fasta == b"".join(b">" + n + b"\n" + c + b"\n" for n, c in zip(names, contigs))
        again = fa.resident_fasta(fasta, engine=engine)                     # unwrapped FASTA is FASTA
        assert [bytes(s) for s in again.sequences] == [bytes(s) for s in g.sequences] and list(again.names) == list(g.names)
        again.release()
        cols = (plain, recs, rc, cut, orphan)
        lits = (b"", b"\t", b"\t", b"\t", b"\t", b"\n")
        want = fmod.model([list(c.sequences) for c in cols], lits)
        assert fa.format_records(cols, literals=lits).tobytes() == want
        assert want.split(b"\n")[3].split(b"\t")[2] == reads[3].translate(fa.DNA_COMPLEMENT)[::-1]
        assert plain.format().tobytes() == b"".join(r + b"\n" for r in reads) == fa.format_records(recs, "lines").tobytes()
        assert rc.format(literals=(b"<", b">")).tobytes() == b"".join(b"<" + r.translate(fa.DNA_COMPLEMENT)[::-1] + b">" for r in reads)
        text = fa.resident_batch([r.decode() for r in reads], engine=engine)
        with pytest.raises(TypeError, match="batch of str"):
            fa.format_records(text, "lines")
        text.release()
    finally:
        for b in (g, held_names, plain, recs, rc, cut, orphan):
            b.release()


# ---- the several-line upload

def model_line(text, fmt, line):
    """-> (starts, sequences) of line `line` of every record by tests/records_model.py (Malformed as model raises it)."""
    rm.model(text, fmt)
    lines = rm.split_lines(bytes(text))
    period = 4 if fmt == "fastq" else 1
    if fmt == "fastq":
        while lines and lines[-1][1] == b"":
            lines.pop()
    kept = lines[line::period]
    return [s for s, _ in kept], [l for _, l in kept]


def check_lines(engine, text, fmt, lines):
    period, _seq, flags = _native.RECORD_FORMATS[fmt]
    try:
        rm.model(text, fmt)
    except rm.Malformed as bad:                                             # (an empty last read loses its quality line to the trim)
        with pytest.raises(ValueError, match="record %d:" % bad.record) as e:
            engine.upload_records_lines(text, period, lines, flags)
        assert (e.value.info["bad_record"], e.value.info["bad_reason"]) == (bad.record, bad.reason)
        return None
    handles = engine.upload_records_lines(text, period, lines, flags)
    try:
        assert len(handles) == len(lines)
        for h, line in zip(handles, lines):
            starts, seqs = model_line(text, fmt, line)
            assert h.n_seqs == len(seqs) == h.info["n_seqs"] and len(h) == sum(map(len, seqs)) == h.info["packed_bytes"]
            assert engine.batch_bytes(h) == b"".join(seqs)
            src, ends = engine.batch_tables(h)
            assert src.tolist() == starts and ends.tolist() == np.cumsum([len(s) for s in seqs]).astype(np.uint64).tolist()
        return handles[0].info
    finally:
        for h in handles:
            h.release()


def test_several_lines_against_the_records_model(engine):
    text, cols = canonical_fastq(500, seed=21)
    info = check_lines(engine, text, "fastq", (0, 1, 3))
    assert info["n_lines"] == 2000
    check_lines(engine, text, "fastq", (3, 0))                              # the order is the caller's
    check_lines(engine, text, "fastq", (2,))                                # line 1 not kept: measured for the verdict only
    check_lines(engine, text, "fastq", (1,))
    check_lines(engine, text, "fastq", (3, 2, 1, 0))
    heads, reads, quals = cols
    crlf = rm.fastq(reads, heads=heads, quals=quals, eol=b"\r\n")
    check_lines(engine, crlf, "fastq", (0, 1, 3))
    check_lines(engine, text + b"\n\r\n\n", "fastq", (0, 3))                # trailing empty lines
    check_lines(engine, text[:-1], "fastq", (3, 1))                         # no final terminator
    check_lines(engine, b"", "fastq", (0, 1, 3))
    check_lines(engine, b"\n\n", "fastq", (0, 3))
    check_lines(engine, b"AC\n\nGT\r\nA", "lines", (0,))
    rnd = rm.rng(77)
    for _ in range(60):
        check_lines(engine, rm.random_fastq_text(rnd), "fastq", rnd.choice([(0, 1, 3), (3, 0), (0,), (2, 3)]))
    big, _ = canonical_fastq(_native.scan_items() + 1, seed=22)             # a scan of two levels per line
    check_lines(engine, big, "fastq", (0, 1, 3))


def test_several_lines_report_as_the_single_line_call(engine):
    rnd = rm.rng(78)
    text, (heads, reads, quals) = canonical_fastq(300, seed=23)
    lines = text.split(b"\n")
    broken = [b"\n".join(lines[:-2]) + b"\n"]                               # 1: a truncated record
    for why, (rec, line, new) in {2: (7, 0, b"r7"), 3: (250, 2, b"-"), 4: (299, 3, lines[4 * 299 + 3] + b"I")}.items():
        b = list(lines)
        b[4 * rec + line] = new
        broken.append(b"\n".join(b))
    both = list(lines)
    both[4 * 100 + 2], both[4 * 5 + 3] = b"x", both[4 * 5 + 3] + b"II"      # two bad records: the lower one
    broken.append(b"\n".join(both))
    broken += [t for t in (rm.random_fastq_text(rnd, break_it=True) for _ in range(40))]
    seen = set()
    free = None
    for t in broken:
        try:
            engine.upload_records(t, 4, 1, 1).release()
            want = None
        except ValueError as e:
            want = (str(e), e.info["bad_record"], e.info["bad_reason"], e.info["n_lines"])
        for kept in ((0, 1, 3), (3, 0), (2,)):
            if want is None:
                check_lines(engine, t, "fastq", kept)
                continue
            with pytest.raises(ValueError) as e:
                engine.upload_records_lines(t, 4, kept, 1)
            assert (str(e.value), e.value.info["bad_record"], e.value.info["bad_reason"], e.value.info["n_lines"]) == want
            assert e.value.info["packed_bytes"] == 0
            seen.add(want[2])
        if want is not None:                                                # no handle is left: the device's free memory stands still
            now = engine.mem_info()[0]
            with pytest.raises(ValueError):
                engine.upload_records_lines(t, 4, (0, 1, 3), 1)
            assert engine.mem_info()[0] == now
    assert seen == {1, 2, 3, 4}
    for kept, match in (((0, 0), "twice"), ((4,), "smaller than"), ((), "between 1 and")):
        with pytest.raises(ValueError, match=match):
            engine.upload_records_lines(text, 4, kept, 1)
    with pytest.raises(ValueError, match="4 lines per record"):
        engine.upload_records_lines(text, 2, (0, 1), 1)


# ---- the pipeline

def test_the_pipeline_ingest_assign_trim_select_write(engine, tmp_path):
    rnd = random.Random(9)
    adapter = b"AGATCGGAAGAGCACACGTC"
    reads = []
    for j in range(400):
        body = bytes(rnd.choice(b"AC") for _ in range(rnd.randint(10, 150)))
        ad = bytearray(adapter)
        if j % 2:
            ad[j % 20] = ord("T") if ad[j % 20] != ord("T") else ord("A")
        reads.append(body + (bytes(ad) + bytes(rnd.choice(b"AC") for _ in range(j % 30)) if j % 6 else b""))
    heads = [b"@read%d/1" % j for j in range(len(reads))]
    quals = [bytes(rnd.choice(b"!5?I") for _ in r) for r in reads]
    src = tmp_path / "run1.fastq"
    src.write_bytes(rm.fastq(reads, heads=heads, quals=quals))
    h, r, q = fa.resident_records(str(src), engine=engine, lines=(0, 1, 3))
    best = fa.find_best_matches_batch([adapter], r, max_l_dist=2)
    ends = np.where(best.pattern >= 0, best.start, r.lengths)
    keep = ends >= 30
    cols = (h.derive(index=keep), r.derive(index=keep, ends=ends[keep]), q.derive(index=keep, ends=ends[keep]))
    path = str(tmp_path / "trimmed.fastq")
    try:
        size = fa.write_records(path, cols, format="fastq")
        kept = [j for j in range(len(reads)) if keep[j]]
        want = rm.fastq([reads[j][:int(ends[j])] for j in kept], heads=[heads[j] for j in kept], quals=[quals[j][:int(ends[j])] for j in kept])
        assert 100 < len(kept) < len(reads) and (best.pattern >= 0).sum() > 300
        assert size == len(want) and open(path, "rb").read() == want and all(adapter not in x for x in want.split(b"\n")[1::4])
        again = fa.resident_records(path, engine=engine, lines=(0, 1, 3))
        for a, b in zip(again, cols):
            assert engine.batch_bytes(a.handle) == engine.batch_bytes(b.handle) and a.lengths.tolist() == b.lengths.tolist()
            a.release()
    finally:
        for b in (h, r, q) + cols:
            b.release()


# ---- refusals that need a device

def test_refusals(engine):
    seqs = [b"ACGT", b"", b"GG"]
    a = upload(engine, seqs)
    short = upload(engine, seqs[:2])
    plain = engine.upload(b"ACGTACGTACGTACGTACGTACGTACGT")
    other = _native.Engine()
    alien = upload(other, seqs)
    try:
        with pytest.raises(ValueError, match="column 1 is no live batch handle of this context"):
            engine.format_batch([a, alien], (b"", b"", b"\n"))
        with pytest.raises(ValueError, match="column 1 has 2 sequences, column 0 has 3"):
            engine.format_batch([a, short], (b"", b"", b"\n"))
        plain.n_seqs = 3
        with pytest.raises(ValueError, match="column 0 is no batch handle"):
            engine.format_batch([plain], (b"", b"\n"))
        with pytest.raises(ValueError, match="literal 1 is longer"):
            engine.format_batch([a], (b"", b"x" * 256))
        with pytest.raises(ValueError, match="columns checked for equal length are columns"):
            engine.format_batch([a], (b"", b"\n"), (0, 1))
        gone = upload(engine, seqs)
        stale = _native.ResidentSequence(engine, ctypes.c_void_p(gone._h.value), gone.nbytes)
        stale.n_seqs = 3
        gone.release()
        with pytest.raises(ValueError, match="column 0 is no live batch handle"):
            engine.format_batch([stale], (b"", b"\n"))
        stale._h = None
        # cap too small, at the C-ABI: FZ_EINVAL, the buffer untouched
        buf = np.full(16, 0xAB, dtype=np.uint8)
        hs = (ctypes.c_void_p * 1)(a._h.value)
        lens = np.array([0, 1], dtype=np.uint32)
        info = _native.FzFormatInfo()
        call = lambda cap: engine._lib.fz_batch_format(engine._h, hs, 1, b"\n", lens.ctypes.data, _native.FORMAT_NO_CHECK, _native.FORMAT_NO_CHECK,
                                                       buf.ctypes.data, cap, ctypes.byref(info))
        assert call(8) == _native.FZ_EINVAL and info.text_bytes == 9 and (buf == 0xAB).all()
        assert b"smaller than the text" in engine._lib.fz_last_error()
        assert call(9) == _native.FZ_OK and buf[:9].tobytes() == b"ACGT\n\nGG\n" and (buf[9:] == 0xAB).all()
        engine.lev_ngrams_begin(plain, b"ACGTACGTACGTACGTACGT", 2)          # a pipelined search outstanding: as the uploads
        try:
            with pytest.raises(ValueError, match="in flight"):
                engine.format_batch([a], (b"", b"\n"))
            with pytest.raises(ValueError, match="in flight"):
                engine.upload_records_lines(b"@r\nAC\n+\nII\n", 4, (0, 1, 3), 1)
        finally:
            assert len(engine.lev_ngrams_end()) >= 1
        assert engine.format_batch([a], (b"", b"\n")).tobytes() == b"ACGT\n\nGG\n"
    finally:
        for h in (a, short, plain, alien):
            h.release()
        other.close()


def test_timing_spans(engine):
    text, _cols = canonical_fastq(2000, seed=24)
    cols = fa.resident_records(text, engine=engine, lines=(0, 1, 3))
    try:
        up = engine.records_ms()
        assert all(np.isfinite(v) and v >= 0 for v in up.values()) and up["kernels"] > 0 and up["h2d"] > 0 and up["call"] > 0, up
        assert fa.format_records(cols, "fastq").tobytes() == text
        ms = engine.format_ms()
        assert sorted(ms) == ["call", "desc_h2d", "gather", "measure_scan", "text_d2h"]
        assert all(np.isfinite(v) and v >= 0 for v in ms.values()) and ms["gather"] > 0 and ms["measure_scan"] > 0 and ms["call"] > 0, ms
    finally:
        for b in cols:
            b.release()
