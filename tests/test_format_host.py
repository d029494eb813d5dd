"""format_records, host side (CPU only): the measure step and scan of fz_batch_format run on the host through the function the
kernel runs (fz_debug_format_plan) against the three-line model (tests/format_model.py), the gather's address rule compiled
with g++ (tests/format_emul.cpp, a stand-alone program; once more under the host sanitizers), and the Python layer over a
stub engine."""
import mmap
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fuzzysearch_amd as fa
from fuzzysearch_amd import _native, egress, records
from fuzzysearch_amd.batch import BatchSequences
from tests import format_model as fmod

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the plan against the model

def plan(cols, lits, equal=None):
    offs, seen = [], {}
    for c in cols:                                                      # a column passed twice: the same table twice
        if id(c) not in seen:
            seen[id(c)] = np.array(fmod.offsets(c), dtype=np.uint64)
        offs.append(seen[id(c)])
    return _native.format_plan(offs, [len(l) for l in lits], equal)


def check_plan(cols, lits, equal=None):
    at, info = plan(cols, lits, equal)
    want = fmod.starts(cols, lits)
    assert at.tolist() == want
    assert info["n_records"] == len(cols[0]) and info["text_bytes"] == want[-1] == len(fmod.model(cols, lits))
    assert info["longest_record"] == max([b - a for a, b in zip(want, want[1:])] or [0])
    assert (info["bad_record"], info["bad_reason"]) == (0, 0)


def test_presets_are_the_models():
    assert _native.FORMAT_PRESETS == fmod.PRESETS == egress.FORMATS
    assert (_native.FORMAT_MAX_COLUMNS, _native.FORMAT_MAX_LITERAL, _native.FORMAT_NO_CHECK) == (8, 255, 0xffffffff)


@pytest.mark.parametrize("preset", sorted(fmod.PRESETS))
def test_plan_of_every_preset(preset):
    rnd = fmod.rng(1)
    lits, equal = fmod.PRESETS[preset]
    if preset == "fastq":
        cols = list(fmod.fastq_columns(rnd, 300))
    else:
        cols = fmod.random_columns(rnd, len(lits) - 1, 300)
    check_plan(cols, lits, equal)


def test_plan_degenerate_cases():
    rnd = fmod.rng(2)
    check_plan([[b""] * 5], (b"", b""))                                 # a text of 0 bytes
    check_plan([[b""] * 5, [b""] * 5], (b"ab", b"", b"\n"))             # empty sequences, literals only
    check_plan([[]], (b"x", b"\n"))                                     # n = 0
    check_plan([[b"ACGT"]], (b"", b"\n"))                               # one record
    col = fmod.random_columns(rnd, 1, 70)[0]
    check_plan([col, col], (b"", b"\t", b"\n"), (0, 1))                 # a column passed twice, checked against itself
    cols = fmod.random_columns(rnd, 8, 40)
    check_plan(cols, tuple(bytes([65 + i]) * (i * 31 % 256) for i in range(9)))   # eight columns, long literals
    check_plan([col], (b"x" * 255, b"y" * 255))


def test_plan_reports_the_lower_of_two_bad_records():
    rnd = fmod.rng(3)
    heads, reads, quals = fmod.fastq_columns(rnd, 3000)
    lits, equal = fmod.PRESETS["fastq"]
    for bad in ([0], [2999], [1234, 2500], [2500, 7]):
        q = list(quals)
        for j in bad:
            q[j] = q[j] + b"I"
        assert fmod.first_bad([heads, reads, q], equal) == (min(bad), 1)
        with pytest.raises(ValueError, match=r"format: record %d: the two columns checked" % min(bad)) as e:
            plan([heads, reads, q], lits, equal)
        assert (e.value.info["bad_record"], e.value.info["bad_reason"]) == (min(bad), 1)
        check_plan([heads, reads, q], lits, None)                       # ... and without the check it is a text
    check_plan([heads, reads, quals], lits, equal)


def test_plan_refusals():
    col = np.array([0, 3, 5], dtype=np.uint64)
    with pytest.raises(ValueError, match="literal 1 is longer"):
        _native.format_plan([col], [0, 256])
    with pytest.raises(ValueError, match="columns"):
        _native.format_plan([col] * 9, [0] * 10)
    with pytest.raises(ValueError, match="columns checked"):
        _native.format_plan([col], [0, 1], (0, 1))
    with pytest.raises(ValueError, match="numbers of sequences"):
        _native.format_plan([col, col[:2]], [0, 1, 1])


# ---- the gather's address rule

@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_gather_address_rule_at_every_alignment_and_length(flags):
    exe = os.path.join(tempfile.gettempdir(), "fz_format_emul_%d_%d" % (os.getpid(), len(flags)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + [os.path.join(HERE, "format_emul.cpp"), "-o", exe])
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    finally:
        os.unlink(exe)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", str(3 * 4 * 16 * 16 * 41)]


# ---- the Python layer over a stub engine

class Handle(object):
    def __init__(self, seqs):
        self.seqs, self._h, self.n_seqs, self.nbytes = seqs, object(), len(seqs), sum(map(len, seqs))

    def __len__(self):
        return self.nbytes

    def release(self):
        self._h = None


class StubEngine(object):
    """A single-device engine that formats by the model and writes every call down."""
    devices = [0]

    def __init__(self):
        self.calls = []

    def comm_info(self):
        return 0, 0, False

    def upload_batch(self, blob, offs):
        return Handle([bytes(blob[int(a):int(b)]) for a, b in zip(offs, offs[1:])])

    def upload_records(self, *a):
        self.calls.append(("upload_records",) + a[1:])
        return Handle([])

    def batch_tables(self, handle):
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)

    def format_batch(self, handles, literals, equal, out):
        self.calls.append(("format_batch", len(handles), tuple(literals), equal, out.size))
        text = fmod.model([h.seqs for h in handles], literals)
        assert len(text) <= out.size
        out[:len(text)] = np.frombuffer(text, dtype=np.uint8)
        return out[:len(text)]


def held(engine, seqs):
    return BatchSequences(seqs, engine=engine)


def test_format_records_sizes_the_text_and_calls_the_engine_once():
    eng = StubEngine()
    heads, reads, quals = fmod.fastq_columns(fmod.rng(4), 50)
    cols = [held(eng, c) for c in (heads, reads, quals)]
    want = fmod.model([heads, reads, quals], fmod.PRESETS["fastq"][0])
    got = fa.format_records(cols, "fastq")
    assert got.dtype == np.uint8 and got.tobytes() == want
    assert eng.calls == [("format_batch", 3, fmod.PRESETS["fastq"][0], (1, 2), len(want))]      # the size: known before the call
    eng.calls.clear()
    assert fa.format_records(cols[1], "lines").tobytes() == b"".join(r + b"\n" for r in reads)
    assert cols[1].format().tobytes() == b"".join(r + b"\n" for r in reads)
    assert cols[1].format(literals=(b"<", b">")).tobytes() == b"".join(b"<" + r + b">" for r in reads)
    assert fa.format_records(cols[:2], "fasta").tobytes() == fmod.model([heads, reads], fmod.PRESETS["fasta"][0])
    assert fa.format_records([cols[0], cols[1], cols[1]], literals=(b"", b"\t", b"\t", b"\n")).tobytes() == \
        fmod.model([heads, reads, reads], (b"", b"\t", b"\t", b"\n"))
    assert [c[4] for c in eng.calls] == [len(b"".join(reads)) + 50, len(b"".join(reads)) + 50, len(b"".join(reads)) + 100,
                                         len(b"".join(heads + reads)) + 150, len(b"".join(heads + reads + reads)) + 150]


def test_every_refusal_comes_before_any_engine_call():
    eng, other = StubEngine(), StubEngine()
    a, b = held(eng, [b"AC", b"G"]), held(eng, [b"II", b"I"])
    short, alien, text = held(eng, [b"AC"]), held(other, [b"AC", b"G"]), held(eng, ["AC", "G"])
    gone = held(eng, [b"AC", b"G"])
    gone.release()
    cases = [(TypeError, "exactly one", lambda: fa.format_records(a)),
             (TypeError, "exactly one", lambda: fa.format_records(a, "lines", (b"", b"\n"))),
             (ValueError, "unknown format", lambda: fa.format_records(a, "bam")),
             (ValueError, "takes 3 columns", lambda: fa.format_records([a, b], "fastq")),
             (ValueError, "takes 1 columns", lambda: fa.format_records([a, b], "lines")),
             (ValueError, "takes 2 columns", lambda: fa.format_records(a, "fasta")),
             (ValueError, "between 1 and 8", lambda: fa.format_records([], literals=(b"",))),
             (ValueError, "between 1 and 8", lambda: fa.format_records([a] * 9, literals=(b"",) * 10)),
             (ValueError, "take 3 literals", lambda: fa.format_records([a, b], literals=(b"", b"\n"))),
             (ValueError, "literal 1 is longer", lambda: fa.format_records(a, literals=(b"", b"x" * 256))),
             (TypeError, None, lambda: fa.format_records(a, literals=(b"", "\n"))),
             (TypeError, "resident batches", lambda: fa.format_records([a, [b"II", b"I"]], literals=(b"", b"", b""))),
             (ValueError, "column 1 has 1 sequences", lambda: fa.format_records([a, short], literals=(b"", b"", b""))),
             (ValueError, "column 1 has been released", lambda: fa.format_records([a, gone], literals=(b"", b"", b""))),
             (ValueError, "another engine", lambda: fa.format_records([a, alien], literals=(b"", b"", b""))),
             (TypeError, "batch of str", lambda: fa.format_records(text, "lines")),
             (ValueError, "out holds 4 bytes, the text has 5", lambda: fa.format_records(a, "lines", out=bytearray(4))),
             (ValueError, "read-only", lambda: fa.format_records(a, "lines", out=bytes(8))),
             (TypeError, "single bytes", lambda: fa.format_records(a, "lines", out=np.zeros(8, dtype=np.uint16))),
             (TypeError, "exactly one", lambda: fa.write_records("/nonexistent/x", a))]
    for exc, match, call in cases:
        with pytest.raises(exc, match=match):
            call()
    assert eng.calls == [] and other.calls == []


def test_out_is_filled_in_place_and_a_view_of_it_returned():
    eng = StubEngine()
    a = held(eng, [b"AC", b"G"])
    buf = bytearray(b"." * 9)
    got = fa.format_records(a, "lines", out=buf)
    assert got.tobytes() == b"AC\nG\n" and bytes(buf) == b"AC\nG\n...." and np.shares_memory(got, np.frombuffer(buf, dtype=np.uint8))
    arr = np.full(5, 46, dtype=np.uint8)
    assert fa.format_records(a, "lines", out=arr).base is not None and arr.tobytes() == b"AC\nG\n"


def test_write_records(tmp_path):
    eng = StubEngine()
    heads, reads, quals = fmod.fastq_columns(fmod.rng(5), 40)
    cols = [held(eng, c) for c in (heads, reads, quals)]
    path = str(tmp_path / "out.fastq")
    want = fmod.model([heads, reads, quals], fmod.PRESETS["fastq"][0])
    assert fa.write_records(path, cols, format="fastq") == len(want)
    assert open(path, "rb").read() == want
    assert fa.write_records(path, cols[1], literals=(b"", b"\n")) == len(b"".join(reads)) + 40      # an existing file is replaced
    assert open(path, "rb").read() == b"".join(r + b"\n" for r in reads)
    eng.calls.clear()
    empty = held(eng, [b"", b"", b""])
    assert fa.write_records(path, empty, literals=(b"", b"")) == 0 and os.path.getsize(path) == 0     # 0 bytes: no mapping, no call
    assert eng.calls == []
    nothing = BatchSequences.__new__(BatchSequences)                    # n = 0 with a handle
    nothing.sequences, nothing.engine, nothing.kind, nothing.handle = [], eng, "bytes", Handle([])
    assert fa.write_records(path, nothing, format="lines") == 0 and os.path.getsize(path) == 0

    def refuse(*a):
        raise ValueError("format: record 3: %s" % egress._REASONS[1])
    eng.format_batch = refuse
    with pytest.raises(ValueError, match="record 3"):
        fa.write_records(path, cols, format="fastq")
    assert not os.path.exists(path)                                     # a refused text leaves no file


class SeveralDevices(object):
    """Stands in for an engine the batched calls do not serve."""
    devices = [0, 1]

    def comm_info(self):
        return 0, 0, False

    def __getattr__(self, name):
        raise AssertionError("an engine of several devices is not called: %s" % name)


def test_columns_without_a_handle_are_joined_in_python(tmp_path):
    eng = SeveralDevices()
    heads, reads, quals = fmod.fastq_columns(fmod.rng(6), 30)
    cols = [held(eng, c) for c in (heads, reads, quals)]
    assert all(c.handle is None for c in cols)
    want = fmod.model([heads, reads, quals], fmod.PRESETS["fastq"][0])
    assert fa.format_records(cols, "fastq").tobytes() == want
    buf = bytearray(len(want) + 3)
    assert fa.format_records(cols, "fastq", out=buf).tobytes() == want and bytes(buf[:len(want)]) == want
    path = str(tmp_path / "host.fastq")
    assert fa.write_records(path, cols, "fastq") == len(want) and open(path, "rb").read() == want
    quals[7] += b"I"
    quals[20] += b"I"
    bad = [cols[0], cols[1], held(eng, quals)]
    with pytest.raises(ValueError, match=r"^format: record 7: the two columns checked for equal length differ in length$"):
        fa.format_records(bad, "fastq")
    assert fa.format_records(bad, literals=fmod.PRESETS["fastq"][0]).tobytes() == fmod.model([heads, reads, quals], fmod.PRESETS["fastq"][0])
    text = fmod.model([heads, reads, [b"I" * len(r) for r in reads]], fmod.PRESETS["fastq"][0])
    h, r, q = fa.resident_records(text, engine=eng, lines=(0, 1, 3))    # split in Python, line by line
    assert (h.line, r.line, q.line) == (0, 1, 3) and h.source is r.source is q.source
    assert list(h.sequences) == heads and list(r.sequences) == reads and [len(x) for x in q.sequences] == [len(x) for x in reads]
    assert fa.format_records((h, r, q), "fastq").tobytes() == text
    assert r.lengths.tolist() == [len(x) for x in reads] and text[int(q.starts[3]):].startswith(b"I" * len(reads[3]))


def test_the_python_words_are_the_library_s():
    col = np.array([0, 1], dtype=np.uint64)
    with pytest.raises(ValueError) as e:
        _native.format_plan([col, np.array([0, 2], dtype=np.uint64)], [0, 0, 0], (0, 1))
    assert str(e.value) == "format: record 0: %s" % egress._REASONS[1]


def test_lines_none_makes_exactly_today_s_upload_call():
    eng = StubEngine()
    b = fa.resident_records(b"@r\nAC\n+\nII\n", engine=eng)
    assert isinstance(b, fa.RecordBatch) and b.line == 1 and eng.calls == [("upload_records", 4, 1, 1)]
    eng.calls.clear()
    assert fa.resident_records(b"AC\nG\n", format="lines", engine=eng).line == 0 and eng.calls == [("upload_records", 1, 0, 0)]
    assert _native.RECORD_FORMATS == {"fastq": (4, 1, 1), "lines": (1, 0, 0)}


def test_resident_records_lines_arguments():
    eng = StubEngine()
    made = []

    def upload_records_lines(text, period, kept, flags):
        made.append((bytes(text), period, list(kept), flags))
        return [Handle([]) for _ in kept]
    eng.upload_records_lines = upload_records_lines
    text = b"@r\nAC\n+\nII\n"
    out = fa.resident_records(text, engine=eng, lines=(3, 0))
    assert isinstance(out, tuple) and [b.line for b in out] == [3, 0] and all(isinstance(b, fa.RecordBatch) for b in out)
    assert made == [(text, 4, [3, 0], 1)] and out[0].source is out[1].source and out[0].kind == "bytes"
    assert [b.line for b in fa.resident_records(b"AC\n", format="lines", engine=eng, lines=(0,))] == [0]
    for lines, match in (((0, 0), "twice"), ((4,), "lines 0 .. 3"), ((-1,), "lines 0 .. 3"), ((), "between 1 and 4"),
                         ((0, 1, 2, 3, 1), "between 1 and 4")):
        with pytest.raises(ValueError, match=match):
            fa.resident_records(text, engine=eng, lines=lines)
    with pytest.raises(ValueError, match="between 1 and 1|lines 0 .. 0"):
        fa.resident_records(b"AC\n", format="lines", engine=eng, lines=(0, 1))
    with pytest.raises(ValueError, match="lines 0 .. 0"):
        fa.resident_records(b"AC\n", format="lines", engine=eng, lines=(1,))
    with pytest.raises(ValueError, match="unknown record format"):
        fa.resident_records(text, format="bam", engine=eng, lines=(0,))
    assert len(made) == 2
    starts, lengths = records.split_records(text, "fastq")              # today's default: the sequence line
    assert (starts.tolist(), lengths.tolist()) == ([3], [2])
    assert [t.tolist() for t in records.split_records(text, "fastq", 0)] == [[0], [2]]
    assert [t.tolist() for t in records.split_records(text, "fastq", 3)] == [[8], [2]]


def test_exports():
    assert {"format_records", "write_records"} <= set(fa.__all__)
    assert fa.format_records is egress.format_records and fa.write_records is egress.write_records
    new = ("fz_batch_upload_records_lines", "fz_batch_format", "fz_debug_format_plan", "fz_debug_format_ms")
    assert set(new) <= set(_native.EXPORTED_SYMBOLS) and set(new) <= _native.OPTIONAL
    lib = _native.load_library()
    assert all(hasattr(lib, name) for name in new)
    assert ctypes_size() == 40


def ctypes_size():
    import ctypes
    return ctypes.sizeof(_native.FzFormatInfo)
